"""`python -m mt3_amd.transcribe --render [RATE]`: NAME.render.wav beside NAME.mid, whose samples are the render of the
notes IN that .mid (the command renders the notes as the file holds them, on its tick grid, so the file can be read back
and compared) to one int16 step: the device tolerance of 2^-16 is half a step, and the int16 conversion truncates."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from scipy.io import wavfile  # noqa: E402

from mt3_amd import audio_io, midi_io, synthetic, transcribe  # noqa: E402
from tests import render_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")


@pytest.fixture(scope="module")
def short_wav(tmp_path_factory):
    _, y = synthetic.synth_music(2.048 + 0.7, seed=21, device="cpu")
    path = tmp_path_factory.mktemp("wavs") / "tune.wav"
    path.write_bytes(audio_io.samples_to_wav_data(np.asarray(y, np.float32), 16000))
    return str(path)


def _check(out_dir, rate):
    with open(out_dir / "tune.mid", "rb") as f:
        ns = midi_io.midi_bytes_to_note_sequence(f.read())
    got_rate, pcm = wavfile.read(out_dir / "tune.render.wav")
    want = ref.wav_samples(ref.render(ns, rate))
    assert got_rate == rate and pcm.dtype == np.int16 and pcm.shape == want.shape
    if len(want):
        worst = int(np.abs(pcm.astype(np.int64) - want).max())
        print("%d notes, %d samples: max int16 difference %d" % (len(ns.notes), len(want), worst))
        assert worst <= 1
    return ns, pcm


def test_render_flag_on_random_weights(short_wav, tmp_path):
    out = tmp_path / "out"
    os.makedirs(out)
    assert transcribe.main(["--checkpoint", "random:0", "--render", "-o", str(out / "tune.mid"), short_wav]) == 0
    assert sorted(os.listdir(out)) == ["tune.mid", "tune.render.wav"]
    _check(out, 16000)


def test_render_flag_with_a_rate_beside_the_other_outputs(short_wav, tmp_path):
    out = tmp_path / "out"
    os.makedirs(out)
    assert transcribe.main(["--checkpoint", CKPT, "--render", "22050", "--pianoroll", "--well-formed",
                            "-o", str(out / "tune.mid"), short_wav]) == 0
    assert sorted(os.listdir(out)) == ["tune.mid", "tune.npy", "tune.render.wav"]
    ns, pcm = _check(out, 22050)
    assert len(ns.notes) >= 5 and 29489 <= np.abs(pcm).max() <= 29491        # real notes, peak 0.9


def test_without_the_flag_no_wav_appears(short_wav, tmp_path):
    out = tmp_path / "out"
    os.makedirs(out)
    assert transcribe.main(["--checkpoint", "random:0", "-o", str(out / "tune.mid"), short_wav]) == 0
    assert os.listdir(out) == ["tune.mid"]
