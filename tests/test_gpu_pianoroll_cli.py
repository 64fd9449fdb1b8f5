"""`python -m mt3_amd.transcribe --pianoroll [FPS]`: an .npy per input beside its .mid, on the two-file job of
tests/test_gpu_pcm.py's command-line test (a 44.1 kHz stereo int16 file and a 48 kHz 24-bit stereo file of the same music).

The rolls are compared against `pianorolls` of the IN-PROCESS NoteSequences (`transcribe_wavs` on the same files, which
the existing test already shows to be what the command writes), not of the notes read back from the .mid: midi_io rounds
times to ticks of 1/440 s, and the decoder's times lie on a 10 ms grid on which many are exact frame boundaries at
62.5 frames/s (0.08 s = frame 5.0), so the rounding moves frame indices."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import audio_io, inference, pianoroll, synthetic, transcribe  # noqa: E402
from tests import pcm_cases as pc  # noqa: E402
from tests import pianoroll_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")


def _wav(name, channels, sr, raw, **kw):
    _, tag, bits, _ = pc.FORMATS[name]
    return pc.wav_file(sr, channels, tag, bits, raw, **kw)


@pytest.fixture(scope="module")
def two_files(tmp_path_factory):
    _, y16 = synthetic.synth_music(3 * 2.048 + 0.7, seed=21, device="cpu")
    y16 = np.clip(np.asarray(y16, np.float64), -1.0, 1.0)
    y44 = np.clip(audio_io.resample(y16.astype(np.float32), 16000, 44100), -1.0, 1.0).astype(np.float64)
    y48 = np.clip(audio_io.resample(y16.astype(np.float32), 16000, 48000), -1.0, 1.0).astype(np.float64)
    st44 = np.rint(np.stack([y44, 0.9 * y44], 1) * 32767).astype("<i2").tobytes()
    v = np.rint(np.stack([0.9 * y48, y48], 1) * (2 ** 23 - 1)).astype(np.int64)
    st48 = (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    d = tmp_path_factory.mktemp("wavs")
    a, b = d / "first.wav", d / "second.wav"
    a.write_bytes(_wav("s16", 2, 44100, st44))
    b.write_bytes(_wav("s24", 2, 48000, st48, extensible=True))
    return str(a), str(b)


@pytest.mark.parametrize("flag,fps", [(["--pianoroll"], 62.5), (["--pianoroll", "100"], 100.0)])
def test_pianoroll_flag_writes_the_job_s_rolls(two_files, tmp_path, flag, fps):
    out = tmp_path / "out"
    assert transcribe.main(["--checkpoint", CKPT, *flag, "-o", str(out), *two_files]) == 0
    sequences = inference.InferenceModel(CKPT, "mt3").transcribe_wavs(list(two_files))
    rolls = pianoroll.pianorolls(sequences, fps)
    for ns, roll, name in zip(sequences, rolls, ("first", "second")):
        assert (out / (name + ".mid")).exists()
        got = np.load(out / (name + ".npy"))
        assert len(ns.notes) >= 5 and got.dtype == np.uint16 and got.shape == tuple(roll.shape) and got.any()
        assert np.array_equal(got, roll.cpu().numpy().astype(np.uint16))
        assert np.array_equal(got.astype(np.float64), ref.pianoroll(ns, fps, False))


def test_without_the_flag_no_npy_appears(two_files, tmp_path):
    out = tmp_path / "out"
    assert transcribe.main(["--checkpoint", CKPT, "-o", str(out), *two_files]) == 0
    assert sorted(os.listdir(out)) == ["first.mid", "second.mid"]
