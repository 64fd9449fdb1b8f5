"""`python -m mt3_amd.transcribe --harmony` in a fresh child process, on the trained fixture: NAME.harmony.json agrees with
`harmony.analyze` on the decoded notes, and NAME.mid reads back with the key signature, the time signature and the chord
markers the JSON holds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import beats, harmony, inference, midi_io, synthetic, transcribe  # noqa: E402
from tests import pcm_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    _, y16 = synthetic.synth_music(3 * 2.048 + 0.7, seed=21, device="cpu")
    y16 = np.clip(np.asarray(y16, np.float64), -1.0, 1.0)
    _, tag, bits, _ = pc.FORMATS["s16"]
    wav = str(tmp_path_factory.mktemp("wavs") / "first.wav")
    with open(wav, "wb") as f:
        f.write(pc.wav_file(16000, 1, tag, bits, np.rint(y16[:, None] * 32767).astype("<i2").tobytes()))
    out = tmp_path_factory.mktemp("out")
    done = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", CKPT, "--harmony", "-o", str(out), wav],
                          cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    ns = inference.InferenceModel(CKPT, "mt3").transcribe_wavs([wav])[0]
    return out, ns


def test_harmony_json_agrees_with_the_analysis_of_the_decoded_notes(outputs):
    out, ns = outputs
    found = beats.track([ns])[0]
    h = harmony.analyze([ns], [found])[0]
    assert len(ns.notes) >= 5 and len(found.frames) >= 2 and len(h.chords) == len(found.frames)
    with open(out / "first.harmony.json") as f:
        rec = json.load(f)
    assert rec == json.loads(json.dumps(transcribe.harmony_record(h)))
    assert sorted(rec) == ["beats_per_bar", "chords", "downbeat", "downbeats", "key", "key_name", "sharps"]
    assert sorted(os.listdir(out)) == ["first.beats.json", "first.harmony.json", "first.mid"]


def test_the_midi_file_reads_back_to_the_json(outputs):
    out, ns = outputs
    found = beats.track([ns])[0]
    with open(out / "first.harmony.json") as f:
        rec = json.load(f)
    with open(out / "first.mid", "rb") as f:
        data = f.read()
    h = harmony.analyze([ns], [found])[0]
    assert data == midi_io.note_sequence_to_midi_bytes(ns, beats=found.times, harmony=h)
    read = midi_io.midi_bytes_to_signatures(data)
    assert read["key_signatures"] == ([(0.0, rec["sharps"], rec["key"] % 2)] if rec["key"] >= 0 else [])
    assert read["time_signatures"] == ([(0.0, rec["beats_per_bar"], 4)] if rec["beats_per_bar"] else [])
    m, t0 = midi_io.preroll(found.times, h)
    if rec["beats_per_bar"]:
        assert (m + rec["downbeat"]) % rec["beats_per_bar"] == 0             # tick 0 is a downbeat
    assert [text for _, text in read["markers"]] == ["N.C." if name == "N" else name for _, _, name in rec["chords"]]
    assert np.allclose([t + t0 for t, _ in read["markers"]], [start for start, _, _ in rec["chords"]], rtol=0, atol=1e-9)
    assert len(midi_io.midi_bytes_to_note_sequence(data).notes) == len(ns.notes)
