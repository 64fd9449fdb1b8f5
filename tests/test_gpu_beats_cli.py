"""`python -m mt3_amd.transcribe --beats --quantize 4` in a fresh child process, on the trained fixture and a two-file job
(a 16 kHz mono and a 44.1 kHz stereo int16 file): NAME.beats.json agrees with `beats.track` on the decoded notes, NAME.mid
reads back with the tempo map, and without --beats the files have the bytes they always had."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import audio_io, beats, inference, midi_io, synthetic  # noqa: E402
from tests import pcm_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")
NAMES = ("first", "second")


def _run(*args):
    done = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", CKPT, *args], cwd=ROOT,
                          capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    _, y16 = synthetic.synth_music(3 * 2.048 + 0.7, seed=21, device="cpu")
    y16 = np.clip(np.asarray(y16, np.float64), -1.0, 1.0)
    y44 = np.clip(audio_io.resample(y16.astype(np.float32), 16000, 44100), -1.0, 1.0).astype(np.float64)
    _, tag, bits, _ = pc.FORMATS["s16"]
    d = tmp_path_factory.mktemp("wavs")
    wavs = [str(d / (name + ".wav")) for name in NAMES]
    with open(wavs[0], "wb") as f:
        f.write(pc.wav_file(16000, 1, tag, bits, np.rint(y16[:, None] * 32767).astype("<i2").tobytes()))
    with open(wavs[1], "wb") as f:
        f.write(pc.wav_file(44100, 2, tag, bits, np.rint(np.stack([y44, 0.9 * y44], 1) * 32767).astype("<i2").tobytes()))
    plain, mapped = tmp_path_factory.mktemp("plain"), tmp_path_factory.mktemp("mapped")
    _run("-o", str(plain), *wavs)
    _run("--beats", "--quantize", "4", "-o", str(mapped), *wavs)
    sequences = inference.InferenceModel(CKPT, "mt3").transcribe_wavs(wavs)
    return plain, mapped, sequences


def test_beats_json_agrees_with_the_tracker_on_the_decoded_notes(outputs):
    _, mapped, sequences = outputs
    found = beats.track(sequences)
    assert all(same.period == ref.period and np.array_equal(same.frames, ref.frames)
               for same, ref in zip(found, beats.track_reference(sequences)))
    for name, ns, b in zip(NAMES, sequences, found):
        assert len(ns.notes) >= 5
        with open(mapped / (name + ".beats.json")) as f:
            rec = json.load(f)
        assert sorted(rec) == ["beats", "period_frames", "qpm"]
        assert rec["beats"] == [float(t) for t in b.times] and rec["period_frames"] == b.period and rec["qpm"] == b.qpm
    assert sorted(os.listdir(mapped)) == sorted(n + e for n in NAMES for e in (".mid", ".beats.json"))


def test_the_midi_file_reads_back_with_the_tempo_map(outputs):
    _, mapped, sequences = outputs
    found = beats.track(sequences)
    snapped = beats.snap(sequences, found, 4)
    assert any(len(b.times) >= 2 for b in found)
    for name, ns, b in zip(NAMES, snapped, found):
        with open(mapped / (name + ".mid"), "rb") as f:
            data = f.read()
        if len(b.times) < 2:                                                # no beats: the constant tempo, as ever
            assert data == midi_io.note_sequence_to_midi_bytes(ns)
            continue
        assert data == midi_io.note_sequence_to_midi_bytes(ns, beats=b.times)
        m, t0 = midi_io.preroll(b.times)
        read = midi_io.midi_bytes_to_beats(data)
        # the tracker's beats lie on 10 ms frames: whole microseconds, which the tempo field holds exactly
        assert np.allclose(np.array(read[m: m + len(b.times)]) + t0, b.times[:len(read) - m], rtol=0, atol=1e-9)
        back = midi_io.midi_bytes_to_note_sequence(data)
        assert len(back.notes) == len(ns.notes)
        # quantised notes sit on quarter-note fractions: every onset is a whole number of ticks of resolution / 4
        res = back.ticks_per_quarter
        quarters = np.interp([n.start_time for n in back.notes], read, np.arange(len(read))) if len(read) > 1 else []
        assert np.allclose(np.asarray(quarters) * 4, np.rint(np.asarray(quarters) * 4), atol=4.0 / res)


def test_without_the_flag_the_files_have_the_bytes_they_always_had(outputs):
    plain, _, sequences = outputs
    assert sorted(os.listdir(plain)) == [n + ".mid" for n in NAMES]
    for name, ns in zip(NAMES, sequences):
        with open(plain / (name + ".mid"), "rb") as f:
            # tests/test_beats_ref.py pins this writer, without beats, to the bytes of the one before the tempo map
            assert f.read() == midi_io.note_sequence_to_midi_bytes(ns)
        assert not hasattr(ns, "beats")


def test_the_model_attaches_beats_on_request(outputs):
    _, _, sequences = outputs
    model = inference.InferenceModel(CKPT, "mt3")
    _, y16 = synthetic.synth_music(3 * 2.048 + 0.7, seed=21, device="cpu")
    ns = model(np.asarray(y16, np.float32), beats=True)
    ref = beats.track_reference([ns])[0]
    assert ns.beats.period == ref.period and np.array_equal(ns.beats.frames, ref.frames)
    assert np.array_equal(inference.InferenceModel.beats(ns).frames, ref.frames)
    plain = model(np.asarray(y16, np.float32))
    assert [(n.start_time, n.end_time, n.pitch) for n in plain.notes] == [(n.start_time, n.end_time, n.pitch) for n in ns.notes]
    with pytest.raises(ValueError, match="beats= takes"):
        model(np.asarray(y16, np.float32), beats={"bpm": 100})
