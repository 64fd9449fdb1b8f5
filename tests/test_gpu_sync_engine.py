"""`InferenceModel.synchronize` on the end-to-end piece of test_sync_ref with the trained fixture's frontend, a job of
three pairs, the sustain pedal, and `python -m mt3_amd.transcribe --sync-midi` in a fresh child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import audio_io, inference, midi_io, sync  # noqa: E402
from mt3_amd import note_sequences as N  # noqa: E402
from tests import sync_cases as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")


@pytest.fixture(scope="module")
def model():
    return inference.InferenceModel(CKPT, "mt3")


@pytest.fixture(scope="module")
def synced(model):
    score, played, wav = SC.piece()
    return model.synchronize(wav, score)


def test_the_onsets_are_within_the_bound_of_the_numpy_rule(synced):
    """the bound: sync_cases.BOUND, measured with the numpy rules on the oracle's log-mel plus one feature frame"""
    score, played, _ = SC.piece()
    err = SC.onset_errors(synced["notes"], played)
    print("onset error on the device: max %.4f s, median %.4f s (bound %.4f s)" % (err.max(), np.median(err), SC.BOUND))
    assert err.max() <= SC.BOUND
    assert len(synced["notes"].notes) == len(score.notes) and synced["fps"] == 25.0
    assert all(a.pitch == b.pitch and a.velocity == b.velocity for a, b in zip(synced["notes"].notes, score.notes))
    assert all(n.end_time >= n.start_time for n in synced["notes"].notes)
    pi, pj = synced["path_frames"]
    assert (pi[0], pj[0]) == (0, 0) and set(zip(np.diff(pi).tolist(), np.diff(pj).tolist())) <= {(1, 1), (1, 0), (0, 1)}
    assert synced["mean_cost"] == synced["total"] / len(pi) and 0.9 < synced["tempo_ratio"] < 1.1


def test_the_device_features_give_the_reference_path(model, synced):
    """the product's frontend, then the numpy rules: the same path as the three ops"""
    score, _, wav = SC.piece()
    _, logmel = model._examples(wav, 16000)
    n_frames = model._num_frames(wav)
    from mt3_amd import spectrograms
    bins = sync.chroma_bins(spectrograms.mel_matrix())
    rec = SC.numpy_synchronize(logmel.reshape(-1, logmel.shape[-1])[:n_frames].cpu().numpy(), score, bins)
    assert rec["total"] == synced["total"]
    assert np.array_equal(rec["path_frames"][0], synced["path_frames"][0])
    assert np.array_equal(rec["path_frames"][1], synced["path_frames"][1])


def test_three_pairs_as_one_job_equal_three_calls(model, synced):
    score, played, wav = SC.piece()
    short = N.NoteSequence(notes=[n for n in score.notes if n.end_time < 6.0])
    pairs = [(wav, score), (wav[: 7 * 16000], short), (wav[: 3000], N.NoteSequence())]
    many = model.synchronize_many(pairs, pool=4, harmonic_weights=(255, 128, 64))
    for (audio, ns), got in zip(pairs, many):
        one = model.synchronize(audio, ns, pool=4, harmonic_weights=(255, 128, 64))
        assert got["total"] == one["total"] and got["tempo_ratio"] == one["tempo_ratio"]
        assert np.array_equal(got["path_frames"][0], one["path_frames"][0])
        assert np.array_equal(got["path_frames"][1], one["path_frames"][1])
        assert got["notes"] == one["notes"]
    assert many[2]["total"] == 0 and len(many[2]["path"][0]) == 0 and many[2]["notes"].notes == []
    assert many[0]["fps"] == 31.25 and many[0]["total"] != synced["total"]


def test_slices_of_one_log_mel_tensor_are_one_job(model):
    """the files' blocks back to back in ONE tensor (the engine's job; `velocity.estimate`'s documented form): the op is
    given the first slice and the job's rows, and every file equals its single call"""
    score, _, wav = SC.piece()
    _, logmel = model._examples(wav, 16000)
    whole = torch.cat([logmel, logmel[:4], logmel[:2]], 0).contiguous()
    S = logmel.shape[0]
    slices = [whole[:S], whole[S: S + 4], whole[S + 4:]]
    assert slices[1].data_ptr() == slices[0].data_ptr() + slices[0].numel() * 4
    T = logmel.shape[1]
    short = N.NoteSequence(notes=[n for n in score.notes if n.end_time < 7.0])
    shorter = N.NoteSequence(notes=[n for n in score.notes if n.end_time < 3.0])
    frames = [model._num_frames(wav), 4 * T - 17, 2 * T]
    many = sync.synchronize(list(zip(slices, frames)), [score, short, shorter])
    for piece, n, ns, got in zip(slices, frames, [score, short, shorter], many):
        one, = sync.synchronize([(piece.clone(), n)], [ns])
        assert got["total"] == one["total"] > 0 and got["notes"] == one["notes"]
        assert np.array_equal(got["path_frames"][0], one["path_frames"][0])
        assert np.array_equal(got["path_frames"][1], one["path_frames"][1])


def test_sustain_runs(model):
    score, played, wav = SC.piece()
    pedalled = N.NoteSequence(notes=list(score.notes), total_time=score.total_time,
                              control_changes=[N.ControlChange(2.0, 64, 127, 0), N.ControlChange(4.0, 64, 0, 0)])
    rec = model.synchronize(wav, pedalled, sustain=True)
    assert len(rec["notes"].notes) > 0 and rec["total"] > 0
    assert SC.onset_errors(rec["notes"], N.NoteSequence(notes=played.notes[: len(rec["notes"].notes)])).shape[0] > 0


def test_the_command_line_writes_its_two_files(model, synced, tmp_path):
    score, _, wav = SC.piece()
    wav_path, out = str(tmp_path / "piece.wav"), tmp_path / "out"
    scores = tmp_path / "scores"
    scores.mkdir()
    with open(wav_path, "wb") as f:
        f.write(audio_io.samples_to_wav_data(wav, 16000))
    midi_io.note_sequence_to_midi_file(score, str(scores / "piece.mid"))
    done = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", CKPT, "--sync-midi", str(scores),
                           "-o", str(out / "piece.mid"), wav_path], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    record, = json.load(open(out / "sync.json"))
    # what the command line synchronises: the WAV's int16 samples and the MIDI file's notes, on its tick grid
    samples, rate = audio_io.read_wav(wav_path)
    with open(scores / "piece.mid", "rb") as f:
        read = midi_io.midi_bytes_to_note_sequence(f.read())
    want = model.synchronize(samples, read, sample_rate=rate)
    assert record["audio"] == wav_path and record["total"] == want["total"]
    assert record["mean_cost"] == want["mean_cost"] and record["tempo_ratio"] == want["tempo_ratio"]
    seconds = [int(a) for a, _ in record["path"][:-1]]
    assert seconds == sorted(set(seconds)) and len(record["path"]) <= int(len(wav) / 16000) + 2
    with open(out / "piece.synced.mid", "rb") as f:
        back = midi_io.midi_bytes_to_note_sequence(f.read())
    expect = midi_io.midi_bytes_to_note_sequence(midi_io.note_sequence_to_midi_bytes(want["notes"]))
    assert back.notes == expect.notes and len(back.notes) == len(score.notes)
    assert os.path.isfile(out / "piece.mid")
