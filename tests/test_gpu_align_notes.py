"""`InferenceModel.align_notes` on the trained fixture checkpoint: the (segment, shift) table against `score_notes` bit
for bit, with the shared encoder pass and without; a piece whose second half is 0.1 s late, end to end; the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import alignment, audio_io, checkpoints, inference, midi_io, note_sequences, synthetic  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [-0.2, -0.1, 0.0, 0.1, 0.2]
T = 2.048                                                     # seconds per segment: 256 frames of 8 ms
CHANGE, DELAY = 8.192, 0.1


@pytest.fixture(scope="module")
def model():
    return inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32")


@pytest.fixture(scope="module")
def piece():
    return synthetic.synth_music(8.192, seed=21)


def _late_half(seconds=16.384, seed=23):
    """(the labels, the truth, the truth's audio): every note at or after CHANGE sounds DELAY later than its label says"""
    ns, _ = synthetic.synth_music(seconds, seed=seed)
    move = (lambda n: DELAY if n.start_time >= CHANGE else 0.0)
    truth = note_sequences.NoteSequence(notes=[note_sequences.Note(n.start_time + move(n), n.end_time + move(n), n.pitch,
                                                                   n.velocity, n.program, n.is_drum, 0) for n in ns.notes])
    amps = np.random.default_rng(seed + 1).uniform(0.3, 1.0, len(ns.notes))
    wav = synthetic.render_notes([n.start_time for n in truth.notes], [n.end_time for n in truth.notes],
                                 [n.pitch for n in truth.notes], amps, np.zeros(len(ns.notes), np.int64), 1,
                                 int(round(seconds * 16000)), seed=seed).reshape(-1).cpu().numpy()
    return ns, truth, wav


def test_the_table_is_score_notes_column_by_column(model, piece):
    ns, wav = piece
    shared = model.align_notes(wav, ns, shifts=GRID, return_table=True)
    replicated = model.align_notes(wav, ns, shifts=GRID, return_table=True, shared_encoder=False)
    assert shared["scores"].shape == (5, len(GRID)) and shared["scores"].dtype == np.float64
    assert np.array_equal(shared["scores"], replicated["scores"])
    for j, shift in enumerate(GRID):
        want = model.score_notes(wav, ns, shifts=[shift])["segment_scores"]
        assert np.array_equal(shared["scores"][:, j], want), (shift, shared["scores"][:, j].tolist(), want.tolist())
    for key in ("segment_shifts", "path_score", "flat_shift", "flat_score"):
        assert np.array_equal(shared[key], replicated[key]), key
    # the path and the flat path are the rule's, on that table
    table = shared["scores"].astype(np.float32)
    path, total = alignment.best_paths_reference(table, [5], GRID, alignment.DEFAULT_SMOOTHNESS)
    assert np.array_equal(shared["segment_shifts"], np.asarray(GRID)[path]) and shared["path_score"] == -total[0]
    flat, flat_total = alignment.best_paths_reference(table, [5], GRID, 0.0, 0.0)
    assert shared["flat_shift"] == GRID[flat[0]] and shared["flat_score"] == -flat_total[0]
    want = alignment.warp_notes(ns, shared["segment_shifts"], T)
    assert [(n.start_time, n.end_time, n.pitch) for n in shared["notes"].notes] == \
        [(n.start_time, n.end_time, n.pitch) for n in want.notes]


def test_a_late_second_half_is_found_and_repaired(model):
    """Segments 0 .. 3 lie wholly before the change and must sit at 0.0; segments 5 .. 8 wholly after it and must sit
    at 0.1; segment 4 starts AT the change (its first notes are the first late ones) and is left free."""
    ns, truth, wav = _late_half()
    out = model.align_notes(wav, ns, shifts=GRID, return_table=True)
    shifts = out["segment_shifts"]
    print("table [segment, shift] of log-probabilities:")
    for s, row in enumerate(out["scores"]):
        print("  segment %d: %s -> %+.1f" % (s, " ".join("%9.3f" % v for v in row), shifts[s]))
    print("path", shifts.tolist(), "path_score %.3f flat_shift %+.1f flat_score %.3f"
          % (out["path_score"], out["flat_shift"], out["flat_score"]))
    assert len(shifts) == 9
    changed = 4                                               # CHANGE / T
    assert np.all(shifts[:changed] == 0.0), shifts.tolist()
    assert np.all(shifts[changed + 1:] == DELAY), shifts.tolist()
    onset = (lambda seq: np.array([n.start_time for n in seq.notes]))
    before, after = np.abs(onset(ns) - onset(truth)).mean(), np.abs(onset(out["notes"]) - onset(truth)).mean()
    print("mean |onset error|: labels %.4f s, aligned %.4f s" % (before, after))
    assert after < before
    loss_before, loss_after = model.score_notes(wav, ns)["loss"], model.score_notes(wav, out["notes"])["loss"]
    print("score_notes loss: labels %.4f, aligned %.4f" % (loss_before, loss_after))
    assert loss_after < loss_before
    assert out["flat_score"] <= out["path_score"]
    assert all(b.end_time >= b.start_time and (b.pitch, b.velocity, b.program, b.is_drum) ==
               (a.pitch, a.velocity, a.program, a.is_drum) for a, b in zip(ns.notes, out["notes"].notes))


def test_many_files_are_one_job_and_refusals(model, piece):
    ns, wav = piece
    one = model.align_notes(wav, ns, shifts=GRID, return_table=True)
    two = model.align_notes_many([(wav, ns), (wav[: 3 * 32768 - 128], ns)], shifts=GRID, return_table=True)
    assert len(two) == 2 and np.array_equal(two[0]["scores"], one["scores"]) and two[1]["scores"].shape == (3, 5)
    assert np.array_equal(two[0]["segment_shifts"], one["segment_shifts"]) and two[0]["path_score"] == one["path_score"]
    with pytest.raises(ValueError):
        model.align_notes(wav, ns, max_shift=1.1, step=0.1)   # a path could jump by 2.2 s: more than a segment
    model.align_notes(wav, ns, max_shift=1.1, step=0.1, max_jump=0.5)
    with pytest.raises(ValueError):
        model.align_notes(wav, ns, shifts=[0.0, 0.0])
    with pytest.raises(ValueError):
        model.align_notes(wav, ns, smoothness=-1.0)
    fp8 = inference.InferenceModel.__new__(inference.InferenceModel)
    fp8.model_config = type("C", (), {"kv_dtype": "e4m3"})()
    with pytest.raises(ValueError):
        fp8.align_notes(wav, ns)


def test_command_line_align_midi(tmp_path, piece):
    ns, wav = piece
    refs = tmp_path / "refs"
    refs.mkdir()
    for name in ("b", "a"):
        (tmp_path / (name + ".wav")).write_bytes(audio_io.samples_to_wav_data(wav, 16000))
        midi_io.note_sequence_to_midi_file(ns, str(refs / (name + ".mid")))
    r = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", CKPT, "--align-midi", str(refs),
                        "--align-max-shift", "0.1", "--align-step", "0.05", "-o", str(tmp_path / "out"),
                        str(tmp_path / "b.wav"), str(tmp_path / "a.wav")], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "out" / "alignment.json") as f:
        records = json.load(f)
    assert [os.path.basename(x["audio"]) for x in records] == ["b.wav", "a.wav"]
    for x in records:
        assert len(x["segment_shifts"]) == 5 and np.isfinite(x["segment_shifts"]).all()
        assert all(np.isfinite(x[k]) for k in ("path_score", "flat_shift", "flat_score"))
        assert x["flat_score"] <= x["path_score"]
    for name in ("a", "b"):
        with open(tmp_path / "out" / (name + ".aligned.mid"), "rb") as f:
            got = midi_io.midi_bytes_to_note_sequence(f.read())
        assert len(got.notes) > 0
