"""mt3_op_tokenize_notes on the device against mt3_notes_tokenize, the same rule on the host (include/mt3_hip.h, mt3t_*),
which tests/test_tokenize_ref.py holds against the recipe; then `InferenceModel.score_notes` on the trained fixture
checkpoint.  Every comparison of rows is ==."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import checkpoints, inference, midi_io, note_sequences, synthetic, tokenize, vocabularies  # noqa: E402
from tests import tokenize_cases  # noqa: E402

TIES, NOTES = note_sequences.NoteEncodingWithTiesSpec, note_sequences.NoteEncodingSpec
CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def files():
    return tokenize_cases.hand_made() + tokenize_cases.random_files() + tokenize_cases.spread_files(seeds=range(2))


def _same(device, host):
    for name in ("ids", "lengths", "truncated", "note_of", "is_onset"):
        got, want = getattr(device, name).cpu().numpy(), getattr(host, name)
        bad = np.argwhere(np.asarray(got != want).reshape(len(want), -1).any(1)).reshape(-1)
        assert bad.size == 0, (name, bad[:8].tolist(), got[bad[0]].tolist()[:40], want[bad[0]].tolist()[:40])
    assert np.array_equal(device.rows_of_file, host.rows_of_file)


def _codec(bins):
    return vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=bins))


def test_kernel_equals_the_host_rule_on_one_job_of_all_files(files):
    seqs, frames = [ns for _, ns, _ in files], [f for _, _, f in files]
    codec = _codec(1)
    device = tokenize.target_rows(seqs, frames, codec, TIES)
    host = tokenize.target_rows_host(seqs, frames, codec, TIES)
    assert len(set(frames)) > 3 and len(host.ids) > 100             # uneven files: the two tables are exercised
    assert host.truncated.sum() >= 1
    _same(device, host)
    empty = host.rows_of_file[0, 0]
    assert [host.ids[r, :2].tolist() for r in range(empty[0], empty[0] + empty[1])] == [[codec.event_type_range("tie")[0] + 3, 1]] * 3


@pytest.mark.parametrize("stride", [8, 2])
def test_the_cut_inside_a_tie_section(files, stride):
    seqs, frames = [ns for _, ns, _ in files], [f for _, _, f in files]
    codec = _codec(1)
    host = tokenize.target_rows_host(seqs, frames, codec, TIES, stride=stride)
    _same(tokenize.target_rows(seqs, frames, codec, TIES, stride=stride), host)
    assert host.truncated.sum() > 10


@pytest.mark.parametrize("spec,bins,granularity", [(NOTES, 127, "full"), (TIES, 1, "flat"), (TIES, 1, "midi_class")])
def test_the_notes_form_and_the_program_maps(files, spec, bins, granularity):
    seqs, frames = [ns for _, ns, _ in files], [f for _, _, f in files]
    codec = _codec(bins)
    kw = dict(granularity=granularity, segment_frames=256)
    _same(tokenize.target_rows(seqs, frames, codec, spec, **kw), tokenize.target_rows_host(seqs, frames, codec, spec, **kw))


def test_shifts_equal_separately_shifted_files():
    codec = _codec(1)
    _, ns, frames = tokenize_cases.spread_files(seeds=[3])[0]
    shifts = [-0.05, 0, 0.05]
    a = tokenize.target_rows([ns], [frames], codec, TIES, shifts=shifts)
    b = tokenize.target_rows([tokenize_cases.shifted(ns, s) for s in shifts], [frames] * 3, codec, TIES)
    assert a.rows_of_file.shape == (1, 3, 2)
    for x, y in zip(list(a)[:5], list(b)[:5]):
        assert torch.equal(x, y)
    _same(a, tokenize.target_rows_host([ns], [frames], codec, TIES, shifts=shifts))


# ------------------------------------------------------------------------------------------- end to end, trained fixture
@pytest.fixture(scope="module")
def model():
    return inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32")


@pytest.fixture(scope="module")
def piece():
    return synthetic.synth_music(8.192, seed=21)


def _moved(ns, seconds=0.0, semitones=0):
    return note_sequences.NoteSequence(notes=[note_sequences.Note(n.start_time + seconds, n.end_time + seconds,
                                                                  n.pitch + semitones, n.velocity, n.program, n.is_drum, 0)
                                              for n in ns.notes])


def test_score_notes_scores_the_rows_of_targets(model, piece):
    ns, wav = piece
    out = model.score_notes(wav, ns, return_note_scores=True)
    again = model.score_notes(wav, ns)
    assert np.array_equal(out["segment_scores"], again["segment_scores"])        # the path is bit-stable between two calls
    targets = model.targets(wav, ns)
    assert len(targets) == len(out["segment_scores"]) == 5 and all(t[-1] == 1 for t in targets)
    want = model.score(wav, targets)
    print("segment_scores", out["segment_scores"].tolist(), "score()", want.tolist())
    assert np.array_equal(out["segment_scores"], want)
    n_ids = sum(len(t) for t in targets)
    assert out["loss"] == pytest.approx(-want.sum() / n_ids, rel=1e-12) and out["truncated_segments"] == 0
    assert 0.0 <= out["token_accuracy"] <= 1.0
    assert len(out["onset_logprob"]) == len(ns.notes) and np.isfinite(out["onset_logprob"]).all()
    assert np.isfinite(out["end_logprob"]).all() and (out["onset_margin"] <= 0).all()


def test_true_notes_score_better_than_wrong_ones(model, piece):
    ns, wav = piece
    true = model.score_notes(wav, ns)["loss"]
    up = model.score_notes(wav, _moved(ns, semitones=1))["loss"]
    late = model.score_notes(wav, _moved(ns, seconds=0.5))["loss"]
    print("loss: true %.4f, a semitone up %.4f, 0.5 s later %.4f" % (true, up, late))
    assert true < up
    assert true < late


def test_best_shift_finds_a_delay(model, piece):
    ns, _ = piece
    delayed = _moved(ns, seconds=0.1)
    amps = np.random.default_rng(22).uniform(0.3, 1.0, len(ns.notes))
    wav = synthetic.render_notes([n.start_time for n in delayed.notes], [n.end_time for n in delayed.notes],
                                 [n.pitch for n in delayed.notes], amps, np.zeros(len(ns.notes), np.int64), 1,
                                 int(round(8.192 * 16000)), seed=21).reshape(-1).cpu().numpy()
    out = model.score_notes(wav, ns, shifts=[-0.2, -0.1, 0, 0.1, 0.2])
    print("loss over shifts", out["loss"].tolist())
    assert out["loss"].shape == (5,)
    assert out["best_shift"] == 0.1


def test_score_notes_many_and_refusals(model, piece):
    ns, wav = piece
    one = model.score_notes(wav, ns)
    two = model.score_notes_many([(wav, ns), (wav[: 3 * 32768 - 128], _moved(ns, semitones=1))])
    assert len(two) == 2 and np.array_equal(two[0]["segment_scores"], one["segment_scores"])
    assert len(two[1]["segment_scores"]) == 3
    fp8 = inference.InferenceModel.__new__(inference.InferenceModel)
    fp8.model_config = type("C", (), {"kv_dtype": "e4m3"})()
    with pytest.raises(ValueError):
        fp8.score_notes(wav, ns)


def test_command_line_score_midi(tmp_path, piece):
    from mt3_amd import audio_io
    ns, wav = piece
    refs = tmp_path / "refs"
    refs.mkdir()
    for name in ("a", "b"):
        (tmp_path / (name + ".wav")).write_bytes(audio_io.samples_to_wav_data(wav, 16000))
        midi_io.note_sequence_to_midi_file(ns, str(refs / (name + ".mid")))
    r = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", CKPT, "--score-midi", str(refs),
                        "--score-shifts=-0.1,0,0.1", "-o", str(tmp_path / "out"), str(tmp_path / "a.wav"),
                        str(tmp_path / "b.wav")], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "out" / "midi_scores.json") as f:
        records = json.load(f)
    assert [os.path.basename(x["audio"]) for x in records] == ["a.wav", "b.wav"]
    assert all(np.isfinite(x["loss"]).all() and x["best_shift"] == 0 for x in records)
