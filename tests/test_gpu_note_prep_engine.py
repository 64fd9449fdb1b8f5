"""`sustain=True` through InferenceModel on the trained fixture checkpoint: the targets, scores and alignment of a sequence
with a sustain pedal are those of the host-sustained sequence (`note_sequences.sustain_reference`), and differ from the
unsustained ones where the pedal carries a note across a segment boundary."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import checkpoints, inference, note_sequences, synthetic  # noqa: E402
from tests import note_prep_ref as ref  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")


@pytest.fixture(scope="module")
def model():
    return inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32")


@pytest.fixture(scope="module")
def piece():
    """the fixture's piece with a pedal that goes down and up every 1.5 s"""
    ns, wav = synthetic.synth_music(8.192, seed=21)
    ns = note_sequences.NoteSequence(list(ns.notes), ns.total_time, ns.ticks_per_quarter)
    for k in range(6):
        ns.control_changes += [note_sequences.ControlChange(1.5 * k + 0.2, 64, 100, 0),
                               note_sequences.ControlChange(1.5 * k + 1.3, 64, 20, 0)]
    return ns, wav


def test_targets_under_the_pedal_are_the_host_sustained_targets(model):
    # segments of 2.048 s; the key of pitch 60 goes up at 1.5, the pedal holds it until 3.0: segment 1 starts with it tied
    ns = ref.seq([(60, 100, 1.0, 1.5), (64, 100, 2.5, 2.75)], [(0.5, 127), (3.0, 0)])
    n_samples = 3 * 32768 - 128
    got = model.targets(n_samples, ns, sustain=True)
    want = model.targets(n_samples, note_sequences.sustain_reference(ns))
    plain = model.targets(n_samples, ns)
    assert len(got) == len(want) == len(plain) == 3
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    tie = model.codec.event_type_range("tie")[0] + 3
    assert plain[1][0] == tie                                 # the key went up in segment 0: nothing is tied
    assert got[1][0] != tie and tie in got[1][1:4].tolist()   # the pedal carries the note over: program, pitch, tie
    assert got[1].tolist() != plain[1].tolist() and len(got[1]) > len(plain[1])
    assert model.targets(n_samples, ns, sustain=False)[1].tolist() == plain[1].tolist()
    assert len(ns.control_changes) == 2 and ns.notes[0].end_time == 1.5       # the caller's sequence is untouched


def test_score_notes_under_the_pedal(model, piece):
    ns, wav = piece
    host = note_sequences.sustain_reference(ns)
    assert [n.end_time for n in host.notes] != [n.end_time for n in ns.notes]
    got = model.score_notes_many([(wav, ns)], sustain=True, return_note_scores=True)[0]
    want = model.score_notes(wav, host, return_note_scores=True)
    plain = model.score_notes(wav, ns)
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=isinstance(want[key], np.ndarray)), key
    assert len(got["onset_logprob"]) == len(host.notes)
    assert not np.array_equal(plain["segment_scores"], want["segment_scores"])
    print("loss: as written %.4f, sustained %.4f" % (plain["loss"], got["loss"]))
    many = model.score_notes_many([(wav, ns), (wav, host)], sustain=True)
    assert np.array_equal(many[0]["segment_scores"], want["segment_scores"])
    assert np.array_equal(many[1]["segment_scores"], want["segment_scores"])      # no pedal left: sustain changes nothing


def test_align_notes_warps_the_sustained_notes(model, piece):
    ns, wav = piece
    host = note_sequences.sustain_reference(ns)
    kw = dict(shifts=[-0.02, 0.0, 0.02])
    got = model.align_notes(wav, ns, sustain=True, **kw)
    want = model.align_notes(wav, host, **kw)
    assert got["notes"] == want["notes"] and len(got["notes"].notes) == len(host.notes)
    assert np.array_equal(got["segment_shifts"], want["segment_shifts"]) and got["path_score"] == want["path_score"]
