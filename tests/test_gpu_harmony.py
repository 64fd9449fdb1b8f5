"""mt3_op_analyze_harmony on the device against the numpy rule, field for field and bit for bit, on ONE job that holds the
rule's edge files and files whose beat and note counts straddle the kernel's tiles (tests/harmony_cases.py); in any order of
the files and of a file's notes, twice, at both ends of change_penalty; on the progressions; and through the model."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import harmony, inference, synthetic  # noqa: E402
from mt3_amd import note_sequences as N  # noqa: E402
from tests import harmony_cases as hc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")
PENALTIES = (harmony.DEFAULT_CHANGE_PENALTY, 0, 1 << 20)


def same(a, b):
    for field in dataclasses.fields(harmony.Harmony):
        x, y = getattr(a, field.name), getattr(b, field.name)
        if isinstance(x, np.ndarray):
            if x.dtype != y.dtype or not np.array_equal(x, y):
                return False
        elif x != y or type(x) is not type(y):
            return False
    return True


@pytest.fixture(scope="module")
def edge():
    job = hc.edge_job()
    names, sequences, beats = [j[0] for j in job], [j[1] for j in job], [j[2] for j in job]
    want = {p: harmony.analyze_reference(sequences, beats, p) for p in PENALTIES}     # computed once, shared, never changed
    return names, sequences, beats, want


@pytest.mark.parametrize("penalty", PENALTIES)
def test_the_device_equals_the_rule_on_every_file_of_the_edge_job(edge, penalty):
    names, sequences, beats, want = edge
    got = harmony.analyze(sequences, beats, penalty)
    assert len(got) == len(names)
    for name, w, g in zip(names, want[penalty], got):
        assert same(w, g), (name, w, g)


def test_the_job_holds_what_it_was_built_to_hold(edge):
    names, _, beats, want = edge
    by = dict(zip(names, want[harmony.DEFAULT_CHANGE_PENALTY]))
    assert [len(by["%d beats" % B].chords) for B in range(6)] == [0, 0, 2, 3, 4, 5]
    assert by["3 beats"].beats_per_bar == 0 and by["4 beats"].beats_per_bar == 2
    assert by["drums only"].key == -1 and not by["drums only"].chords.any() and by["no notes"].key == -1
    assert by["notes and no beats"].key == 0 and by["twelve keys tie"].key == 0
    assert len(set(by["twelve keys tie"].key_scores[::2].tolist())) == 1
    assert set(by["two chords tie"].chords.tolist()) == {1}
    assert (by["two phases tie"].beats_per_bar, by["two phases tie"].downbeat) == (4, 0)
    assert by["m = 2 over m = 4"].beats_per_bar == 2 and by["every beat alike"].beats_per_bar == 0
    assert {len(b) for b in beats} >= {hc.BEAT_TILE - 1, hc.BEAT_TILE, hc.BEAT_TILE + 1, 3 * hc.BEAT_TILE + 1}
    loose, tight = want[0], want[1 << 20]
    assert any(len(set(h.chords.tolist())) > 2 for h in loose) and all(len(set(h.chords.tolist())) <= 1 for h in tight)


def test_any_order_of_the_files_and_of_a_files_notes_and_twice_the_same_bits(edge):
    names, sequences, beats, want = edge
    want = want[harmony.DEFAULT_CHANGE_PENALTY]
    backwards = harmony.analyze(sequences[::-1], beats[::-1])[::-1]
    assert all(same(w, g) for w, g in zip(want, backwards))
    rng = np.random.RandomState(0)
    shuffled = [N.NoteSequence(notes=[s.notes[i] for i in rng.permutation(len(s.notes))], total_time=s.total_time)
                for s in sequences]
    for name, w, g in zip(names, want, harmony.analyze(shuffled, beats)):
        assert same(w, g), name
    # a smaller job first, so that the second call's workspace is not the first one's: nothing stale is read
    few = harmony.analyze(sequences[5:9], beats[5:9])
    assert all(same(w, g) for w, g in zip(want[5:9], few))
    assert all(same(w, g) for w, g in zip(want, harmony.analyze(sequences, beats)))


@pytest.mark.parametrize("jitter", [0, 2])
def test_the_device_equals_the_rule_on_the_progressions(jitter):
    cases = hc.progressions(jitter)
    sequences, beats = [c[1] for c in cases], [c[2] for c in cases]
    got = harmony.analyze(sequences, beats)
    for (name, _, _, truth), w, g in zip(cases, harmony.analyze_reference(sequences, beats), got):
        assert same(w, g), name
        assert g.key == truth["key"] and np.array_equal(g.chords, truth["chords"]), name
        assert (g.beats_per_bar, g.downbeat) == (truth["beats_per_bar"], truth["downbeat"]), name


def test_empty_jobs():
    assert harmony.analyze([], []) == []
    for h in harmony.analyze([N.NoteSequence(), N.NoteSequence()], [np.zeros(0, np.int32), hc.grid(4)]):
        assert (h.key, h.beats_per_bar, h.downbeat, h.chord_score) == (-1, 0, -1, 0) and not h.chords.any()


def test_the_model_attaches_harmony_on_request():
    model = inference.InferenceModel(CKPT, "mt3")
    _, y16 = synthetic.synth_music(3 * 2.048 + 0.7, seed=21, device="cpu")
    audio = np.asarray(y16, np.float32)
    ns = model(audio, harmony=True)
    assert len(ns.notes) >= 5 and len(ns.beats.frames) >= 2
    assert same(ns.harmony, harmony.analyze_reference([ns], [ns.beats])[0])
    assert len(ns.harmony.chords) == len(ns.beats.frames)
    assert same(inference.InferenceModel.harmony(ns), ns.harmony)
    plain = model(audio)
    assert not hasattr(plain, "harmony") and not hasattr(plain, "beats")
    assert [dataclasses.astuple(n) for n in plain.notes] == [dataclasses.astuple(n) for n in ns.notes]
    loose = model(audio, harmony={"change_penalty": 0}, beats={"prior_bpm": 100.0})
    assert same(loose.harmony, harmony.analyze_reference([loose], [loose.beats], 0)[0])
    with pytest.raises(ValueError, match="harmony= takes"):
        model(audio, harmony={"penalty": 3})
    with pytest.raises(ValueError, match="harmony= is for the transcribing methods"):
        model._transcribe([], False, {}, scored=True, harmony=True)
