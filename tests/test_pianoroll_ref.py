"""The numpy restatement of the piano roll / frame count rule (tests/pianoroll_ref.py) against literals worked out by
hand (tests/pianoroll_cases.py), and the host half of mt3_amd/pianoroll.py: widths and packing.  No device here."""
import copy

import numpy as np
import pytest

from mt3_amd import pianoroll
from tests import pianoroll_cases as cases
from tests import pianoroll_ref as ref


@pytest.mark.parametrize("name,ns,fps,is_drum,want", cases.ROLL_CASES, ids=[c[0] for c in cases.ROLL_CASES])
def test_roll_literals(name, ns, fps, is_drum, want):
    before = copy.deepcopy(ns)
    got = ref.pianoroll(ns, fps, is_drum)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert ns == before                                # the reference mutates its argument; the rule here does not


def test_the_literals_say_what_their_names_say():
    by_name = {c[0]: c[4] for c in cases.ROLL_CASES}
    assert 0.29 * 100 == 28.999999999999996 and int(0.29 * 100) == 28
    short = by_name["short note becomes 0.05 s"]
    assert short.shape == (128, 105) and short[60].nonzero()[0].tolist() == [100, 101, 102, 103, 104]
    trunc = by_name["truncation of 0.29 * 100"]
    assert trunc[60, 28] == 80 and trunc[60, 27] == 0
    assert by_name["two programs on one pitch sum"][60].tolist() == [50] * 5 + [120] * 5
    silent = by_name["drum note widens the roll and stays silent"]
    assert silent.shape == (128, 200) and not silent[36].any() and silent[60, :50].all() and not silent[60, 50:].any()
    drums = by_name["is_drum renders every note at 0.05 s"]
    assert drums.shape == (128, 105) and drums[36, 100:105].tolist() == [90] * 5 and drums.sum() == 5 * 100 + 5 * 90
    assert by_name["coinciding indices add nothing"].shape == (128, 1)
    assert by_name["an empty sequence"].shape == (128, 0)


@pytest.mark.parametrize("name,r,e,thr,counts,prf", cases.COUNT_CASES, ids=[c[0] for c in cases.COUNT_CASES])
def test_frame_metric_literals(name, r, e, thr, counts, prf):
    assert ref.frame_counts(r, e, thr) == counts
    assert ref.frame_metrics(r, e, thr) == prf
    assert ref.precision_recall_f1(*counts) == pianoroll.precision_recall_f1(*counts) == prf


def test_worked_example_values():
    p, r, f = ref.precision_recall_f1(3, 1, 2)
    assert (p, r) == (0.75, 0.6) and abs(f - 2 / 3) < 1e-15
    assert ref.precision_recall_f1(0, 0, 0) == (0.0, 0.0, 0.0)
    assert ref.precision_recall_f1(0, 5, 0) == (0.0, 0.0, 0.0) and ref.precision_recall_f1(0, 0, 5) == (0.0, 0.0, 0.0)


# ------------------------------------------------------------------ the host half of mt3_amd/pianoroll.py
@pytest.mark.parametrize("name,ns,fps,is_drum,want", cases.ROLL_CASES, ids=[c[0] for c in cases.ROLL_CASES])
def test_packed_widths_are_the_rule_s(name, ns, fps, is_drum, want):
    packed, n, offs, widths = pianoroll._pack([ns, ns], fps, is_drum)
    assert n == 2 * len(ns.notes) and offs.tolist() == [0, len(ns.notes), n]
    assert widths.tolist() == [want.shape[1]] * 2 and widths.dtype == np.int32
    assert packed.dtype == np.uint8 and packed.size == 28 * n
    start = packed[: 8 * n].view("<f8")
    pitch = packed[16 * n: 20 * n].view("<i4")
    assert start.tolist() == [x.start_time for x in ns.notes] * 2 and pitch.tolist() == [x.pitch for x in ns.notes] * 2


def test_random_widths_follow_the_restatement():
    rng = np.random.default_rng(5)
    for fps in (62.5, 100.0):
        for is_drum in (False, True):
            seqs = [cases.random_sequence(rng, 40, 3.0, fps) for _ in range(5)]
            widths = pianoroll._pack(seqs, fps, is_drum)[3]
            assert widths.tolist() == [ref.pianoroll(s, fps, is_drum).shape[1] for s in seqs]


def test_what_the_host_refuses():
    for bad in (cases.ns_of((0.0, 1.0, 128, 80)), cases.ns_of((0.0, 1.0, -1, 80))):
        with pytest.raises(ValueError, match="pitches 0 .. 127"):
            pianoroll._pack([cases.ns_of((0.0, 1.0, 5, 80)), bad], 62.5, False)
    for bad in (cases.ns_of((-0.5, 1.0, 60, 80)), cases.ns_of((0.0, float("nan"), 60, 80)), cases.ns_of((0.0, float("inf"), 60, 80))):
        with pytest.raises(ValueError, match="note times"):
            pianoroll._pack([bad], 62.5, False)
    for fps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="fps"):
            pianoroll._pack([cases.ns_of()], fps, False)
    with pytest.raises(ValueError, match="velocity_threshold"):
        pianoroll._threshold(30.5)
    with pytest.raises(ValueError, match="reference sequences"):
        pianoroll.frame_counts([cases.ns_of()], [])
