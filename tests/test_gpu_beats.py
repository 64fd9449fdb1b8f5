"""mt3_op_track_beats and mt3_op_snap_notes on the device against the numpy rule, bit for bit, on ONE job that holds the
rule's edge files, jittered files whose lengths straddle the kernel's own seams, a long file beside a tiny one, and the two
ends of the lag range."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, beats  # noqa: E402
from mt3_amd import note_sequences as N  # noqa: E402
from tests import beats_cases as bc  # noqa: E402

RING = 512                       # kRing of mt3_amd/csrc/beats.hip: the LDS ring of C
TILE = _lib.BEATS_TILE           # the autocorrelation's tile of E


def cut(bpm, n_frames, seed):
    """a jittered metrical file of exactly n_frames frames: its onsets below n_frames - 1, and one in the last frame"""
    ns, _ = bc.metrical(bpm, int(n_frames * bpm / 6000.0) + 4, jitter_frames=1, drop=0.2, extra=0.2, seed=seed, first=3)
    frames = [f for f in (int(round(n.start_time * 100)) for n in ns.notes) if f < n_frames - 1]
    return bc.sequence(frames + [n_frames - 1])


def job():
    files = {
        "no notes": bc.sequence([]),
        "one note": bc.sequence([731]),
        "22 apart": bc.sequence([10, 32]),
        "24 apart": bc.sequence([10, 34]),
        "25 apart: two beats, LAG_MIN": bc.sequence([10, 35]),
        "one frame": bc.sequence([40] * 7),
        "300 in a frame": bc.sequence(list(range(37, 600, 50)) + [287] * 299),
        "every frame": bc.sequence(list(range(400))),
        "LAG_MIN": bc.sequence([10, 35, 60]),
        "LAG_MAX": bc.sequence(list(range(5, 1300, 200))),
        "tiny": bc.sequence([0, 29]),
        "long": cut(124, 60000, 11),
    }
    for p in (25, 40):                                                      # F = lo, lo + 1, hi, hi + 1, p of the rule's edges
        for F in sorted({(p + 1) // 2, (p + 1) // 2 + 1, 2 * p, 2 * p + 1, p}):
            files["p %d, F %d" % (p, F)] = bc.sequence(sorted(set(range(0, F, p)) | {F - 1}))
    # 120 bpm: period 50 +- 1, lo = 25 or 26 -- lengths around a whole number of blocks of lo frames for either
    for F in (249, 250, 251, 259, 260, 261, RING - 1, RING, RING + 1, 2 * RING + 1, TILE - 1, TILE, TILE + 1,
              TILE + _lib.BEATS_LAG_MAX - 1, TILE + _lib.BEATS_LAG_MAX, TILE + _lib.BEATS_LAG_MAX + 1, 2 * TILE + 1):
        files["seam %d" % F] = cut(120, F, F)
    return files


@pytest.fixture(scope="module")
def tracked():
    files = job()
    sequences = list(files.values())
    want = beats.track_reference(sequences)                                 # computed once, shared, never changed
    got = beats.track(sequences)
    return files, sequences, want, got


def same(a, b):
    return (a.period == b.period and a.score == b.score and a.qpm == b.qpm and a.frames.dtype == b.frames.dtype and
            np.array_equal(a.frames, b.frames) and np.array_equal(a.times, b.times))


def test_the_device_equals_the_rule_on_every_file(tracked):
    files, _, want, got = tracked
    assert len(got) == len(files)
    for name, w, g in zip(files, want, got):
        assert same(w, g), (name, w, g)
    by = dict(zip(files, want))                                             # the job holds what it was built to hold
    assert by["LAG_MIN"].period == 25 and by["LAG_MAX"].period == 200
    assert len(by["25 apart: two beats, LAG_MIN"].frames) == 2 and by["22 apart"].period == 0
    assert len(by["long"].frames) > 1000 and by["tiny"].period in (0, 27, 28, 29, 30, 31)
    assert by["seam 250"].period == 50 and by["seam %d" % RING].period == 50 and by["seam %d" % TILE].period == 50


def test_twice_the_same_bits_and_any_order_of_the_files(tracked):
    _, sequences, _, got = tracked
    again = beats.track(sequences)
    assert all(same(a, b) for a, b in zip(got, again))
    backwards = beats.track(sequences[::-1])[::-1]
    assert all(same(a, b) for a, b in zip(got, backwards))


def test_more_files_than_one_launch_holds(tracked):
    files, sequences, want, _ = tracked
    few = [s for name, s in files.items() if name != "long"]
    many = (few * 3)[:70]                                                   # 32 files per launch: three launches
    got = beats.track(many)
    expect = ([w for name, w in zip(files, want) if name != "long"] * 3)[:70]
    assert all(same(a, b) for a, b in zip(expect, got))


@pytest.mark.parametrize("subdivisions", [1, 3, 4, 48])
def test_snap_equals_its_rule(tracked, subdivisions):
    files, sequences, want, _ = tracked
    keep = [i for i, name in enumerate(files) if name != "long"]
    sequences, found = [sequences[i] for i in keep], [want[i] for i in keep]
    assert any(len(b.frames) == 2 for b in found) and any(len(b.frames) == 0 and len(s.notes) for b, s in zip(found, sequences))
    # times off the 10 ms grid too, notes before the first and after the last beat, and notes shorter than a step
    rng = np.random.RandomState(subdivisions)
    moved = []
    for s in sequences:
        notes = [N.Note(n.start_time + rng.uniform(0, 0.3), n.start_time + rng.uniform(0, 0.3) + rng.choice([0.0, 0.004, 0.4]),
                        n.pitch, n.velocity, n.program, n.is_drum) for n in s.notes]
        moved.append(N.NoteSequence(notes=[n for n in notes] + [N.Note(0.0, 0.013, 60, 90), N.Note(700.0, 700.5, 61, 90)]))
    before = [[(n.start_time, n.end_time) for n in s.notes] for s in moved]
    ref = beats.snap_reference(moved, found, subdivisions)
    got = beats.snap(moved, found, subdivisions)
    for name, r, g, s, b in zip([n for n in files if n != "long"], ref, got, moved, found):
        assert [(n.start_time, n.end_time) for n in r.notes] == [(n.start_time, n.end_time) for n in g.notes], name
        assert g.total_time == r.total_time and len(g.notes) == len(s.notes)
        assert [(n.pitch, n.program, n.is_drum) for n in g.notes] == [(n.pitch, n.program, n.is_drum) for n in s.notes]
        if len(b.frames) < 2:
            assert [(n.start_time, n.end_time) for n in g.notes] == [(n.start_time, n.end_time) for n in s.notes], name
        else:
            assert all(n.end_time > n.start_time for n in g.notes), name
    assert [[(n.start_time, n.end_time) for n in s.notes] for s in moved] == before       # the inputs are untouched


def test_empty_jobs():
    assert beats.track([]) == []
    for b in beats.track([bc.sequence([]), bc.sequence([])]):
        assert (b.period, len(b.frames), b.score) == (0, 0, 0)
    empty = N.NoteSequence()
    assert [len(s.notes) for s in beats.snap([empty, empty], [np.array([10, 60]), np.array([], np.int32)], 4)] == [0, 0]
