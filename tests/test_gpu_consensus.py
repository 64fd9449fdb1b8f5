"""mt3_op_note_consensus on the device == `consensus.consensus_reference` (numpy), exactly: every integer column equal,
the times equal as uint64, note_votes equal per voter -- on the hand-written cases of tests/consensus_ref.py, one ragged
job (empty file, one note, four tiles, a cluster across a tile boundary, a cluster of 300 members, 1 / 2 / 3 / 64
voters), more files than one launch holds, random jobs dense in ties, and twice for determinism."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mt3_amd import _lib, consensus  # noqa: E402
from tests import consensus_ref as ref  # noqa: E402

TILE = _lib.CONSENSUS_TILE
AT = float(TILE + 10)        # where the cluster that straddles the first tile boundary begins, in seconds


def _both(groups, **kw):
    got, want = consensus.consensus(groups, **kw), consensus.consensus_reference(groups, **kw)
    ref.assert_same(got, want)
    return got


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_hand_written_cases(name):
    groups, kw = ref.CASES[name]
    _both(groups, **kw)


def _jittered(rng, n, voters, pitches=8, seconds=60.0):
    """`voters` transcriptions of n random notes: onsets moved by up to 0.02 s, one note in ten dropped"""
    start = np.sort(rng.uniform(0, seconds, n))
    length = rng.uniform(0.05, 1.0, n)
    pitch, program = 40 + rng.randint(pitches, size=n), rng.randint(2, size=n) * 33
    out = []
    for _ in range(voters):
        keep = rng.uniform(size=n) > 0.1
        s = start[keep] + rng.uniform(-0.02, 0.02, int(keep.sum()))
        e = s + length[keep] + rng.uniform(-0.02, 0.02, int(keep.sum()))
        out.append(ref.ns([(max(a, 0.0), max(a, b, 0.0), p, rng.randint(1, 128), g)
                           for a, b, p, g in zip(s, e, pitch[keep], program[keep])]))
    return out


def _ragged_job():
    rng = np.random.RandomState(5)
    four_tiles = _jittered(rng, 4 * TILE // 3 + 20, 3)                # about four tiles of notes from 3 voters
    assert 3 * TILE < sum(len(v.notes) for v in four_tiles) <= 5 * TILE
    # one key, so the sorted order is the onset order: TILE - 1 single notes a second apart, then a cluster of three
    # voters' notes at sorted positions TILE - 1, TILE, TILE + 1, then a cluster that starts further on
    at = AT
    singles = [(float(i), i + 0.5, 60, 1 + i % 127) for i in range(TILE - 1)]
    straddle = [ref.ns(singles + [(at, at + 0.5, 60, 10), (at + 5.0, at + 5.5, 60, 40)]),
                ref.ns([(at + 0.01, at + 0.4, 60, 20), (at + 5.01, at + 5.6, 60, 50)]),
                ref.ns([(at + 0.02, at + 0.6, 60, 30)])]
    # one cluster of 300 members from 64 voters: onsets a millisecond apart, ends and velocities in no order
    big = [[] for _ in range(64)]
    for i in range(300):
        big[(i * 7) % 64].append((1.0 + i * 0.001, 2.0 + rng.randint(0, 50) / 64.0, 72, rng.randint(1, 128)))
    groups = [[ref.ns([]), ref.ns([])], [ref.ns([(0.25, 0.75, 60, 64, 3)])], four_tiles, straddle,
              [ref.ns(v) for v in big]]
    return groups, dict(min_votes=[2, 1, 2, 1, 33])


def test_one_ragged_job():
    groups, kw = _ragged_job()
    assert [len(g) for g in groups] == [2, 1, 3, 3, 64]
    packed = consensus.pack(groups, **kw)
    key, onset = packed.column(2), packed.column(0)
    a = int(packed.files["first"][3])                                  # the straddling cluster lies where it is meant to
    assert onset[a + TILE - 1] == AT and onset[a + TILE + 1] == AT + 0.02 and (key[a: a + TILE + 4] == 60).all()
    got = _both(groups, **kw)
    assert [len(r.notes.notes) for r in got[:2]] == [0, 1] and list(got[1].votes) == [1]
    assert len(got[2].notes.notes) > TILE // 2
    assert len(got[3].notes.notes) == TILE + 1                         # every single note, and the two clusters
    assert list(got[3].votes[-2:]) == [3, 2] and list(got[3].members[-2:]) == [3, 2]
    assert got[3].notes.notes[-2].start_time == AT + 0.01
    assert list(got[4].votes) == [64] and list(got[4].members) == [300]
    assert got[4].notes.notes[0].start_time == 1.0 + 149 * 0.001


def test_more_files_than_one_launch_holds():
    groups = ref.random_job(11, files=150)
    got = _both(groups)
    assert sum(len(r.notes.notes) for r in got) > 150


@pytest.mark.parametrize("grid", [True, False])
def test_random_jobs_dense_in_ties(grid):
    for seed in range(6):
        groups = ref.random_job(200 + seed, files=8, grid=grid, max_voters=9, notes=40)
        for kw in (dict(), dict(min_votes=1, tolerance=3 * ref.G), dict(programs=False, tolerance=0.0)):
            _both(groups, **kw)


def test_the_same_bits_on_every_run_and_for_any_order_of_the_input():
    groups, kw = _ragged_job()
    a, b = consensus.consensus(groups, **kw), consensus.consensus(groups, **kw)
    ref.assert_same(a, b)
    other, voter_order, note_order = ref.shuffled(groups, 3)
    c = consensus.consensus(other, **kw)
    for ra, rc, order, perms in zip(a, c, voter_order, note_order):
        ref.assert_same([dataclasses.replace(rc, note_votes=[])], [dataclasses.replace(ra, note_votes=[])])
        for new, (old, p) in enumerate(zip(order, perms)):
            assert np.array_equal(rc.note_votes[new], ra.note_votes[old][p])


def test_unsorted_columns_stay_inside_the_file():
    """the memory-safety statement of the op, and nothing more: the columns of a valid job in another order (one
    permutation per file, applied to all five columns) give MT3_OK and counts within [0, the file's notes]"""
    groups = ref.random_job(31, files=5, max_voters=6, notes=60) + [_jittered(np.random.RandomState(2), 2 * TILE, 2)]
    packed = consensus.pack(groups)
    rng = np.random.RandomState(9)
    perm = np.concatenate([int(f["first"]) + rng.permutation(int(f["n_notes"])) for f in packed.files])
    columns = [packed.column(k)[perm] for k in range(5)]
    mixed = dataclasses.replace(packed, columns=np.concatenate([c.view(np.uint8) for c in columns]))
    counts = consensus.run(mixed)[-1]                                  # raises unless the op returns MT3_OK
    torch.cuda.synchronize()
    assert ((counts >= 0) & (counts <= packed.files["n_notes"])).all()
