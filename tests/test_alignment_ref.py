"""mt3_amd.alignment on the host: `best_paths_reference` against the brute force of tests/alignment_ref.py, its special
cases, and the warp (`warp_notes`) with its refusals."""
import numpy as np
import pytest

from mt3_amd import alignment
from mt3_amd.note_sequences import Note, NoteSequence
from tests import alignment_ref as ar


def _ref(scores, grid, lam, max_jump=None):
    path, total = alignment.best_paths_reference(scores, [len(scores)], grid, lam, max_jump)
    return tuple(int(j) for j in path), total[0]


def test_shift_grid():
    g = alignment.shift_grid(0.2, 0.02)
    assert g.dtype == np.float64 and len(g) == 21 and g[10] == 0.0 and g[0] == -10 * 0.02 and g[-1] == 10 * 0.02
    assert np.all(np.diff(g) > 0)
    assert list(alignment.shift_grid(0.2, 0.1)) == [-0.2, -0.1, 0.0, 0.1, 0.2]
    assert list(alignment.shift_grid(0.05, 0.1)) == [0.0]
    for bad in [(0.2, 0.0), (-0.1, 0.1), (float("nan"), 0.1), (1.0, 0.01)]:       # the last: 201 shifts
        with pytest.raises(ValueError):
            alignment.shift_grid(*bad)


@pytest.mark.parametrize("S,K", [(1, 1), (1, 4), (2, 2), (3, 3), (4, 4), (5, 3), (5, 4)])
def test_integer_tables_full_of_ties_against_all_paths(S, K):
    """exact arithmetic (integer scores, grid and penalty), so the tie rule decides: cost bit-equal, path equal"""
    rng = np.random.default_rng(100 * S + K)
    grid = np.arange(K, dtype=np.float64)
    ties = 0
    for trial in range(12):
        scores = -rng.integers(0, 3, size=(S, K)).astype(np.float32)
        for lam, max_jump in [(0.0, np.inf), (1.0, np.inf), (2.0, 1.0), (1.0, 2.0), (1000.0, np.inf), (1.0, 0.0)]:
            cost, path, n_best = ar.exhaustive(scores, grid, lam, max_jump)
            got_path, got_cost = _ref(scores, grid, lam, max_jump)
            assert got_cost == cost and np.float64(got_cost).tobytes() == np.float64(cost).tobytes()
            assert got_path == path, (scores, lam, max_jump)
            ties += n_best > 1
    assert K == 1 or ties > 0                    # equal costs did occur


@pytest.mark.parametrize("S,K", [(2, 3), (4, 4), (5, 4)])
def test_float_tables_on_a_non_uniform_grid_cost_bit_equal(S, K):
    """rounded arithmetic: the least cost over all paths, each summed in the rule's order, is the rule's cost to the bit
    (rounding is monotone), and the path returned has that cost"""
    rng = np.random.default_rng(7 * S + K)
    grid = np.sort(rng.uniform(-0.2, 0.2, K))
    for trial in range(8):
        scores = (-rng.uniform(5, 300, (S, K))).astype(np.float32)
        for lam, max_jump in [(0.0, np.inf), (13.7, np.inf), (250.0, 0.15), (1e6, np.inf)]:
            cost, _, _ = ar.exhaustive(scores, grid, lam, max_jump)
            got_path, got_cost = _ref(scores, grid, lam, max_jump)
            assert np.float64(got_cost).tobytes() == np.float64(cost).tobytes()
            assert ar.path_cost(scores, grid, lam, max_jump, got_path) == cost


def test_special_cases():
    rng = np.random.default_rng(3)
    S, K = 40, 7
    scores = (-rng.uniform(5, 300, (S, K))).astype(np.float32)
    grid = alignment.shift_grid(0.3, 0.1)
    path, _ = _ref(scores, grid, 0.0)
    assert path == tuple(int(j) for j in scores.argmax(1))                      # no smoothness: each segment's best
    column = int(np.argmin(np.cumsum(-scores.astype(np.float64), axis=0)[-1]))
    path, total = _ref(scores, grid, 1e9)
    assert path == (column,) * S                                                # huge: the best constant path
    assert total == np.cumsum(-scores.astype(np.float64), axis=0)[-1, column]
    path2, total2 = _ref(scores, grid, 3.0, 0.05)                               # max_jump below the step: constant too
    assert path2 == (column,) * S and total2 == total
    path3, total3 = _ref(scores, grid, 0.0, 0.0)
    assert path3 == path2 and total3 == total
    zero_path, zero_total = _ref(np.zeros((9, K), np.float32), grid, 1.0)
    assert zero_path == (0,) * 9 and zero_total == 0.0                          # all equal: index 0 throughout


def test_files_are_independent_and_arguments_are_checked():
    rng = np.random.default_rng(11)
    scores, counts = ar.ragged_job(rng, 5, "float")
    grid = alignment.shift_grid(0.2, 0.1)
    path, total = alignment.best_paths_reference(scores, counts, grid, 20.0, 0.1)
    assert path.dtype == np.int32 and total.dtype == np.float64 and len(total) == len(counts)
    first = 0
    for i, n in enumerate(counts):
        p, t = alignment.best_paths_reference(scores[first: first + n], [n], grid, 20.0, 0.1)
        assert np.array_equal(p, path[first: first + n]) and t[0] == total[i]
        assert np.all(np.abs(np.diff(grid[p])) <= 0.1 + 1e-12)
        first += n
    for bad in [dict(grid=[0.0, 0.0]), dict(grid=[0.1, 0.0]), dict(grid=[0.0, np.nan]), dict(grid=[]),
                dict(grid=np.arange(65.0)), dict(lam=-1.0), dict(lam=np.nan), dict(lam=np.inf), dict(max_jump=-0.1),
                dict(max_jump=np.nan), dict(counts=[0, 4]), dict(counts=[3])]:
        kw = dict(dict(grid=[0.0, 0.1], lam=1.0, max_jump=None, counts=[4]), **bad)
        with pytest.raises(ValueError):
            alignment.best_paths_reference(np.zeros((4, len(kw["grid"])), np.float32), kw["counts"], kw["grid"], kw["lam"],
                                           kw["max_jump"])


def _ns():
    notes = [Note(0.0, 0.05, 60, 90, 0, False, 0), Note(0.5, 0.9, 62, 80, 5, False, 1), Note(2.5, 3.5, 36, 100, 0, True, 9),
             Note(3.0, 3.0, 70, 64, 40, False, 2), Note(5.75, 6.5, 65, 77, 0, False, 0)]
    return NoteSequence(notes=notes, total_time=6.5, ticks_per_quarter=480)


def test_constant_path_adds_the_shift_and_clamps_at_zero():
    ns = _ns()
    for shift in (0.1, -0.02, -0.7):
        out = alignment.warp_notes(ns, [shift] * 3, 2.0)
        for a, b in zip(ns.notes, out.notes):
            assert b.start_time == max(a.start_time + shift, 0.0) and b.end_time == max(a.end_time + shift, 0.0)
            assert (b.pitch, b.velocity, b.program, b.is_drum, b.instrument) == \
                   (a.pitch, a.velocity, a.program, a.is_drum, a.instrument)
        assert out.ticks_per_quarter == 480 and out.total_time == max(n.end_time for n in out.notes)
    assert [n.start_time for n in ns.notes] == [0.0, 0.5, 2.5, 3.0, 5.75]       # the input is not touched
    assert alignment.warp_notes(NoteSequence(), [0.1], 2.0).notes == []


def test_interpolation_between_anchors_by_hand():
    """three segments of 2 s, shifts 0.0, 0.5, -0.5: anchors at 1, 3 and 5 s"""
    shifts, T = [0.0, 0.5, -0.5], 2.0
    by_hand = {0.0: 0.0, 0.5: 0.0, 1.0: 0.0, 2.0: 0.25, 2.5: 0.375, 3.0: 0.5, 3.5: 0.25, 4.0: 0.0, 4.5: -0.25, 5.0: -0.5,
               5.75: -0.5, 6.5: -0.5}
    for t, d in by_hand.items():
        assert alignment.shift_at(t, shifts, T) == d, t
    out = alignment.warp_notes(_ns(), shifts, T)
    assert [(n.start_time, n.end_time) for n in out.notes] == \
        [(0.0, 0.05), (0.5, 0.9), (2.875, 3.75), (3.5, 3.5), (5.25, 6.0)]


def test_warp_is_monotone_and_keeps_end_after_start():
    rng = np.random.default_rng(5)
    T = 2.048
    for trial in range(20):
        S = int(rng.integers(1, 12))
        shifts = rng.uniform(-0.49 * T, 0.49 * T, S)             # neighbours differ by less than T
        starts = np.sort(rng.uniform(0, S * T + 1, 200))
        ns = NoteSequence(notes=[Note(float(t), float(t + d), 60) for t, d in zip(starts, rng.uniform(0, 1.5, 200))])
        out = alignment.warp_notes(ns, shifts, T)
        got = np.array([n.start_time for n in out.notes])
        assert np.all(np.diff(got) >= 0)
        assert all(n.end_time >= n.start_time for n in out.notes)


def test_jumps_of_a_segment_or_more_are_refused():
    ns = _ns()
    with pytest.raises(ValueError):
        alignment.warp_notes(ns, [0.0, 2.0], 2.0)
    with pytest.raises(ValueError):
        alignment.warp_notes(ns, [1.0, -1.5, 0.0], 2.0)
    alignment.warp_notes(ns, [0.0, 1.999], 2.0)
    for bad in [dict(path_shifts=[], segment_seconds=2.0), dict(path_shifts=[np.nan], segment_seconds=2.0),
                dict(path_shifts=[0.0], segment_seconds=0.0)]:
        with pytest.raises(ValueError):
            alignment.warp_notes(ns, **bad)
    # the grid-level check align_notes makes before any device work
    assert alignment.check_jumps(alignment.shift_grid(0.2, 0.02), None, 2.048) == pytest.approx(0.4)
    assert alignment.check_jumps(alignment.shift_grid(1.5, 0.1), 0.35, 2.048) == pytest.approx(0.3)
    with pytest.raises(ValueError):
        alignment.check_jumps(alignment.shift_grid(1.1, 0.1), None, 2.048)      # -1.1 .. 1.1: a jump of 2.2 s
    with pytest.raises(ValueError):
        alignment.check_jumps([-1.024, 1.024], None, 2.048)                     # exactly a segment
