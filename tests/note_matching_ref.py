"""An independent restatement of the note-matching rule for the tests: the edge predicate written out densely (the
n_ref x n_est matrices mir_eval builds), a brute force over permutations for tiny problems, and a first-fit greedy."""
import itertools

import numpy as np


def dense_adjacency(ref_iv, ref_p, est_iv, est_p, onset_tolerance=0.05, pitch_tolerance=50.0, offset_ratio=0.2,
                    offset_min_tolerance=0.05, strict=False):
    """bool [n_ref, n_est]: mir_eval.transcription.match_notes' three tests on every pair"""
    cmp = np.less if strict else np.less_equal
    ref_iv, est_iv = np.asarray(ref_iv, np.float64).reshape(-1, 2), np.asarray(est_iv, np.float64).reshape(-1, 2)
    ref_p, est_p = np.asarray(ref_p, np.float64), np.asarray(est_p, np.float64)
    onset = np.around(np.abs(np.subtract.outer(ref_iv[:, 0], est_iv[:, 0])), 6)
    ok = cmp(onset, onset_tolerance)
    with np.errstate(divide="ignore", invalid="ignore"):
        cents = np.abs(1200.0 * np.subtract.outer(np.log2(ref_p), np.log2(est_p)))
    ok &= cmp(np.nan_to_num(cents, nan=0.0), pitch_tolerance)
    if offset_ratio is not None:
        offset = np.around(np.abs(np.subtract.outer(ref_iv[:, 1], est_iv[:, 1])), 6)
        tol = np.maximum(offset_ratio * (ref_iv[:, 1] - ref_iv[:, 0]), offset_min_tolerance)
        ok &= cmp(offset, tol[:, None])
    return ok


def brute_force_maximum(adjacency) -> int:
    """the size of a maximum matching by trying every injection of the smaller side; min side <= 6"""
    a = np.asarray(adjacency, bool)
    if a.shape[0] > a.shape[1]:
        a = a.T
    n, m = a.shape
    assert n <= 6 and m <= 9, "brute force is for tiny problems"
    best = 0
    for cols in itertools.permutations(range(m), n):
        best = max(best, int(sum(a[i, c] for i, c in enumerate(cols))))
    return best


def greedy_first_fit(adjacency, est_onsets) -> int:
    """each reference in turn takes the first free adjacent estimate in onset order: what a pass without augmenting paths
    finds"""
    a = np.asarray(adjacency, bool)
    order = np.argsort(np.asarray(est_onsets), kind="stable")
    used = np.zeros(a.shape[1], bool)
    count = 0
    for i in range(a.shape[0]):
        free = order[a[i, order] & ~used[order]]
        if len(free):
            used[free[0]] = True
            count += 1
    return count
