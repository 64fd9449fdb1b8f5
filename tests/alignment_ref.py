"""Shift paths by brute force: every one of the K^S paths of a small table, its cost summed in the order the rule of
mt3_op_align_paths writes (include/mt3_hip.h) -- the yardstick of `alignment.best_paths_reference`, which in turn is the
yardstick of the kernel.  Also the tables the path tests share."""
import itertools

import numpy as np


def path_cost(scores, grid, lam, max_jump, path):
    """cost of one path in the rule's order, every operation rounded once; None where a jump exceeds max_jump"""
    c = -np.asarray(scores, np.float32).astype(np.float64)
    g = np.asarray(grid, np.float64)
    cost = c[0, path[0]]
    for s in range(1, len(path)):
        jump = np.abs(g[path[s]] - g[path[s - 1]])
        if not jump <= max_jump:
            return None
        cost = c[s, path[s]] + (cost + np.float64(lam) * jump)
    return cost


def exhaustive(scores, grid, lam, max_jump=np.inf):
    """(the least cost, the path the tie rule names among the paths of that cost, how many paths have that cost): the
    lowest last index, then the lowest index one segment earlier, and so on -- what reading back through "the lowest k on
    equal values" gives when the arithmetic is exact (integer tables, grids and penalties)"""
    S, K = np.asarray(scores).shape
    best, paths = None, []
    for p in itertools.product(range(K), repeat=S):
        cost = path_cost(scores, grid, lam, max_jump, p)
        if cost is None:
            continue
        if best is None or cost < best:
            best, paths = cost, [p]
        elif cost == best:
            paths.append(p)
    return best, min(paths, key=lambda p: p[::-1]), len(paths)


def ragged_job(rng, K, kind):
    """files of 1, 2, 3 and 300 segments (and a second file of 3) over K shifts -> (scores float32 [sum, K], counts).
    kind 'float': log-probabilities as a scoring call gives them (negative, tens to hundreds, a ridge that drifts);
    'ties': small integers, so equal costs are everywhere; 'zero': all 0"""
    counts = [1, 300, 2, 3, 3]
    total = sum(counts)
    if kind == "zero":
        return np.zeros((total, K), np.float32), counts
    if kind == "ties":
        return -rng.integers(0, 3, size=(total, K)).astype(np.float32), counts
    ridge = (np.cumsum(rng.normal(0, 0.7, total)) % K)[:, None]
    depth = rng.uniform(20, 400, (total, 1))
    scores = -depth - 8.0 * np.abs(np.arange(K)[None, :] - ridge) + rng.normal(0, 3.0, (total, K))
    return scores.astype(np.float32), counts
