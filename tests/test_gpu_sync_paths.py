"""mt3_op_sync_paths on the device EQUALS sync.paths_reference: path, length and total, at the sizes where the kernel
takes another route -- one strip, a strip's last column (16), a wave's last strip (64 strips = 1024 columns), a panel's
last strip (1024 strips = 16384 columns) -- and in one job of many files.

The yardstick above 64 x 65 cells is sync_cases.fast_paths: the same rule evaluated row by row, written without any
knowledge of the kernel.  It is tied to sync.paths_reference and to a brute-force full-matrix DTW at N, M <= 12 in
test_sync_ref, and to sync.paths_reference again at every size up to 64 x 65 here; larger sizes would take
paths_reference's double loop minutes.  A sequence against its exact copy needs no yardstick: the diagonal, total 0."""
import numpy as np
import pytest
import torch

from mt3_amd import sync
from tests import sync_cases as SC

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (65, 63), (255, 257), (1025, 300), (300, 1025),
         (5, 16), (5, 17), (3, 1024), (3, 1025), (40, 1040)]


def run(pairs):
    """the device's (path_i, path_j, total) per (a, s) pair of one job"""
    files = sync.file_table([len(a) for a, _ in pairs], [0] * len(pairs), [len(s) for _, s in pairs], 1)
    a = torch.from_numpy(np.concatenate([a for a, _ in pairs] + [np.zeros((0, 12), np.uint8)])).cuda()
    s = torch.from_numpy(np.concatenate([s for _, s in pairs] + [np.zeros((0, 12), np.uint8)])).cuda()
    path_i, path_j, length, total = (t.cpu().numpy() for t in sync.paths(a, s, files))
    out = []
    for f, n, tot in zip(files, length, total):
        at = int(f["path0"])
        out.append((path_i[at: at + n], path_j[at: at + n], int(tot)))
    return out


@pytest.fixture(scope="module")
def references():
    """reference paths of the random case, computed once per size (fast_paths: test_sync_ref ties it to paths_reference)"""
    rng = np.random.default_rng(11)
    out = {}
    for n, m in SIZES:
        a, s = SC.features(rng, n), SC.features(rng, m)
        out[n, m] = (a, s, SC.fast_paths(a, s))
    return out


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("size", SIZES, ids=lambda v: "%dx%d" % v)
def test_random_features(size, references):
    a, s, want = references[size]
    assert same(run([(a, s)])[0], want)
    if size[0] * size[1] <= 64 * 65:
        assert same(want, sync.paths_reference(a, s))


@pytest.mark.parametrize("kind", ["zeros", "extremes"])
def test_ties_and_extremes(kind):
    rng = np.random.default_rng(12)
    pairs = [(SC.features(rng, n, kind), SC.features(rng, m, kind)) for n, m in SIZES]
    for (a, s), got in zip(pairs, run(pairs)):
        assert same(got, SC.fast_paths(a, s)), (kind, len(a), len(s))


def test_a_sequence_against_its_copy_is_the_diagonal():
    rng = np.random.default_rng(13)
    for n in (1, 16, 17, 1024, 1500, 16384, 16400):                     # the last two: a panel's last strip, and past it
        a = SC.features(rng, n)
        pi, pj, total = run([(a, a.copy())])[0]
        assert total == 0 and np.array_equal(pi, np.arange(n)) and np.array_equal(pj, np.arange(n))


def test_a_score_of_more_than_one_panel():
    """16384 columns are one panel of 1024 strips; the 16385th starts the second, behind the boundary column"""
    rng = np.random.default_rng(14)
    for n, m in ((3, 16385), (40, 16400)):
        a, s = SC.features(rng, n), np.repeat(SC.features(rng, (m + 63) // 64), 64, axis=0)[:m]
        assert same(run([(a, s)])[0], SC.fast_paths(a, s)), (n, m)


def test_one_job_of_eleven_files_twice():
    rng = np.random.default_rng(15)
    sizes = [(1, 1), (0, 5), (33, 70), (5, 0), (64, 64), (200, 31), (17, 16), (1, 40), (40, 1), (129, 255), (300, 300)]
    pairs = [(SC.features(rng, n), SC.features(rng, m)) for n, m in sizes]
    first, again = run(pairs), run(pairs)
    for (a, s), got, got2 in zip(pairs, first, again):
        want = SC.fast_paths(a, s)
        assert same(got, want), (len(a), len(s))
        assert got[0].tobytes() == got2[0].tobytes() and got[1].tobytes() == got2[1].tobytes() and got[2] == got2[2]
    assert len(first[1][0]) == 0 and first[1][2] == 0 and len(first[3][0]) == 0 and first[3][2] == 0
