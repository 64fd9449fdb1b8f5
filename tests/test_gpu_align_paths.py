"""mt3_op_align_paths on the GPU against `alignment.best_paths_reference` (which tests/test_alignment_ref.py holds against
all K^S paths): paths ==, totals bit-equal.  One ragged job of files of 1, 300, 2, 3 and 3 segments per case."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import alignment  # noqa: E402
from tests import alignment_ref as ar  # noqa: E402

INF = float("inf")


def _grid(K, uniform=True):
    if uniform:
        return (np.arange(K) - K // 2).astype(np.float64) * 0.02
    return np.sort(np.random.default_rng(K).uniform(-0.3, 0.3, K))


def _both(scores, counts, grid, lam, max_jump):
    want_path, want_total = alignment.best_paths_reference(scores, counts, grid, lam, max_jump)
    path, total = alignment.best_paths(torch.from_numpy(scores).cuda(), counts, grid, lam, max_jump)
    path, total = path.cpu().numpy(), total.cpu().numpy()
    assert path.dtype == np.int32 and total.dtype == np.float64
    bad = np.flatnonzero(path != want_path)
    assert bad.size == 0, (bad[:8].tolist(), path[bad[:8]].tolist(), want_path[bad[:8]].tolist())
    assert np.array_equal(total.view(np.uint64), want_total.view(np.uint64)), (total.tolist(), want_total.tolist())
    return path, total


@pytest.mark.parametrize("K", [1, 2, 63, 64])
@pytest.mark.parametrize("kind", ["float", "ties"])
def test_kernel_equals_the_rule(K, kind):
    scores, counts = ar.ragged_job(np.random.default_rng(1000 + K), K, kind)
    grid = _grid(K)
    step = 0.02 if kind == "float" else 1.0
    if kind == "ties":
        grid = np.arange(K, dtype=np.float64)                # integer jumps and penalties: equal costs everywhere
    for lam in (0.0, 1.0 if kind == "ties" else 37.5, 1e9):
        for max_jump in (INF, 3 * step, 0.5 * step):
            path, _ = _both(scores, counts, grid, lam, max_jump)
            if max_jump < step:
                first = 0
                for n in counts:                             # below the grid step: constant paths
                    assert np.all(path[first: first + n] == path[first])
                    first += n


def test_non_uniform_grid_and_the_zero_table():
    K = 17
    scores, counts = ar.ragged_job(np.random.default_rng(5), K, "float")
    for lam, max_jump in [(20.0, INF), (150.0, 0.11), (0.0, 0.05)]:
        _both(scores, counts, _grid(K, uniform=False), lam, max_jump)
    zero, counts = ar.ragged_job(None, 64, "zero")
    path, total = _both(zero, counts, _grid(64), 5.0, INF)
    assert not path.any() and not total.any()                # all equal: index 0 throughout


def test_two_launches_give_the_same_bits_and_many_files_take_several_launches():
    rng = np.random.default_rng(9)
    K, counts = 21, [int(n) for n in rng.integers(1, 12, 150)]          # 150 files: three launches of 64, 64 and 22
    scores = (-rng.uniform(5, 300, (sum(counts), K))).astype(np.float32)
    grid = alignment.shift_grid(0.2, 0.02)
    a_path, a_total = _both(scores, counts, grid, 25.0, INF)
    b_path, b_total = _both(scores, counts, grid, 25.0, INF)
    assert np.array_equal(a_path, b_path) and np.array_equal(a_total.view(np.uint64), b_total.view(np.uint64))
