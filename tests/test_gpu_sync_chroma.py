"""mt3_op_logmel_chroma and mt3_op_note_chroma on the device EQUAL their numpy rules, byte for byte."""
import numpy as np
import pytest
import torch

from mt3_amd import sync

pytestmark = pytest.mark.gpu


def logmel_job(rng, n_mel, pool, frames):
    """files back to back, each with a few rows of padding after its valid frames, the last one short"""
    rows_per_file = [n + 3 for n in frames]
    files = sync.file_table(frames, [0] * len(frames), [0] * len(frames), pool, rows_per_file)
    lm = rng.normal(0.0, 3.0, (sum(rows_per_file), n_mel)).astype(np.float32)
    lm[rng.random(lm.shape) < 0.05] = -np.inf
    lm[rng.random(lm.shape) < 0.03] = np.nan
    lm[rng.random(len(lm)) < 0.1] = np.nan                               # NaN rows
    lm[rng.random(len(lm)) < 0.1] = 1.5                                  # all-equal rows
    lm[rng.random(len(lm)) < 0.1] = -7.0                                 # below the floor: silent unless pooled with more
    bins = rng.integers(-1, 13, n_mel).astype(np.int8)                   # -1 and 12: unused
    return lm, files, bins


@pytest.mark.parametrize("n_mel", [8, 512, 30])
@pytest.mark.parametrize("pool", [1, 5, 16])
def test_logmel_chroma_equals_the_rule(pool, n_mel):
    rng = np.random.default_rng(100 * pool + n_mel)
    frames = [0, 1, pool - 1, pool, pool + 1, 3 * pool + 2, 40, 2 * pool, 2]
    lm, files, bins = logmel_job(rng, n_mel, pool, frames)
    lm[int(files["row0"][-2]): int(files["row0"][-2]) + 2 * pool] = -7.0     # a file below the floor: silent frames
    want = sync.logmel_chroma_reference(lm, files, bins, pool, 4.0, 0.0)
    got = sync.logmel_chroma(torch.from_numpy(lm).cuda(), files, bins, pool=pool, range=4.0, floor=0.0).cpu().numpy()
    assert got.shape == want.shape == (int(files["n"].sum()), 12) and np.array_equal(got, want)
    assert want.any() and (want.max(1) == 0).any()                       # sounding frames and silent ones
    if n_mel == 512:                                                     # the single-float path: a log-mel off the 16 bytes
        shifted = torch.zeros(lm.size + 1, dtype=torch.float32, device="cuda")
        shifted[1:] = torch.from_numpy(lm.reshape(-1)).cuda()
        got = sync.logmel_chroma(shifted[1:].view(len(lm), n_mel), files, bins, pool=pool, range=4.0, floor=0.0)
        assert np.array_equal(got.cpu().numpy(), want)


def test_logmel_chroma_with_another_range_and_floor():
    rng = np.random.default_rng(7)
    lm, files, bins = logmel_job(rng, 512, 5, [37, 11])
    for rng_, floor in ((1.0, -1.0), (10.0, 2.5), (3.3, float("-inf"))):
        want = sync.logmel_chroma_reference(lm, files, bins, 5, rng_, floor)
        got = sync.logmel_chroma(torch.from_numpy(lm).cuda(), files, bins, pool=5, range=rng_, floor=floor).cpu().numpy()
        assert np.array_equal(got, want), (rng_, floor)


@pytest.mark.parametrize("weights", [(255,), (255, 128, 64, 32, 16, 8)])
def test_note_chroma_equals_the_rule(weights):
    rng = np.random.default_rng(len(weights))
    cols = [[], [], []]

    def add(j0, j1, pitch):
        for col, v in zip(cols, (j0, j1, pitch)):
            col.append(np.asarray(v, np.int32).reshape(-1))
        return len(np.asarray(j0).reshape(-1))

    counts, ms = [], []
    # file 0: short notes (one frame), random notes, and a note past the end, a negative start and a bad pitch: skipped
    n = add([3, 3, 9], [4, 4, 10], [60, 61, 127]) + add(rng.integers(0, 500, 200), rng.integers(0, 540, 200),
                                                        rng.integers(0, 128, 200))
    n += add([10, -1, 5, 700], [700, 4, 9, 701], [64, 64, 128, 64])
    counts.append(n), ms.append(600)
    counts.append(add([], [], [])), ms.append(0)                         # file 1: no notes
    counts.append(add(np.full(300, 2), np.full(300, 9), np.full(300, 45))), ms.append(9)      # file 2: 300 stacked notes
    counts.append(add([0], [1], [0])), ms.append(1)                      # file 3: one frame
    j0, j1, pitch = (np.concatenate(c) for c in cols)
    j1 = np.where((j1 <= j0) & (j0 >= 0) & (j0 < 600), j0 + 1, j1).astype(np.int32)
    files = sync.file_table([0] * 4, counts, ms, 5)
    want = sync.note_chroma_reference(j0, j1, pitch, files, weights)
    got = sync.note_chroma((j0, j1, pitch), files, weights).cpu().numpy()
    assert got.shape == want.shape == (610, 12) and np.array_equal(got, want)
    assert want[600 + 2: 600 + 9, 45 % 12].tolist() == [255] * 7 and want.max() == 255
    again = sync.note_chroma((j0, j1, pitch), files, weights).cpu().numpy()
    assert again.tobytes() == got.tobytes()
