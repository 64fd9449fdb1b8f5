"""What the synchronisation tests share: the end-to-end piece (a score, its performance under a smooth tempo curve, the
performance's audio), the numpy rules run as one pipeline, and random feature blocks.  No test in here."""
import dataclasses
import functools

import numpy as np

from mt3_amd import note_sequences as N
from mt3_amd import sync, synthetic

SECONDS, SEED, LEAD_IN, TAIL = 16.0, 7, 0.5, 0.05      # TAIL: the last note's 40 ms release
# Measured 2026-10-21 with the numpy rules (default keywords) on oracle.frontend.compute_logmel(float32, tf32 tables) of
# piece(): the onset error of the synchronised score against the performed onsets.  The asserted bound is that maximum
# plus one feature frame (pool / 125 s): one quantised cell moves a path by at most one frame.
MEASURED_MAX, MEASURED_MEDIAN = 0.2544, 0.0508
BOUND = MEASURED_MAX + sync.DEFAULT_POOL / 125.0


def tempo(t):
    """the performance's tempo relative to the score's at score time t: smooth, between 0.8x and 1.25x"""
    return np.exp(np.log(1.25) * np.sin(2.0 * np.pi * np.asarray(t, np.float64) / 11.0))


def performed(t):
    """score time -> performance time: LEAD_IN plus the integral of 1 / tempo, on a 1 ms grid"""
    grid = np.arange(0.0, SECONDS + 1.0, 0.001)
    elapsed = np.concatenate([[0.0], np.cumsum(0.001 / tempo(grid[:-1] + 0.0005))])
    return LEAD_IN + np.interp(np.asarray(t, np.float64), grid, elapsed)


@functools.lru_cache(maxsize=None)
def piece(device: str = "cpu"):
    """(score NoteSequence, performance NoteSequence, performance audio float32 [n] at 16 kHz)"""
    score = synthetic.random_music(SECONDS, seed=SEED)
    played = N.NoteSequence(notes=[dataclasses.replace(n, start_time=float(performed(n.start_time)),
                                                       end_time=float(performed(n.end_time))) for n in score.notes])
    played.total_time = max(n.end_time for n in played.notes)
    n_samples = int(round((played.total_time + TAIL) * 16000))
    amps = np.random.default_rng(SEED + 1).uniform(0.3, 1.0, len(played.notes))
    wav = synthetic.render_notes([n.start_time for n in played.notes], [n.end_time for n in played.notes],
                                 [n.pitch for n in played.notes], amps, np.zeros(len(played.notes), np.int64), 1, n_samples,
                                 seed=SEED, device=device)
    return score, played, wav.reshape(-1).cpu().numpy()


def numpy_synchronize(logmel, ns, bins, **kw):
    """the three numpy rules on one file's [frames, mel] log-mel -> `sync.record`"""
    pool = kw.pop("pool", sync.DEFAULT_POOL)
    weights = kw.pop("harmonic_weights", sync.DEFAULT_WEIGHTS)
    packed = sync.pack([ns], [len(logmel)], [len(logmel)], pool, sync.LOGMEL_FPS / pool)
    j0, j1, pitch = (packed.notes[4 * packed.n_notes * k: 4 * packed.n_notes * (k + 1)].view("<i4") for k in range(3))
    a = sync.logmel_chroma_reference(logmel, packed.files, bins, pool, **kw)
    s = sync.note_chroma_reference(j0, j1, pitch, packed.files, weights)
    path_i, path_j, total = fast_paths(a, s)
    return sync.record(ns, path_i, path_j, total, sync.LOGMEL_FPS / pool)


def fast_paths(a, s):
    """`sync.paths_reference`'s result by rows: numpy over the columns for the two predecessors of the row above, a plain
    loop for the one to the left.  (test_sync_ref checks it against paths_reference and the brute force.)"""
    a, s = np.asarray(a, np.int64), np.asarray(s, np.int64)
    n, m = len(a), len(s)
    if n == 0 or m == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    big = np.int64(1) << 60
    back = np.zeros((n, m), np.int8)
    prev = None
    for i in range(n):
        cost = np.abs(a[i][None, :] - s).sum(1)
        if prev is None:
            above, choice = np.full(m, big), np.zeros(m, np.int8)
            above[0] = 0
        else:
            diag = np.concatenate([[big], prev[:-1]])
            choice = (prev < diag).astype(np.int8)
            above = np.where(choice == 1, prev, diag)
        row = np.empty(m, np.int64)
        left = big
        above, cost_l, ch = above.tolist(), cost.tolist(), choice.tolist()
        out = []
        for j in range(m):
            best = above[j]
            if left < best:
                best, ch[j] = left, 2
            left = best + cost_l[j]
            out.append(left)
        row[:] = out
        back[i] = ch
        prev = row
    i, j, pi, pj = n - 1, m - 1, [], []
    while True:
        pi.append(i), pj.append(j)
        if i == 0 and j == 0:
            break
        c = back[i, j]
        i, j = (i - 1, j - 1) if c == 0 else (i - 1, j) if c == 1 else (i, j - 1)
    return np.array(pi[::-1], np.int32), np.array(pj[::-1], np.int32), int(prev[m - 1])


def onset_errors(synced, played):
    """|synchronised onset - performed onset| per note (the notes keep their order)"""
    return np.abs(np.array([n.start_time for n in synced.notes]) - np.array([n.start_time for n in played.notes]))


def features(rng, n, kind="random"):
    """uint8 [n, 12] feature rows"""
    if kind == "zeros":
        return np.zeros((n, 12), np.uint8)
    if kind == "extremes":
        return (rng.integers(0, 2, (n, 12)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (n, 12)).astype(np.uint8)
