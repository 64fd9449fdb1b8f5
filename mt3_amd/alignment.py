"""Alignment of known notes to audio: a time shift per segment, chosen as a smooth path through the job's
(segment, shift) table of log-probabilities, and the notes warped by it.

  shift_grid(max_shift, step)        the candidate shifts in seconds
  best_paths(scores, ...)            the paths of a job on the device (mt3_op_align_paths; include/mt3_hip.h states the rule)
  best_paths_reference(scores, ...)  the rule in numpy: the yardstick of the kernel, bit for bit
  warp_notes(ns, shifts, T)          the notes moved by the path, on the host in float64

`InferenceModel.align_notes` puts them together: the tokenizer's shifts= launch, `Transformer.score_candidates` (each
segment encoded once for all shifts), `best_paths`, `warp_notes`.
"""
from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np

from . import _lib, note_sequences

# log-probability per second of jump: the middle of the range (393 .. 16,747) over which the path of the end-to-end test
# is stable on the one synthetic checkpoint there is; DESIGN.md section 6m
DEFAULT_SMOOTHNESS = 8570.0


def shift_grid(max_shift: float, step: float) -> np.ndarray:
    """The shifts -n * step .. n * step (float64, 0.0 in the middle), n = the most steps that stay within max_shift."""
    max_shift, step = float(max_shift), float(step)
    if not (np.isfinite(max_shift) and np.isfinite(step)) or step <= 0 or max_shift < 0:
        raise ValueError("shift_grid needs max_shift >= 0 and step > 0, got %r and %r" % (max_shift, step))
    n = int(np.floor(max_shift / step + 1e-9))
    if 2 * n + 1 > _lib.ALIGN_MAX_SHIFTS:
        raise ValueError("a grid of %d shifts; at most %d fit (a larger step, or a smaller max_shift)"
                         % (2 * n + 1, _lib.ALIGN_MAX_SHIFTS))
    return np.arange(-n, n + 1).astype(np.float64) * step


def _check(segments_of_file, total, grid, smoothness, max_jump):
    grid = np.ascontiguousarray(np.asarray(grid, np.float64).reshape(-1))
    counts = [int(n) for n in segments_of_file]
    if not 1 <= len(grid) <= _lib.ALIGN_MAX_SHIFTS:
        raise ValueError("the grid must hold 1 .. %d shifts, got %d" % (_lib.ALIGN_MAX_SHIFTS, len(grid)))
    if not np.all(np.isfinite(grid)) or np.any(np.diff(grid) <= 0):
        raise ValueError("the grid must be finite and strictly increasing")
    smoothness = float(smoothness)
    if not (np.isfinite(smoothness) and smoothness >= 0):
        raise ValueError("smoothness must be finite and not negative, got %r" % (smoothness,))
    max_jump = float("inf") if max_jump is None else float(max_jump)
    if not max_jump >= 0:
        raise ValueError("max_jump must not be negative, got %r" % (max_jump,))
    if any(n < 1 for n in counts):
        raise ValueError("every file needs at least 1 segment")
    if sum(counts) != total:
        raise ValueError("segments_of_file sums to %d; the table has %d rows" % (sum(counts), total))
    return counts, grid, smoothness, max_jump


def best_paths_reference(scores, segments_of_file: Sequence[int], grid, smoothness: float, max_jump: Optional[float] = None):
    """The rule of mt3_op_align_paths in numpy.  scores: float32 [total_segments, K], the files one after the other,
    file i on `segments_of_file[i]` rows.  All in float64:
        c[s][j] = -score[s][j];  D[0][j] = c[0][j]
        D[s][j] = c[s][j] + min over k with |g_j - g_k| <= max_jump of (D[s-1][k] + smoothness * |g_j - g_k|)
    the lowest k on equal values; the path ends at the lowest j of minimal D[S-1][j] and is read back through the stored k.
    -> (path int32 [total_segments], total float64 [n_files])."""
    scores = np.asarray(scores, np.float32)
    if scores.ndim != 2:
        raise ValueError("scores must be [total_segments, K], got %r" % (scores.shape,))
    counts, g, lam, max_jump = _check(segments_of_file, scores.shape[0], grid, smoothness, max_jump)
    if scores.shape[1] != len(g):
        raise ValueError("the table has %d columns for a grid of %d shifts" % (scores.shape[1], len(g)))
    jump = np.abs(g[:, None] - g[None, :])                   # [j][k]
    allowed = jump <= max_jump
    penalty = lam * jump
    path, total, first = np.zeros(scores.shape[0], np.int32), np.zeros(len(counts), np.float64), 0
    for i, S in enumerate(counts):
        c = -scores[first: first + S].astype(np.float64)
        back = np.zeros((S, len(g)), np.int64)
        D = c[0]
        for s in range(1, S):
            through = np.where(allowed, D[None, :] + penalty, np.inf)
            # the first admissible k of the least value (argmin alone would name a forbidden k when every value is inf)
            back[s] = np.argmax(allowed & (through == through.min(axis=1, keepdims=True)), axis=1)
            D = c[s] + through[np.arange(len(g)), back[s]]
        at = int(np.argmin(D))
        total[i] = D[at]
        for s in range(S - 1, 0, -1):
            path[first + s] = at
            at = int(back[s, at])
        path[first] = at
        first += S
    return path, total


def best_paths(scores, segments_of_file: Sequence[int], grid, smoothness: float, max_jump: Optional[float] = None):
    """`best_paths_reference` on the device: scores is a float32 CUDA tensor [total_segments, K] (what
    `Transformer.score_candidates` returns, viewed [segments, K]) -> (path int32 CUDA [total_segments], total float64 CUDA
    [n_files]).  Nothing is copied back and nothing is waited for."""
    import torch
    if not (hasattr(scores, "is_cuda") and scores.is_cuda and scores.dim() == 2 and scores.dtype == torch.float32):
        raise ValueError("scores must be a float32 CUDA tensor [total_segments, K]")
    counts, g, lam, max_jump = _check(segments_of_file, int(scores.shape[0]), grid, smoothness, max_jump)
    if scores.shape[1] != len(g):
        raise ValueError("the table has %d columns for a grid of %d shifts" % (scores.shape[1], len(g)))
    scores = scores.contiguous()
    total_segments, K = int(scores.shape[0]), len(g)
    files = np.zeros((len(counts), 2), np.int32)
    files[:, 1] = counts
    files[1:, 0] = np.cumsum(counts)[:-1]
    back = torch.empty(max(total_segments * K, 1), device="cuda", dtype=torch.uint8)
    path = torch.empty(total_segments, device="cuda", dtype=torch.int32)
    total = torch.empty(len(counts), device="cuda", dtype=torch.float64)
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_align_paths(scores.data_ptr(), total_segments, K, files.ctypes.data, len(counts),
                                              g.ctypes.data, lam, max_jump, back.data_ptr(), path.data_ptr(),
                                              total.data_ptr(), stream.cuda_stream))
    for t in (scores, back):
        t.record_stream(stream)
    return path, total


def check_jumps(grid, max_jump, segment_seconds: float):
    """ValueError if a path over `grid` under `max_jump` may jump by `segment_seconds` or more between two segments: the
    warp is then no longer monotone.  -> the largest jump a path can make."""
    grid = np.asarray(grid, np.float64).reshape(-1)
    gaps = np.abs(grid[:, None] - grid[None, :])
    limit = float("inf") if max_jump is None else float(max_jump)
    largest = float(gaps[gaps <= limit].max()) if gaps.size else 0.0
    if largest >= float(segment_seconds):
        raise ValueError("a path may jump by %.6g s between segments of %.6g s: the jump must stay below the segment "
                         "(a smaller max_shift or max_jump)" % (largest, float(segment_seconds)))
    return largest


def shift_at(times, path_shifts, segment_seconds: float) -> np.ndarray:
    """delta(t) of `warp_notes` at the given times (float64)"""
    shifts = np.asarray(path_shifts, np.float64).reshape(-1)
    if len(shifts) < 1:
        raise ValueError("path_shifts must hold at least 1 segment")
    anchors = (np.arange(len(shifts)) + 0.5) * float(segment_seconds)
    return np.interp(np.asarray(times, np.float64), anchors, shifts)


def warp_notes(ns, path_shifts, segment_seconds: float):
    """The notes of `ns` moved by a shift path (seconds per segment of `segment_seconds`): a new NoteSequence.
    The offset is a function of time: delta(a_s) = path_shifts[s] at the anchors a_s = (s + 0.5) * segment_seconds, linear
    between anchors, the first segment's shift before a_0 and the last one's after a_{S-1}.  Every note time t, start and
    end alike, becomes max(t + delta(t), 0); every other field is kept.  Two neighbouring shifts must differ by less
    than `segment_seconds` (ValueError): t + delta(t) then never decreases and end >= start survives."""
    shifts = np.asarray(path_shifts, np.float64).reshape(-1)
    T = float(segment_seconds)
    if not (np.isfinite(T) and T > 0):
        raise ValueError("segment_seconds must be positive, got %r" % (segment_seconds,))
    if not np.all(np.isfinite(shifts)):
        raise ValueError("path_shifts must be finite")
    if len(shifts) > 1 and float(np.abs(np.diff(shifts)).max()) >= T:
        raise ValueError("neighbouring segments' shifts differ by %.6g s, not less than the segment's %.6g s"
                         % (float(np.abs(np.diff(shifts)).max()), T))
    start = np.array([n.start_time for n in ns.notes], np.float64)
    end = np.array([n.end_time for n in ns.notes], np.float64)
    start = np.maximum(start + shift_at(start, shifts, T), 0.0)
    end = np.maximum(end + shift_at(end, shifts, T), 0.0)
    notes = [dataclasses.replace(n, start_time=float(a), end_time=float(b)) for n, a, b in zip(ns.notes, start, end)]
    return note_sequences.NoteSequence(notes=notes, total_time=float(end.max()) if len(end) else 0.0,
                                       ticks_per_quarter=ns.ticks_per_quarter)
