"""Piano rolls of NoteSequences and frame-level (TP, FP, FN) counts, rasterised and counted on the device
(mt3_op_pianoroll / mt3_op_frame_counts; the rule: include/mt3_hip.h, "piano rolls and frame counts").

The device side of `metrics_utils.get_prettymidi_pianoroll` / `metrics_utils.frame_metrics` and of
`metrics.frame_scores`: all the rolls of a job come from ONE upload of the packed notes and ONE rasterise call, all the
counts of a job from one count call and one copy of 24 bytes per pair back to the host.  There is no host fallback.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

from . import _lib, note_arrays

PITCHES = _lib.PIANOROLL_PITCHES
MIN_NOTE_SECONDS = _lib.PIANOROLL_MIN_NOTE_SECONDS
DEFAULT_FPS = 62.5                      # mt3/metrics.py: frame_fps
DEFAULT_VELOCITY_THRESHOLD = 30         # mt3/metrics.py: frame_velocity_threshold
LAYOUT = ("<f8", "<f8", "<i4", "<i4", "<i4")      # the types of the columns that _pack lays out


def roll_width(start: np.ndarray, end: np.ndarray, drum: np.ndarray, fps: float, is_drum: bool) -> int:
    """F of one roll: int(fps * max end) over all notes, drum notes included, after the 0.05 s rule -- in float64, the
    expression the kernel's indices use.  The one place widths come from."""
    if len(start) == 0:
        return 0
    short = np.ones(len(start), bool) if is_drum else (end - start < MIN_NOTE_SECONDS)
    return max(0, int(float(fps) * float(np.where(short, start + MIN_NOTE_SECONDS, end).max())))


def _pack(sequences, fps: float, is_drum: bool):
    """the job's notes as one byte buffer (start f64 | end f64 | pitch i32 | velocity i32 | is_drum i32, each [n]) and the
    host tables: note offsets int64 [n_rolls + 1], widths int32 [n_rolls]"""
    fps = float(fps)
    if not np.isfinite(fps) or fps <= 0:
        raise ValueError("fps must be finite and positive, got %r" % (fps,))
    parts = [note_arrays.fields(s) for s in sequences]
    offs = note_arrays.offsets([len(p[0]) for p in parts])
    widths = np.zeros(len(parts), np.int32)
    for i, (start, end, pitch, velocity, drum) in enumerate(parts):
        note_arrays.check_range("sequence %d: a piano roll has pitches 0 .. 127" % i, pitch)
        note_arrays.check_times(start, end, not_negative=True, prefix="sequence %d: " % i)
        if (np.abs(velocity) >= 2 ** 31).any():
            raise ValueError("sequence %d: velocities must fit int32" % i)
        w = roll_width(start, end, drum, fps, is_drum)
        if w >= 2 ** 31:
            raise ValueError("sequence %d: %d frames do not fit a roll" % (i, w))
        widths[i] = w
    return note_arrays.pack([[p[k] for p in parts] for k in range(5)], LAYOUT), int(offs[-1]), offs, widths


def _rasterise(sequences, fps: float, is_drum: bool):
    """-> (the float32 buffer of all rolls, column offsets int64 [n_rolls], widths int32 [n_rolls]); roll i is
    buffer[128 * col[i] : 128 * (col[i] + width[i])] as [128, width[i]]"""
    import torch
    packed, n, offs, widths = _pack(sequences, fps, is_drum)
    cols = note_arrays.offsets(widths)
    total = PITCHES * int(cols[-1])
    out = torch.empty(total, device="cuda", dtype=torch.float32)
    if total == 0:
        return out, cols[:-1], widths
    notes, ptr = note_arrays.upload(packed, n, LAYOUT)             # the one upload
    _lib.check(_lib.load().mt3_op_pianoroll(*ptr, n, len(widths), offs.ctypes.data, cols.ctypes.data, widths.ctypes.data,
                                            float(fps), 1 if is_drum else 0, out.data_ptr(), total,
                                            torch.cuda.current_stream().cuda_stream))
    return out, cols[:-1], widths


def _views(out, cols, widths) -> list:
    return [out[PITCHES * int(c): PITCHES * (int(c) + int(w))].view(PITCHES, int(w)) for c, w in zip(cols, widths)]


def pianorolls(sequences: Sequence, fps: float = DEFAULT_FPS, is_drum: bool = False) -> list:
    """The piano rolls of `sequences` (NoteSequences; NOTE_DTYPE record arrays are taken too): a list of float32 CUDA
    tensors [128, F_i], views of one buffer written by one mt3_op_pianoroll call after one upload of the packed notes.
    roll[pitch, int(start * fps) : int(end * fps)] += velocity per note, F_i = int(fps * latest end), notes shorter than
    0.05 s (all notes with is_drum=True) lengthened to 0.05 s, drum notes silent unless is_drum=True -- the rule of
    metrics_utils.get_prettymidi_pianoroll (include/mt3_hip.h).  The sequences are not modified.  ValueError for a pitch
    outside 0 .. 127 or a negative or non-finite time.  An empty list gives an empty list."""
    sequences = list(sequences)
    if not sequences:
        return []
    return _views(*_rasterise(sequences, fps, is_drum))


def _count(rolls_buffer, ref_cols, ref_widths, est_cols, est_widths, velocity_threshold: int) -> np.ndarray:
    import torch
    n = len(ref_cols)
    if n == 0:
        return np.zeros((0, 3), np.int64)
    counts = torch.empty((n, 3), device="cuda", dtype=torch.int64)
    tables = [np.ascontiguousarray(ref_cols, np.int64), np.ascontiguousarray(ref_widths, np.int32),
              np.ascontiguousarray(est_cols, np.int64), np.ascontiguousarray(est_widths, np.int32)]
    _lib.check(_lib.load().mt3_op_frame_counts(rolls_buffer.data_ptr() if rolls_buffer.numel() else None,
                                               rolls_buffer.numel(), n, *[t.ctypes.data for t in tables],
                                               int(velocity_threshold), counts.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
    return counts.cpu().numpy()                        # the one copy back: 24 n bytes


def _threshold(velocity_threshold) -> int:
    if int(velocity_threshold) != velocity_threshold:
        raise ValueError("velocity_threshold must be an integer (the reference's is), got %r" % (velocity_threshold,))
    return int(velocity_threshold)


def frame_counts(ref_sequences: Sequence, est_sequences: Sequence, fps: float = DEFAULT_FPS,
                 velocity_threshold: int = DEFAULT_VELOCITY_THRESHOLD, is_drum: bool = False) -> np.ndarray:
    """(TP, FP, FN) of every (ref_sequences[i], est_sequences[i]) pair: int64 numpy [n, 3].  A cell is on in the reference
    where its roll is > velocity_threshold and on in the estimate where its roll is > 0; the narrower roll counts as zero
    past its own width.  All 2n rolls come from one rasterise call, the counts from one count call and one copy."""
    ref_sequences, est_sequences = list(ref_sequences), list(est_sequences)
    if len(ref_sequences) != len(est_sequences):
        raise ValueError("%d reference sequences, %d estimated" % (len(ref_sequences), len(est_sequences)))
    thr, n = _threshold(velocity_threshold), len(ref_sequences)
    if n == 0:
        return np.zeros((0, 3), np.int64)
    out, cols, widths = _rasterise(ref_sequences + est_sequences, fps, is_drum)
    return _count(out, cols[:n], widths[:n], cols[n:], widths[n:], thr)


def roll_pair_counts(ref_roll, est_roll, velocity_threshold: int = DEFAULT_VELOCITY_THRESHOLD) -> Tuple[int, int, int]:
    """(TP, FP, FN) of two rolls [128, F_ref], [128, F_est] that already exist: numpy arrays or CUDA tensors of any real
    dtype (taken to float32).  One small buffer holds both for the count call."""
    import torch
    thr = _threshold(velocity_threshold)
    pair = [torch.as_tensor(r).to(device="cuda", dtype=torch.float32) for r in (ref_roll, est_roll)]
    for r in pair:
        if r.ndim != 2 or r.shape[0] != PITCHES:
            raise ValueError("a piano roll is [128, frames], got %s" % (tuple(r.shape),))
    widths = np.array([r.shape[1] for r in pair], np.int32)
    cols = np.array([0, widths[0]], np.int64)
    buf = torch.cat([r.contiguous().reshape(-1) for r in pair])
    tp, fp, fn = _count(buf, cols[:1], widths[:1], cols[1:], widths[1:], thr)[0]
    return int(tp), int(fp), int(fn)


def precision_recall_f1(tp: int, fp: int, fn: int) -> Tuple[float, float, float]:
    """sklearn.metrics.precision_recall_fscore_support's values for the positive class: each 0.0 where its denominator is
    0 (sklearn also warns there; this does not)"""
    tp, fp, fn = int(tp), int(fp), int(fn)
    p = tp / (tp + fp) if tp + fp else 0.0
    r = tp / (tp + fn) if tp + fn else 0.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)
