"""Synchronise a score to a recording: chroma of the audio from the log-mel the engine already holds, chroma of the score
from its notes, and the dynamic-time-warping path between the two (mt3_op_logmel_chroma, mt3_op_note_chroma,
mt3_op_sync_paths; the rules: include/mt3_hip.h, "score-to-audio synchronisation", derived in DESIGN 6s).

  chroma_bins(mel_matrix)                      the host-built table: each mel bin's pitch class, or -1
  logmel_chroma_reference / note_chroma_reference / paths_reference
                                               the rules, stated once in numpy: the yardsticks, bit for bit
  logmel_chroma / note_chroma / paths          the device calls: CUDA tensors in, CUDA tensors out, nothing copied back
  warp_times / warp_notes                      a path as a map from score time to audio time (host, float64)
  synchronize(logmels, sequences)              every file of a job: one pack, one upload, the three op calls, one copy
                                               back of the paths

`align_notes` repairs labels that drift by a fraction of a second; this is the step before it, for a SCORE (quantised,
another tempo, ritardandi) against a PERFORMANCE: `synchronize` for the tempo, then `align_notes` for the last +-0.2 s.
The audio feature is the largest log-mel value per pitch class over `pool` frames, relative to the frame's loudest class
and quantised to a byte over `range` natural-log units (max-log chroma: this project's own feature, parity with no
library is claimed); the score feature is a clipped sum of integer weights per class; the cost of a cell is the L1
distance of two such rows and the path is the plain three-step DTW in int32 with a fixed tie order.  range, floor, fmin,
fmax, pool and the harmonic weights are design choices, not measurements (DESIGN 6s records the error they give on one
synthetic piece).  Limits: full-to-full alignment, no band constraint (MAX_CELLS is the guard), no repeats or skips, drums
carry no chroma, programs are ignored, one workgroup per file.  There is no host fallback: the device calls need the
library and a device.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List

import numpy as np

from . import _lib, note_arrays

CLASSES = _lib.SYNC_CLASSES
MAX_POOL, MAX_FRAMES, MAX_CELLS = _lib.SYNC_MAX_POOL, _lib.SYNC_MAX_FRAMES, _lib.SYNC_MAX_CELLS
LANES, STRIP = _lib.SYNC_LANES, _lib.SYNC_STRIP
OFFSETS = (0, 12, 19, 24, 28, 31)                     # the semitones of a note's harmonics 1 .. 6
LOGMEL_FPS = 125.0
DEFAULT_POOL, DEFAULT_RANGE, DEFAULT_FLOOR = 5, 4.0, 0.0
DEFAULT_FMIN, DEFAULT_FMAX = 250.0, 4400.0
DEFAULT_WEIGHTS = (255,)
NOTE_LAYOUT = ("<i4", "<i4", "<i4")                   # j0 | j1 | pitch
FILE_DTYPE = np.dtype([("row0", "<i8"), ("first", "<i8"), ("a0", "<i8"), ("s0", "<i8"), ("path0", "<i8"),
                       ("work0", "<i8"), ("n_frames", "<i4"), ("n_notes", "<i4"), ("n", "<i4"), ("m", "<i4")])   # mt3_sync_file


def chroma_bins(mel_matrix, fmin: float = DEFAULT_FMIN, fmax: float = DEFAULT_FMAX, sample_rate: int = 16000,
                fft_size: int = 2048) -> np.ndarray:
    """int8 [mel]: each mel bin's pitch class 0 .. 11, or -1 for unused.  A bin's centre is the frequency of the FFT row
    where its column of the [fft_size / 2 + 1, mel] matrix is largest (the lowest row on a tie); its pitch is
    69 + 12 log2(f / 440) in float64 and its class floor(pitch + 0.5) mod 12; a centre below fmin or above fmax (an
    all-zero column's centre is 0 Hz) gives -1.  An FFT row is sample_rate / fft_size = 7.8 Hz wide and a semitone spans
    two rows only from about 260 Hz on, so the default fmin is 250 Hz, a quarter tone below C4: below it neighbouring
    pitch classes share FFT rows, and lower notes are seen through their harmonics.  The default fmax, 4400 Hz, lies a
    quarter tone above C8, the top of the piano."""
    w = np.asarray(mel_matrix)
    if w.ndim != 2 or w.shape[0] != fft_size // 2 + 1:
        raise ValueError("mel_matrix must be [fft_size / 2 + 1, mel], got %r" % (w.shape,))
    if not (math.isfinite(fmin) and math.isfinite(fmax) and 0 < fmin <= fmax):
        raise ValueError("0 < fmin <= fmax must hold, got %r, %r" % (fmin, fmax))
    centre = np.argmax(w, axis=0).astype(np.float64) * (float(sample_rate) / float(fft_size))
    out = np.full(w.shape[1], -1, np.int8)
    ok = (centre >= float(fmin)) & (centre <= float(fmax))
    pitch = 69.0 + 12.0 * np.log2(centre[ok] / 440.0)
    out[ok] = (np.floor(pitch + 0.5).astype(np.int64) % 12).astype(np.int8)
    return out


def feature_frames(n_frames, pool: int) -> np.ndarray:
    """ceil(n_frames / pool)"""
    return (np.asarray(n_frames, np.int64) + int(pool) - 1) // int(pool)


def note_frames(start, end, fps: float):
    """(j0, j1) int32: j0 = floor(start * fps), j1 = max(j0 + 1, floor(end * fps)), in float64; what does not fit int32
    is cut to its ends, outside every file"""
    a = np.clip(np.floor(np.asarray(start, np.float64) * float(fps)), -1, 2 ** 31 - 2)
    b = np.clip(np.floor(np.asarray(end, np.float64) * float(fps)), -1, 2 ** 31 - 2)
    return a.astype(np.int32), np.maximum(a + 1, b).astype(np.int32)


def workspace_words(n: int, m: int) -> int:
    """mt3s_workspace_words: a file's int32 words of workspace"""
    if n <= 0 or m <= 0:
        return 0
    strips = (int(m) + STRIP - 1) // STRIP
    full, rest = divmod(strips, LANES)
    return full * (int(n) + LANES - 1) * LANES + ((int(n) + rest - 1) * rest if rest else 0) + int(n)


def path_capacity(n: int, m: int) -> int:
    return int(n) + int(m) - 1 if n > 0 and m > 0 else 0


def file_table(n_frames, n_notes, m, pool: int, rows_per_file=None) -> np.ndarray:
    """FILE_DTYPE [n_files] of a job whose ranges lie back to back in file order (rows: rows_per_file, default n_frames)"""
    t = np.zeros(len(n_frames), FILE_DTYPE)
    t["n_frames"], t["n_notes"], t["m"] = n_frames, n_notes, m
    t["n"] = feature_frames(n_frames, pool)
    t["row0"] = note_arrays.offsets(t["n_frames"] if rows_per_file is None else rows_per_file)[:-1]
    t["first"] = note_arrays.offsets(t["n_notes"])[:-1]
    t["a0"], t["s0"] = note_arrays.offsets(t["n"])[:-1], note_arrays.offsets(t["m"])[:-1]
    t["path0"] = note_arrays.offsets([path_capacity(a, b) for a, b in zip(t["n"], t["m"])])[:-1]
    t["work0"] = note_arrays.offsets([workspace_words(a, b) for a, b in zip(t["n"], t["m"])])[:-1]
    return t


# ---------------------------------------------------------------------------------------------------------- the rules
def logmel_chroma_reference(logmel, files, bins, pool: int = DEFAULT_POOL, range: float = DEFAULT_RANGE,
                            floor: float = DEFAULT_FLOOR) -> np.ndarray:
    """THE RULE, audio.  logmel float32 [rows, mel]; files: FILE_DTYPE records (row0, n_frames, a0, n); bins int8 [mel].
    -> uint8 [sum n, 12] (files back to back from a0 = 0 on).  Per feature frame: v[c] = np.fmax over its rows and the
    bins of class c; mx = fmax over c; q[c] = clamp(floor(((v[c] - mx) + range) * float32(255 / range))) in float32, NaN
    and unmeasured -> 0; all zeros unless mx >= floor."""
    logmel = np.asarray(logmel, np.float32)
    bins = np.asarray(bins, np.int8)
    rng, scale = np.float32(range), np.float32(255.0 / np.float64(np.float32(range)))
    total = int(max([int(f["a0"]) + int(f["n"]) for f in files], default=0))
    out = np.zeros((total, CLASSES), np.uint8)
    members = [np.flatnonzero(bins == c) for c in np.arange(CLASSES)]
    for f in files:
        for i in np.arange(int(f["n"])):
            r0 = int(f["row0"]) + int(i) * int(pool)
            r1 = int(f["row0"]) + min((int(i) + 1) * int(pool), int(f["n_frames"]))
            block = logmel[r0:r1]
            v = np.full(CLASSES, np.nan, np.float32)
            for c, which in enumerate(members):
                if len(which) and block.size:
                    v[c] = np.fmax.reduce(block[:, which].reshape(-1))
            mx = np.fmax.reduce(v)
            if not mx >= np.float32(floor):
                continue
            with np.errstate(invalid="ignore"):                         # inf - inf: NaN, 0
                t = np.floor(((v - mx) + rng) * scale)
            q = np.where(t >= 255, 255, np.where(t >= 0, t, 0))
            out[int(f["a0"]) + int(i)] = q.astype(np.uint8)
    return out


def note_chroma_reference(j0, j1, pitch, files, weights=DEFAULT_WEIGHTS) -> np.ndarray:
    """THE RULE, score.  j0, j1, pitch: int32 per note; files: FILE_DTYPE records (first, n_notes, s0, m).
    -> uint8 [sum m, 12]: s[j][c] = min(255, the sum of weights[h] over the notes and harmonics h with
    (pitch + OFFSETS[h]) mod 12 == c and j0 <= j < j1); a note with pitch outside 0 .. 127, j0 outside [0, m) or j1
    outside (j0, m] adds nothing."""
    total = int(max([int(f["s0"]) + int(f["m"]) for f in files], default=0))
    acc = np.zeros((total, CLASSES), np.int64)
    for f in files:
        m, s0 = int(f["m"]), int(f["s0"])
        for i in np.arange(int(f["first"]), int(f["first"]) + int(f["n_notes"])):
            a, b, p = int(j0[i]), int(j1[i]), int(pitch[i])
            if not (0 <= p <= 127 and 0 <= a < m and a < b <= m):
                continue
            for h, w in enumerate(weights):
                acc[s0 + a: s0 + b, (p + OFFSETS[h]) % 12] += int(w)
    return np.minimum(acc, 255).astype(np.uint8)


def paths_reference(a, s):
    """THE RULE, path, for ONE file.  a uint8 [N, 12], s uint8 [M, 12] -> (path_i int32, path_j int32, total int).
    cost(i, j) = sum |a[i] - s[j]|; D[i][j] = cost + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) over the predecessors that
    exist, the first of equal values in that order; the path from (N-1, M-1) back to (0, 0), returned in forward order.
    N == 0 or M == 0: empty path, total 0.  Plain loops: for small sizes."""
    a, s = np.asarray(a, np.int64).reshape(-1, CLASSES), np.asarray(s, np.int64).reshape(-1, CLASSES)
    N, M = len(a), len(s)
    if N == 0 or M == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    cost = np.abs(a[:, None, :] - s[None, :, :]).sum(2)
    D = np.zeros((N, M), np.int64)
    back = np.zeros((N, M), np.int8)
    for i in range(N):
        for j in range(M):
            if i == 0 and j == 0:
                D[i, j] = cost[i, j]
                continue
            best, ch = None, 0
            if i > 0 and j > 0:
                best, ch = D[i - 1, j - 1], 0
            if i > 0 and (best is None or D[i - 1, j] < best):
                best, ch = D[i - 1, j], 1
            if j > 0 and (best is None or D[i, j - 1] < best):
                best, ch = D[i, j - 1], 2
            D[i, j], back[i, j] = cost[i, j] + best, ch
    i, j, pi, pj = N - 1, M - 1, [], []
    while True:
        pi.append(i), pj.append(j)
        if i == 0 and j == 0:
            break
        ch = back[i, j]
        i, j = (i - 1, j - 1) if ch == 0 else (i - 1, j) if ch == 1 else (i, j - 1)
    return np.array(pi[::-1], np.int32), np.array(pj[::-1], np.int32), int(D[N - 1, M - 1])


# ---------------------------------------------------------------------------------------------------- the device calls
def _device_table(files):
    files = np.ascontiguousarray(files, FILE_DTYPE)
    return files, note_arrays.to_device(files.view(np.uint8).copy()) if len(files) else None


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def logmel_chroma(logmel, files, bins, *, pool: int = DEFAULT_POOL, range: float = DEFAULT_RANGE,
                  floor: float = DEFAULT_FLOOR, d_files=None, n_rows=None):
    """mt3_op_logmel_chroma.  logmel: a contiguous CUDA float32 tensor whose storage holds the job's [rows, mel] rows
    from its first element on (the last dimension is mel); n_rows: the job's rows when the tensor is only the first of
    several blocks that lie back to back in memory (default: the tensor's own rows); files: FILE_DTYPE records; bins: int8
    [mel] (numpy or CUDA).  -> CUDA uint8 [total_a, 12], total_a = the end of the last file's features; features between
    two files' ranges are zero."""
    import torch
    if not (hasattr(logmel, "is_cuda") and logmel.is_cuda and logmel.dtype == torch.float32 and logmel.is_contiguous()
            and logmel.dim() >= 2):
        raise ValueError("the log-mel must be a contiguous CUDA float32 tensor [..., mel]")
    n_mel = int(logmel.shape[-1])
    files, dev = (np.ascontiguousarray(files, FILE_DTYPE), d_files) if d_files is not None else _device_table(files)
    bins_dev = bins if hasattr(bins, "is_cuda") else note_arrays.to_device(np.ascontiguousarray(bins, np.int8))
    if bins_dev.numel() != n_mel:
        raise ValueError("bins has %d entries for a log-mel of %d bins" % (bins_dev.numel(), n_mel))
    total = int(max([int(f["a0"]) + int(f["n"]) for f in files], default=0))
    out = torch.zeros((total, CLASSES), device="cuda", dtype=torch.uint8)
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_logmel_chroma(
        _ptr(logmel), logmel.numel() // n_mel if n_rows is None else int(n_rows), n_mel, files.ctypes.data if len(files) else None, _ptr(dev), len(files),
        _ptr(bins_dev), int(pool), float(range), float(floor), _ptr(out), total, stream.cuda_stream))
    for t in (logmel, dev, bins_dev):
        if t is not None:
            t.record_stream(stream)
    return out


def note_chroma(notes, files, weights=DEFAULT_WEIGHTS, *, d_files=None):
    """mt3_op_note_chroma.  notes: (j0, j1, pitch) as CUDA int32 tensors, or numpy arrays (uploaded); files: FILE_DTYPE
    records.  -> CUDA uint8 [total_s, 12]."""
    import torch
    cols = [c if hasattr(c, "is_cuda") else note_arrays.to_device(np.ascontiguousarray(c, np.int32)) for c in notes]
    if any(c.dtype != torch.int32 or not c.is_contiguous() or c.numel() != cols[0].numel() for c in cols):
        raise ValueError("j0, j1 and pitch must be contiguous int32 columns of one length")
    files, dev = (np.ascontiguousarray(files, FILE_DTYPE), d_files) if d_files is not None else _device_table(files)
    w = np.ascontiguousarray(weights, np.int32).reshape(-1)
    total = int(max([int(f["s0"]) + int(f["m"]) for f in files], default=0))
    out = torch.zeros((total, CLASSES), device="cuda", dtype=torch.uint8)
    scratch = torch.empty(max(total * CLASSES, 1), device="cuda", dtype=torch.int32)
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_note_chroma(
        _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), cols[0].numel(), files.ctypes.data if len(files) else None, _ptr(dev),
        len(files), w.ctypes.data, len(w), scratch.data_ptr(), _ptr(out), total, stream.cuda_stream))
    for t in cols + [dev, scratch]:
        if t is not None:
            t.record_stream(stream)
    return out


def paths(a, s, files, *, d_files=None):
    """mt3_op_sync_paths.  a, s: CUDA uint8 [total, 12]; files: FILE_DTYPE records (a0, n, s0, m, path0, work0).
    -> (path_i, path_j int32 [total_path], path_len int32 [n_files], total int32 [n_files]), CUDA tensors: file f's path
    lies in path0 .. path0 + path_len - 1; the rest of its slots is unspecified."""
    import torch
    for t in (a, s):
        if not (hasattr(t, "is_cuda") and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 2
                and t.shape[1] == CLASSES):
            raise ValueError("features must be contiguous CUDA uint8 tensors [frames, 12]")
    files, dev = (np.ascontiguousarray(files, FILE_DTYPE), d_files) if d_files is not None else _device_table(files)
    for f in files:
        if int(f["n"]) > MAX_FRAMES or int(f["m"]) > MAX_FRAMES:
            raise ValueError("a file has more than %d feature frames" % MAX_FRAMES)
        if int(f["n"]) * int(f["m"]) > MAX_CELLS:
            raise ValueError("a file of %d x %d feature frames exceeds %d cells: there is no band constraint; use a larger "
                             "pool" % (int(f["n"]), int(f["m"]), MAX_CELLS))
    total_path = int(max([int(f["path0"]) + path_capacity(f["n"], f["m"]) for f in files], default=0))
    words = int(max([int(f["work0"]) + workspace_words(f["n"], f["m"]) for f in files], default=0))
    path = torch.empty((2, max(total_path, 1)), device="cuda", dtype=torch.int32)
    counts = torch.zeros((2, max(len(files), 1)), device="cuda", dtype=torch.int32)
    work = torch.empty(max(words, 1), device="cuda", dtype=torch.int32)
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_sync_paths(
        _ptr(a), a.shape[0], _ptr(s), s.shape[0], files.ctypes.data if len(files) else None, _ptr(dev), len(files),
        work.data_ptr(), words * 4, path[0].data_ptr(), path[1].data_ptr(), total_path, counts[0].data_ptr(),
        counts[1].data_ptr(), stream.cuda_stream))
    for t in (a, s, dev, work):
        if t is not None:
            t.record_stream(stream)
    return path[0, :total_path], path[1, :total_path], counts[0, :len(files)], counts[1, :len(files)]


# ------------------------------------------------------------------------------------------------------------ warping
def anchors(path_i, path_j, fps: float):
    """(score seconds, audio seconds) float64 [M]: score frame j's anchor is ((j + 0.5) / fps, (lo_j + hi_j + 1) /
    (2 fps)) with lo_j .. hi_j the audio frames the path pairs with j (a monotone path pairs every j with a run)"""
    pi, pj = np.asarray(path_i, np.int64), np.asarray(path_j, np.int64)
    if len(pi) != len(pj) or len(pi) == 0:
        raise ValueError("a path holds as many i as j, at least one")
    if (np.diff(pi) < 0).any() or (np.diff(pj) < 0).any() or (np.diff(pj) > 1).any() or pj[0] != 0:
        raise ValueError("the path must be monotone and visit every score frame from 0 on")
    first = np.flatnonzero(np.concatenate([[True], np.diff(pj) > 0]))
    last = np.concatenate([first[1:] - 1, [len(pj) - 1]])
    lo, hi = pi[first].astype(np.float64), pi[last].astype(np.float64)
    j = pj[first].astype(np.float64)
    return (j + 0.5) / float(fps), (lo + hi + 1.0) / (2.0 * float(fps))


def warp_times(times, path_i, path_j, fps: float) -> np.ndarray:
    """score times -> audio times (float64) along a path: np.interp over `anchors`, extended with slope 1 before the
    first anchor and after the last.  The path is monotone, so the map never decreases."""
    x, y = anchors(path_i, path_j, fps)
    t = np.asarray(times, np.float64)
    out = np.interp(t, x, y)
    out = np.where(t < x[0], y[0] + (t - x[0]), out)
    return np.where(t > x[-1], y[-1] + (t - x[-1]), out)


def warp_notes(ns, path_i, path_j, fps: float):
    """The notes of `ns` moved from score time to audio time: a new NoteSequence.  Every note time, start and end alike,
    and every control change's time go through `warp_times` (cut at 0); every other field is kept."""
    if len(path_i) == 0:
        return dataclasses.replace(ns, notes=list(ns.notes), control_changes=list(ns.control_changes))
    start = np.maximum(warp_times([n.start_time for n in ns.notes], path_i, path_j, fps), 0.0)
    end = np.maximum(warp_times([n.end_time for n in ns.notes], path_i, path_j, fps), 0.0)
    cc = np.maximum(warp_times([c.time for c in ns.control_changes], path_i, path_j, fps), 0.0)
    notes = [dataclasses.replace(n, start_time=float(a), end_time=float(b)) for n, a, b in zip(ns.notes, start, end)]
    changes = [dataclasses.replace(c, time=float(t)) for c, t in zip(ns.control_changes, cc)]
    return dataclasses.replace(ns, notes=notes, control_changes=changes,
                               total_time=float(end.max()) if len(end) else ns.total_time)


# ---------------------------------------------------------------------------------------------------------- the job
@dataclasses.dataclass
class Packed:
    """the host side of one job"""
    notes: np.ndarray                   # uint8: the NOTE_LAYOUT columns back to back, each file's pitched notes in its order
    n_notes: int
    files: np.ndarray                   # FILE_DTYPE [n_files]


def pack(sequences, n_frames, rows_per_file, pool: int, fps: float) -> Packed:
    """every check on the notes, and the job's columns: per file its pitched notes (drums carry no chroma) as frames"""
    cols, counts, ms = [[] for _ in NOTE_LAYOUT], [], []
    for f, ns in enumerate(sequences):
        prefix = "file %d: " % f
        start, end, pitch, _, drum = note_arrays.fields(ns)
        note_arrays.check_times(start, end, prefix=prefix)
        note_arrays.check_range(prefix + "pitches are 0 .. 127", pitch)
        keep = drum == 0
        j0, j1 = note_frames(start[keep], end[keep], fps)
        if (j0 < 0).any():
            raise ValueError(prefix + "note times must not be negative")
        for col, a in zip(cols, (j0, j1, pitch[keep])):
            col.append(a)
        counts.append(int(keep.sum()))
        ms.append(int(j1.max()) if len(j1) else 0)
    table = file_table(n_frames, counts, ms, pool, rows_per_file)
    return Packed(note_arrays.pack(cols, NOTE_LAYOUT), int(sum(counts)), table)


def synchronize(logmels, sequences, *, pool: int = DEFAULT_POOL, harmonic_weights=DEFAULT_WEIGHTS,
                range: float = DEFAULT_RANGE, floor: float = DEFAULT_FLOOR, fmin: float = DEFAULT_FMIN,
                fmax: float = DEFAULT_FMAX, bins=None, frames_per_second: float = LOGMEL_FPS) -> List[dict]:
    """Every (recording, score) pair of a job synchronised on the device.  logmels: per file a CUDA float32
    [segments, T, mel] tensor, or the pair (tensor, n_frames) with the file's valid frame count (`velocity.estimate`'s
    form); sequences: one NoteSequence per file, in SCORE time.  pool: log-mel rows per feature frame (1 .. 16; both
    features then run at frames_per_second / pool frames per second); harmonic_weights: 1 .. 6 integers 0 .. 255, the
    weight of a note's harmonics 1 .. 6 in the score's chroma; range, floor: the audio feature's quantisation;
    fmin, fmax (or `bins`, an int8 [mel] table): `chroma_bins` of spectrograms.mel_matrix().
    -> one dict per file:
      'notes'        the NoteSequence in audio time (`warp_notes`)
      'path'         (audio seconds, score seconds): float64 arrays, the centres of the path's cells
      'path_frames'  (path_i, path_j): int32 arrays, for `warp_times`
      'fps'          feature frames per second
      'total', 'mean_cost'   D[n-1][m-1] and total / len(path)
      'tempo_ratio'  the path's overall slope: audio seconds per score second between the first and the last score
                     frame's anchors (> 1: played slower than written); 1.0 for fewer than two score frames
    A file without pitched notes or without frames has an empty path and keeps its notes.  One pack, one upload, the
    three op calls, one copy back.  ValueError before anything is uploaded: see `velocity.estimate` for the log-mels;
    pool outside 1 .. 16; a note time that is not finite or negative; a pitch outside 0 .. 127; a file with more than
    2^18 feature frames on a side or more than 2^31 cells (there is no band constraint: use a larger pool)."""
    import torch
    sequences, logmels = list(sequences), list(logmels)
    if len(logmels) != len(sequences):
        raise ValueError("logmels has %d entries for %d sequences" % (len(logmels), len(sequences)))
    if not (isinstance(pool, (int, np.integer)) and 1 <= pool <= MAX_POOL):
        raise ValueError("pool must be 1 .. %d log-mel rows, got %r" % (MAX_POOL, pool))
    if not (math.isfinite(frames_per_second) and frames_per_second > 0):
        raise ValueError("frames_per_second must be a finite number > 0, got %r" % (frames_per_second,))
    if not (math.isfinite(range) and range > 0) or math.isnan(floor):
        raise ValueError("range must be a finite number > 0 and floor a number, got %r, %r" % (range, floor))
    weights = np.asarray(harmonic_weights).reshape(-1)
    if not (1 <= len(weights) <= len(OFFSETS)) or (weights != np.floor(weights)).any() or (weights < 0).any() or \
            (weights > 255).any():
        raise ValueError("harmonic_weights must be 1 .. 6 integers 0 .. 255, got %r" % (harmonic_weights,))
    if not sequences:
        return []
    tensors, n_frames = [], []
    for f, entry in enumerate(logmels):
        t, n = entry if isinstance(entry, (tuple, list)) else (entry, None)
        if not (hasattr(t, "is_cuda") and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()):
            raise ValueError("file %d: the log-mel must be a contiguous CUDA float32 [segments, T, mel] tensor" % f)
        if not 1 <= t.shape[2] <= 4096 or (tensors and t.shape[2] != tensors[0].shape[2]):
            raise ValueError("file %d: mel must be 1 .. 4096 and the same for every file, got %d" % (f, t.shape[2]))
        rows = t.shape[0] * t.shape[1]
        n = rows if n is None else int(n)
        if not 0 <= n <= rows:
            raise ValueError("file %d: n_frames must be 0 .. %d (segments * T), got %d" % (f, rows, n))
        tensors.append(t)
        n_frames.append(n)
    n_mel = int(tensors[0].shape[2])
    fps = float(frames_per_second) / int(pool)
    if bins is None:
        from . import spectrograms
        bins = chroma_bins(spectrograms.mel_matrix(spectrograms.SpectrogramConfig(num_mel_bins=n_mel)), fmin, fmax)
    bins = np.ascontiguousarray(bins, np.int8)
    if bins.shape != (n_mel,):
        raise ValueError("bins must be int8 [%d], got %r" % (n_mel, bins.shape))
    packed = pack(sequences, n_frames, [t.shape[0] * t.shape[1] for t in tensors], int(pool), fps)
    files = packed.files
    for f, rec in enumerate(files):
        if int(rec["n"]) > MAX_FRAMES or int(rec["m"]) > MAX_FRAMES or int(rec["n"]) * int(rec["m"]) > MAX_CELLS:
            raise ValueError("file %d: %d x %d feature frames exceed the limits (%d a side, %d cells; there is no band "
                             "constraint): use a larger pool" % (f, int(rec["n"]), int(rec["m"]), MAX_FRAMES, MAX_CELLS))
    # the one upload: the file table | j0, j1, pitch i32 [n] each | bins i8 [mel]
    head = files.view(np.uint8)
    data = note_arrays.to_device(np.concatenate([head, packed.notes, bins.view(np.uint8)]))
    n = packed.n_notes
    table_dev = data[: len(head)]
    cols = [data[len(head) + at: len(head) + at + 4 * n].view(torch.int32) for at in note_arrays.column_offsets([4, 4, 4], n)]
    bins_dev = data[len(head) + 12 * n:].view(torch.int8)
    # (slices of one tensor lie back to back and come as its first slice: the rows are the job's, not that slice's)
    a = logmel_chroma(note_arrays.one_buffer(tensors), files, bins_dev, pool=int(pool), range=range, floor=floor,
                      d_files=table_dev, n_rows=sum(t.shape[0] * t.shape[1] for t in tensors))
    s = note_chroma(cols, files, weights, d_files=table_dev)
    path_i, path_j, path_len, total = paths(a, s, files, d_files=table_dev)
    host = torch.cat([path_i, path_j, path_len, total]).cpu().numpy()                # the one copy back
    P = len(path_i)
    path_i, path_j, path_len, total = host[:P], host[P: 2 * P], host[2 * P: 2 * P + len(files)], host[2 * P + len(files):]
    out = []
    for ns, rec, length, tot in zip(sequences, files, path_len, total):
        at = int(rec["path0"])
        pi, pj = path_i[at: at + int(length)].copy(), path_j[at: at + int(length)].copy()
        out.append(record(ns, pi, pj, int(tot), fps))
    return out


def record(ns, path_i, path_j, total: int, fps: float) -> dict:
    """one file's result of `synchronize` from its path"""
    ratio = 1.0
    if len(path_i):
        x, y = anchors(path_i, path_j, fps)
        if len(x) > 1:
            ratio = float((y[-1] - y[0]) / (x[-1] - x[0]))
    return {"notes": warp_notes(ns, path_i, path_j, fps),
            "path": ((np.asarray(path_i, np.float64) + 0.5) / fps, (np.asarray(path_j, np.float64) + 0.5) / fps),
            "path_frames": (path_i, path_j), "fps": fps, "total": int(total),
            "mean_cost": float(total) / len(path_i) if len(path_i) else 0.0, "tempo_ratio": ratio}
