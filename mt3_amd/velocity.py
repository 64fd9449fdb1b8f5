"""Note velocities from the log-mel the engine already holds (mt3_op_note_levels, mt3_op_level_velocities; the rule:
include/mt3_hip.h, "note velocities", derived in DESIGN 6q).

  harmonic_bins(mel_matrix)            the host-built table: per pitch the mel bins of its first harmonics, one drum row
  levels_reference / velocities_reference    the rule, stated once in numpy: the yardstick, bit for bit
  estimate(logmels, sequences)         every file of a job on the device: one pack, one upload, the two op calls and one
                                       copy back

Nothing is measured from the samples.  A note's LEVEL is the largest, over the `window` frames from its onset, of the mean
log-mel value at its pitch's harmonic bins; a file's pitched notes and its drum notes are each ranked on their own, the
member at the `quantile` rank is the group's ANCHOR, and a note's velocity follows from its level minus the anchor through
a table of 126 thresholds: log-mel is the natural log of a magnitude, so a difference d is an amplitude ratio e^d, and with
amplitude ~ (v / 127)^gamma the note is as loud as velocity anchor_velocity * e^(d / gamma).  gamma = 2 (the usual
40 log10 convention) and anchor_velocity = 80 are design choices, not measurements; gamma = 1 is this project's `render`
(gain = v / 127).  The dynamics are relative to the file's own anchor, not absolute.  Every step on the device is a gather,
a float64 add in table order, one float64 division by the count, a max, a rank selection or a comparison with the table:
the device equals the two reference functions bit for bit.  There is no host fallback: `estimate` needs the library and a
device.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List

import numpy as np

from . import _lib, note_arrays

DRUM_KEY = 128                                        # the key of a drum note: the table's last row
N_KEYS = 129
N_THRESHOLDS = 126                                    # th[v], v = 2 .. 127
MAX_WINDOW, MAX_MEL = _lib.VELOCITY_MAX_WINDOW, _lib.VELOCITY_MAX_MEL
NOTE_LAYOUT = ("<i4", "<i4", "<i4")                   # frame | key | velocity_in: what pack lays out, sorted
FILE_DTYPE = np.dtype([("first", "<i8"), ("row0", "<i8"), ("n_notes", "<i4"), ("n_pitched", "<i4"), ("n_frames", "<i4"),
                       ("reserved", "<i4")])                                                   # mt3_velocity_file


def harmonic_bins(mel_matrix, harmonics: int = 6, sample_rate: int = 16000, fft_size: int = 2048):
    """(bin_first int32 [130], bins int32): row p (0 .. 127) lists, for h = 1 .. harmonics in order, the mel bin of largest
    weight (the lowest on a tie) in row k = floor(h * f0(p) * fft_size / sample_rate + 0.5) of the [fft_size / 2 + 1, mel]
    matrix, f0(p) = 440 * 2^((p - 69) / 12) in float64; a harmonic with k > fft_size / 2 or an all-zero row k is dropped;
    consecutive duplicates stay (they are a weighting).  Row 128, the drums: mel bins 0, 8, 16, ..."""
    w = np.asarray(mel_matrix)
    if w.ndim != 2 or w.shape[0] != fft_size // 2 + 1:
        raise ValueError("mel_matrix must be [fft_size / 2 + 1, mel], got %r" % (w.shape,))
    if int(harmonics) < 1:
        raise ValueError("harmonics must be at least 1, got %r" % (harmonics,))
    rows = []
    for p in range(128):
        row = []
        for h in range(1, int(harmonics) + 1):
            f = h * 440.0 * 2.0 ** ((p - 69) / 12.0)
            k = int(math.floor(f * fft_size / sample_rate + 0.5))
            if k > fft_size // 2 or not w[k].any():
                continue
            row.append(int(np.argmax(w[k])))                            # the first of equal maxima
        rows.append(row)
    rows.append(list(range(0, w.shape[1], 8)))
    first = note_arrays.offsets([len(r) for r in rows])
    return first.astype(np.int32), np.array([b for r in rows for b in r], np.int32)


def thresholds(gamma: float = 2.0, anchor_velocity: float = 80) -> np.ndarray:
    """float64 [126]: th[v] = gamma * ln((v - 0.5) / anchor_velocity) for v = 2 .. 127 -- a note whose level lies d above
    the anchor has velocity 1 + #{v : d >= th[v]}"""
    if not (math.isfinite(gamma) and gamma > 0):
        raise ValueError("gamma must be a finite number > 0, got %r" % (gamma,))
    if not (math.isfinite(anchor_velocity) and anchor_velocity > 0):
        raise ValueError("anchor_velocity must be a finite number > 0, got %r" % (anchor_velocity,))
    return float(gamma) * np.log((np.arange(2, 128, dtype=np.float64) - 0.5) / float(anchor_velocity))


def frames_of(onsets, frames_per_second: float) -> np.ndarray:
    """int32: floor(onset * frames_per_second) in float64; what does not fit is -1 or 2^31 - 1, outside every file"""
    return np.clip(np.floor(np.asarray(onsets, np.float64) * float(frames_per_second)), -1, 2 ** 31 - 1).astype(np.int32)


def levels_reference(logmel, files, frame, key, bin_first, bins, window: int = 8) -> np.ndarray:
    """THE RULE, part 1.  logmel: float32 [rows, mel]; files: FILE_DTYPE records (file f owns rows row0 .. row0 + n_frames
    - 1 and notes first .. first + n_notes - 1); frame, key: int32 per note.  -> float64 [notes]: per note the np.fmax over
    the frames frame .. frame + window - 1 cut to [0, n_frames) of s(g) = (the float64 sum of the row's values at the
    key's bins, added left to right in table order) / their count; NaN (unmeasured) for a frame outside [0, n_frames), an
    empty bin row, or a window whose every s is NaN."""
    logmel = np.asarray(logmel, np.float32)
    level = np.full(len(frame), np.nan, np.float64)
    for f in files:
        row0, n_frames = int(f["row0"]), int(f["n_frames"])
        for i in range(int(f["first"]), int(f["first"]) + int(f["n_notes"])):
            at, k = int(frame[i]), int(key[i])
            row = bins[bin_first[k]: bin_first[k + 1]] if 0 <= k < N_KEYS else bins[:0]
            if not 0 <= at < n_frames or len(row) == 0:
                continue
            for g in range(max(at, 0), min(at + int(window), n_frames)):
                s = np.float64(0.0)
                with np.errstate(invalid="ignore"):                     # inf - inf: a NaN frame, skipped
                    for b in row:
                        s = s + np.float64(logmel[row0 + g, b])
                level[i] = np.fmax(level[i], s / np.float64(len(row)))
    return level


def velocities_reference(level, velocity_in, files, th, quantile: float = 0.5):
    """THE RULE, part 2.  level: float64 per note, NaN = unmeasured; files: FILE_DTYPE records whose notes are the
    n_pitched pitched ones, then the drums: two groups per file.  -> (velocity int32 [notes], anchor float64 [files, 2],
    measured int32 [files, 2]): a group's anchor is its measured member at ascending rank floor(quantile * (n - 1)) (NaN
    for n = 0); d = level - anchor; velocity = 1 + #{v : d >= th[v]}; an unmeasured note keeps velocity_in."""
    level, th = np.asarray(level, np.float64), np.asarray(th, np.float64)
    velocity = np.array(velocity_in, np.int32)
    anchor = np.full((len(files), 2), np.nan, np.float64)
    measured = np.zeros((len(files), 2), np.int32)
    for f, rec in enumerate(files):
        a, m, b = int(rec["first"]), int(rec["first"]) + int(rec["n_pitched"]), int(rec["first"]) + int(rec["n_notes"])
        for g, (lo, hi) in enumerate(((a, m), (m, b))):
            ok = ~np.isnan(level[lo:hi])
            n = int(ok.sum())
            measured[f, g] = n
            if n == 0:
                continue
            anchor[f, g] = np.sort(level[lo:hi][ok])[int(np.floor(np.float64(quantile) * np.float64(n - 1)))]
            with np.errstate(invalid="ignore"):                         # inf - inf: d is NaN, no threshold is reached
                d = level[lo:hi][ok] - anchor[f, g]
                velocity[lo:hi][ok] = 1 + (d[:, None] >= th[None, :]).sum(1)
    return velocity, anchor, measured


@dataclasses.dataclass
class Packed:
    """the host side of one job"""
    notes: np.ndarray                   # uint8: the NOTE_LAYOUT columns back to back, each file's pitched notes then its drums
    n_notes: int
    files: np.ndarray                   # FILE_DTYPE [n_files]
    n_rows: int                         # log-mel rows of the job: the files' blocks back to back
    src: List[np.ndarray]               # per file: the position in the caller's `ns.notes` of each packed note


def pack(sequences, n_frames, rows_per_file, frames_per_second: float) -> Packed:
    """every check of `estimate` on the notes, and the job's columns: per file the pitched notes, then the drums, each in
    the caller's order; file f's rows start where file f - 1's rows_per_file end"""
    cols, src = [[] for _ in NOTE_LAYOUT], []
    table = np.zeros(len(sequences), FILE_DTYPE)
    for f, ns in enumerate(sequences):
        prefix = "file %d: " % f
        start, _, pitch, velocity, drum = note_arrays.fields(ns)
        note_arrays.check_times(start, prefix=prefix)
        note_arrays.check_range(prefix + "pitches are 0 .. 127", pitch)
        if ((velocity < -2 ** 31) | (velocity >= 2 ** 31)).any():
            raise ValueError(prefix + "velocities must fit int32")
        by = np.argsort(drum != 0, kind="stable")
        for col, a in zip(cols, (frames_of(start, frames_per_second), np.where(drum != 0, DRUM_KEY, pitch), velocity)):
            col.append(a[by])
        src.append(by)
        table[f] = (0, 0, len(by), int((drum == 0).sum()), n_frames[f], 0)
    table["first"] = note_arrays.offsets(table["n_notes"])[:-1]
    table["row0"] = note_arrays.offsets(rows_per_file)[:-1]
    return Packed(note_arrays.pack(cols, NOTE_LAYOUT), int(table["n_notes"].sum()), table, int(np.sum(rows_per_file)), src)


def _check_table(bin_first, bins, n_mel: int):
    if len(bin_first) != N_KEYS + 1 or bin_first[0] != 0 or (np.diff(bin_first) < 0).any() or bin_first[-1] != len(bins):
        raise ValueError("bin_first must be 130 offsets that rise from 0 to len(bins)")
    if len(bins) and not (0 <= bins.min() and bins.max() < n_mel):
        raise ValueError("a bin of the table is outside the log-mel's 0 .. %d" % (n_mel - 1))


def estimate(logmels, sequences, *, window: int = 8, harmonics: int = 6, gamma: float = 2.0, quantile: float = 0.5,
             anchor_velocity: float = 80, return_levels: bool = False, table=None, frames_per_second: float = 125.0):
    """The notes of every file of a job with velocities estimated from the file's log-mel, on the device.  logmels: per file
    a CUDA float32 [segments, T, mel] tensor (what the frontend writes for the engine), or the pair (tensor, n_frames) with
    the file's valid frame count -- rows past it, a short last segment's zero rows, are never read (default: all of them).
    sequences: one NoteSequence per file.  window: frames from the onset on (1 .. 64); harmonics: per pitch, for the table;
    gamma, anchor_velocity: the thresholds (`thresholds`); quantile: the anchor's rank (0 .. 1).  table: (bin_first, bins)
    instead of `harmonic_bins(spectrograms.mel_matrix(), harmonics)`; frames_per_second: of the log-mel's rows.
    -> one new NoteSequence per file: copies of the notes with the new `velocity`; a note that could not be measured (its
    onset outside the file's frames, no bin for its pitch, nothing but NaN in its window) keeps the one it came with.  With
    return_levels: (sequences, records), one dict per file -- 'levels' float64 aligned with `ns.notes` (NaN: unmeasured),
    'anchors' float64 [2] and 'measured' int [2] (pitched notes, drums).
    One pack, one upload, the two op calls, one copy back.  ValueError, before anything is uploaded: as many logmels as
    sequences; a tensor that is not CUDA float32 [segments, T, mel] and contiguous; mel outside 1 .. 4096; n_frames outside
    0 .. segments * T; window outside 1 .. 64; quantile outside [0, 1]; gamma or anchor_velocity not finite and > 0; a table
    bin >= mel; an onset that is not finite; a pitch outside 0 .. 127."""
    import torch
    sequences, logmels = list(sequences), list(logmels)
    if len(logmels) != len(sequences):
        raise ValueError("logmels has %d entries for %d sequences" % (len(logmels), len(sequences)))
    if not (isinstance(window, (int, np.integer)) and 1 <= window <= MAX_WINDOW):
        raise ValueError("window must be 1 .. %d frames, got %r" % (MAX_WINDOW, window))
    if not 0.0 <= quantile <= 1.0:                                      # NaN fails too
        raise ValueError("quantile must lie in [0, 1], got %r" % (quantile,))
    if not (math.isfinite(frames_per_second) and frames_per_second > 0):
        raise ValueError("frames_per_second must be a finite number > 0, got %r" % (frames_per_second,))
    th = thresholds(gamma, anchor_velocity)
    if not sequences:
        return ([], []) if return_levels else []
    tensors, n_frames = [], []
    for f, entry in enumerate(logmels):
        t, n = entry if isinstance(entry, (tuple, list)) else (entry, None)
        if not (hasattr(t, "is_cuda") and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()):
            raise ValueError("file %d: the log-mel must be a contiguous CUDA float32 [segments, T, mel] tensor" % f)
        if not 1 <= t.shape[2] <= MAX_MEL or (tensors and t.shape[2] != tensors[0].shape[2]):
            raise ValueError("file %d: mel must be 1 .. %d and the same for every file, got %d" % (f, MAX_MEL, t.shape[2]))
        rows = t.shape[0] * t.shape[1]
        n = rows if n is None else int(n)
        if not 0 <= n <= rows:
            raise ValueError("file %d: n_frames must be 0 .. %d (segments * T), got %d" % (f, rows, n))
        tensors.append(t)
        n_frames.append(n)
    n_mel = int(tensors[0].shape[2])
    if table is None:
        from . import spectrograms
        table = harmonic_bins(spectrograms.mel_matrix(spectrograms.SpectrogramConfig(num_mel_bins=n_mel)), harmonics)
    bin_first, bins = (np.ascontiguousarray(a, np.int32) for a in table)
    _check_table(bin_first, bins, n_mel)
    packed = pack(sequences, n_frames, [t.shape[0] * t.shape[1] for t in tensors], frames_per_second)
    level, velocity, anchor, measured = run(packed, note_arrays.one_buffer(tensors), n_mel, bin_first, bins, th, int(window),
                                            float(quantile))
    out, records = [], []
    for f, (ns, rec, src) in enumerate(zip(sequences, packed.files, packed.src)):
        a, b = int(rec["first"]), int(rec["first"]) + int(rec["n_notes"])
        new = np.zeros(len(src), np.int64)
        new[src] = velocity[a:b]
        out.append(dataclasses.replace(ns, notes=[dataclasses.replace(note, velocity=int(v))
                                                  for note, v in zip(ns.notes, new)]))
        levels = np.full(len(src), np.nan, np.float64)
        levels[src] = level[a:b]
        records.append({"levels": levels, "anchors": anchor[f].copy(), "measured": measured[f].astype(np.int64)})
    return (out, records) if return_levels else out


def run(packed: Packed, logmel, n_mel: int, bin_first, bins, th, window: int, quantile: float):
    """one upload, the two op calls, one copy back -> (level f64 [n], velocity i32 [n], anchor f64 [files, 2], measured i32
    [files, 2]), the notes in the packed order.  logmel: the CUDA tensor whose storage holds every file's rows from its
    first element on."""
    import torch
    n, n_files = packed.n_notes, len(packed.files)
    # the one upload: th f64 [126] | frame, key, velocity_in i32 [n] each | bin_first i32 [130] | bins i32
    head = np.ascontiguousarray(th, "<f8").view(np.uint8)
    data = note_arrays.to_device(np.concatenate([head, packed.notes, bin_first.view(np.uint8), bins.view(np.uint8)]))
    base = data.data_ptr()
    frame_at, key_at, vel_at = (len(head) + a for a in note_arrays.column_offsets([4, 4, 4], n))
    first_at = len(head) + len(packed.notes)
    # the one output: level f64 [n] | anchor f64 [files * 2] | velocity i32 [n] | measured i32 [files * 2]
    anchor_at, out_vel_at, measured_at = 8 * n, 8 * (n + 2 * n_files), 12 * n + 16 * n_files
    out = torch.empty(measured_at + 8 * n_files, device="cuda", dtype=torch.uint8)
    stream = torch.cuda.current_stream()
    lib = _lib.load()
    _lib.check(lib.mt3_op_note_levels(
        logmel.data_ptr(), packed.n_rows, n_mel, packed.files.ctypes.data, n_files, base + frame_at, base + key_at, n,
        bin_first.ctypes.data, bins.ctypes.data, base + first_at, base + first_at + 4 * len(bin_first), len(bins), window,
        out.data_ptr(), stream.cuda_stream))
    _lib.check(lib.mt3_op_level_velocities(
        out.data_ptr(), n, packed.files.ctypes.data, n_files, quantile, base, base + vel_at, out.data_ptr() + out_vel_at,
        out.data_ptr() + anchor_at, out.data_ptr() + measured_at, stream.cuda_stream))
    logmel.record_stream(stream)
    host = out.cpu().numpy()                                            # the one copy back
    return (host[:anchor_at].view("<f8"), host[out_vel_at: measured_at].view("<i4"),
            host[anchor_at: out_vel_at].view("<f8").reshape(n_files, 2), host[measured_at:].view("<i4").reshape(n_files, 2))
