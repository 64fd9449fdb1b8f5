"""Beat tracking and tempo maps: the beats of a transcription from its own onsets, and its notes on the beats' grid.

  track(sequences, ...)              the beats of every file of a job on the device (mt3_op_track_beats): one upload, one op
                                     call, one copy back
  track_reference(sequences, ...)    THE RULE in numpy: the yardstick of the kernel, bit for bit
  snap(sequences, beats, ...)        the notes moved onto the grid of `subdivisions` steps per beat (mt3_op_snap_notes)
  snap_reference(sequences, ...)     the snapping rule in numpy, bit for bit

`midi_io.note_sequence_to_midi_bytes(ns, beats=b.times)` writes the tempo map: every beat one quarter note.

THE RULE is the dynamic-programming beat tracker of Ellis (2007, "Beat tracking by dynamic programming") restated in
integers, so that any summation order and integer atomics give the same bits.  Per file, fps = 100 (the codec's
steps_per_second):

 1. ONSET FRAMES (host, float64)  f = int(floor(start_time * fps + 0.5)), one int32 per note, drums like any other note.
    F = max(f) + 1 frames; no notes: F = 0, no beats, period 0.  F < 2^20 (2.9 hours): ValueError.
 2. ENVELOPE  n[t] = the onsets in frame t, at most 255.  E[t] = n[t-1] + 2 n[t] + n[t+1] for t in 0 .. F-1, zeros outside
    the file.  peak = max E;  S[t] = (E[t] << 16) // peak.
 3. PERIOD  for l in LAG_MIN .. LAG_MAX (25 .. 200 frames = 240 .. 30 bpm): A[l] = sum over t of E[t] * E[t + l] (int64;
    E <= 1020 and F < 2^20, so A < 2^40 and A * W < 2^57).  W[l] = round(2^16 * exp(-0.5 * (log2(l / l0) / width)^2)),
    l0 = 60 * fps / prior_bpm: a log-normal tempo prior (`prior_table`).  p = the LOWEST l of maximal A[l] * W[l]; when every
    product is 0 the period is 0 and there are no beats.  (E reaches one frame to either side of an onset, so two onsets
    d frames apart give products at lags d - 2 .. d + 2.)
 4. PATH  lo = (p + 1) // 2, hi = 2 p;  pen[l] = round(tightness * 2^16 * ln(l / p)^2) for l in lo .. hi (`penalty_table`):
        best(t) = max over l in lo .. hi with t - l >= 0 of (C[t - l] - pen[l])       the LOWEST l on equal values
        C[t] = S[t] + max(best(t), 0);   back[t] = that l, or 0 when best(t) <= 0 or no l is admissible
 5. BEATS  the path ends at the LOWEST t of maximal C[t] among the last p frames (all frames when F <= p) and is read back
    through `back` until back[t] == 0; the beats are those frames, ascending.  score = C[end].  At most F // 13 + 2 beats.

prior_bpm (120), the prior's width (one octave), the [1, 2, 1] smoothing and the tightness are DESIGN CHOICES, not
measurements: they were set on synthetic metrical input (DESIGN.md section 6r holds the procedure and the numbers).
Measure them on your music.  Limits: one period per file; half / double tempo is the prior's choice; every beat is a quarter
note (downbeats and the time signature: `mt3_amd.harmony`); no triplets beyond `subdivisions`.

SNAPPING (float64, every operation rounded once, no fused multiply-add).  A file's beat times b = frame / fps; with fewer
than 2 beats its notes stay.  For a time t: i = the last beat at or before t, kept within 0 .. n - 2 (so before the first
and after the last beat the grid of the first / last interval continues); d = b[i+1] - b[i];
u = ((t - b[i]) / d) * subdivisions;  k = ceil(u - 0.5) (the nearest step, the lower one on a tie);
point(i, k) = b[i+1] when k == subdivisions, else b[i] + (k / subdivisions) * d.  start' = point(i, k) of the start,
end' = that of the end; when end' <= start', end' = point(i, k + 1) of the START: the note keeps one grid step.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List, Sequence

import numpy as np

from . import _lib, note_arrays, note_sequences

FPS = _lib.BEATS_FPS
LAG_MIN, LAG_MAX = _lib.BEATS_LAG_MIN, _lib.BEATS_LAG_MAX
N_LAGS = LAG_MAX - LAG_MIN + 1
LAG_MIN_HALF = (LAG_MIN + 1) // 2                       # 13: the shortest step of a path
PEN_STRIDE = _lib.BEATS_PEN_STRIDE                       # 301 = hi - lo + 1 of the longest period
MAX_FRAMES = _lib.BEATS_MAX_FRAMES                       # F < 2^20
MAX_SUBDIVISIONS = _lib.BEATS_MAX_SUBDIVISIONS
DEFAULT_PRIOR_BPM = 120.0
DEFAULT_WIDTH = 1.0                                      # octaves
# the middle of the range (20 .. 184) over which the numpy rule finds every beat of all 8 jittered files of
# tests/test_beats_ref.py (F-measure 1.0 at 70 ms); DESIGN.md section 6r.  Ellis's 100 is for an envelope in standard
# deviations; this one is for S, where 2^16 is the envelope's peak
DEFAULT_TIGHTNESS = 102.0
MAX_TIGHTNESS = float(1 << 20)                           # pen < 2^36: C - pen stays far inside int64
FILE_DTYPE = np.dtype([("first", "<i8"), ("frame0", "<i8"), ("beat0", "<i8"), ("n_notes", "<i4"), ("n_frames", "<i4")])
SNAP_FILE_DTYPE = np.dtype([("first", "<i8"), ("beat0", "<i8"), ("n_notes", "<i4"), ("n_beats", "<i4")])


@dataclasses.dataclass
class Beats:
    """One file's beats.  times: float64 seconds (frame / fps), ascending; frames: the same as int32 frames; period: frames
    per beat of the file's one tempo (0: none found); qpm: 60 * fps / period (0.0 without a period); score: C at the path's
    end."""
    times: np.ndarray
    frames: np.ndarray
    period: int
    qpm: float
    score: int


@dataclasses.dataclass
class Packed:
    """the host side of one mt3_op_track_beats call"""
    column: np.ndarray                  # uint8: the onset frames, int32, the files one after the other
    n_notes: int
    files: np.ndarray                   # FILE_DTYPE [n_files]
    total_frames: int
    total_beats: int                    # the sum of the files' capacities

    def frames(self, f: int) -> np.ndarray:
        a = int(self.files["first"][f])
        return self.column.view("<i4")[a: a + int(self.files["n_notes"][f])]


def capacity(n_frames):
    """the beats a file of `n_frames` frames can have at most, plus one: steps of a path are >= 13 frames"""
    return np.asarray(n_frames, np.int64) // LAG_MIN_HALF + 2


@functools.lru_cache(maxsize=8)
def prior_table(prior_bpm: float = DEFAULT_PRIOR_BPM, width: float = DEFAULT_WIDTH) -> np.ndarray:
    """W[l] for l in LAG_MIN .. LAG_MAX, int64 [176]: the tempo prior, built here and nowhere else"""
    prior_bpm, width = float(prior_bpm), float(width)
    if not (np.isfinite(prior_bpm) and prior_bpm > 0):
        raise ValueError("prior_bpm must be a finite number > 0, got %r" % (prior_bpm,))
    if not (np.isfinite(width) and width > 0):
        raise ValueError("width must be a finite number of octaves > 0, got %r" % (width,))
    lags = np.arange(LAG_MIN, LAG_MAX + 1, dtype=np.float64)
    w = np.rint(65536.0 * np.exp(-0.5 * (np.log2(lags / (60.0 * FPS / prior_bpm)) / width) ** 2)).astype(np.int64)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=8)
def penalty_table(tightness: float = DEFAULT_TIGHTNESS) -> np.ndarray:
    """pen of every period, int64 [176, 301]: row p - LAG_MIN holds pen[l] for l = lo .. hi at columns l - lo, zeros after
    them; built here and nowhere else"""
    tightness = float(tightness)
    if not (np.isfinite(tightness) and 0 <= tightness <= MAX_TIGHTNESS):
        raise ValueError("tightness must be 0 .. %g, got %r" % (MAX_TIGHTNESS, tightness))
    pen = np.zeros((N_LAGS, PEN_STRIDE), np.int64)
    for p in range(LAG_MIN, LAG_MAX + 1):
        lags = np.arange((p + 1) // 2, 2 * p + 1, dtype=np.float64)
        pen[p - LAG_MIN, :len(lags)] = np.rint(tightness * 65536.0 * np.log(lags / p) ** 2).astype(np.int64)
    pen.setflags(write=False)
    return pen


def _check_sequences(sequences, who: str, records: bool = True) -> list:
    sequences = list(sequences) if isinstance(sequences, (list, tuple)) else None
    if sequences is None or not all(hasattr(s, "notes") or (records and isinstance(s, np.ndarray) and s.dtype.names)
                                    for s in sequences):
        raise ValueError("%s takes a list of NoteSequences%s" % (who, " (or note record arrays)" if records else ""))
    return sequences


def pack(sequences) -> Packed:
    """every check of `track` and step 1 of the rule: the onset frames of every file as one int32 column"""
    sequences = _check_sequences(sequences, "track")
    cols, files = [], np.zeros(len(sequences), FILE_DTYPE)
    for f, seq in enumerate(sequences):
        start, end = note_arrays.fields(seq)[:2]
        note_arrays.check_times(start, end, not_negative=True, prefix="file %d: " % f)
        frames = np.floor(start * float(FPS) + 0.5).astype(np.int64)
        n_frames = int(frames.max()) + 1 if len(frames) else 0
        if n_frames >= MAX_FRAMES:
            raise ValueError("file %d: %d frames; a file has fewer than %d (%.1f hours)"
                             % (f, n_frames, MAX_FRAMES, MAX_FRAMES / FPS / 3600.0))
        assert n_frames < MAX_FRAMES                                   # so that A * W < 2^63 (step 3 of the rule)
        cols.append(frames)
        files[f] = (0, 0, 0, len(frames), n_frames)
    files["first"] = note_arrays.offsets(files["n_notes"])[:-1]
    files["frame0"] = note_arrays.offsets(files["n_frames"])[:-1]
    files["beat0"] = note_arrays.offsets(capacity(files["n_frames"]))[:-1]
    return Packed(note_arrays.pack([cols], ("<i4",)), int(files["n_notes"].sum()), files, int(files["n_frames"].sum()),
                  int(capacity(files["n_frames"]).sum()) if len(files) else 0)


def envelope(frames: np.ndarray, n_frames: int) -> np.ndarray:
    """step 2: E, int64 [n_frames]"""
    n = np.zeros(n_frames + 2, np.int64)
    n[1:-1] = np.minimum(np.bincount(frames, minlength=n_frames), 255)
    return n[:-2] + 2 * n[1:-1] + n[2:]


def track_frames(frames: np.ndarray, n_frames: int, prior: np.ndarray, penalties: np.ndarray):
    """steps 2 .. 5 of THE RULE for one file -> (period, beat frames int32, score)"""
    F = int(n_frames)
    none = (0, np.zeros(0, np.int32), 0)
    if F == 0:
        return none
    E = envelope(np.asarray(frames, np.int64), F)
    S = (E << 16) // int(E.max())
    A = np.array([int(np.dot(E[:F - l], E[l:])) if l < F else 0 for l in range(LAG_MIN, LAG_MAX + 1)], np.int64)
    product = A * prior
    if int(product.max()) == 0:
        return none
    p = LAG_MIN + int(np.argmax(product))                              # argmax: the first of the maximal ones
    lo, hi = (p + 1) // 2, 2 * p
    lags = np.arange(lo, hi + 1)
    pen = penalties[p - LAG_MIN, :len(lags)]
    C, back = np.zeros(F, np.int64), np.zeros(F, np.int64)
    lowest = np.iinfo(np.int64).min
    for b in range(0, F, lo):                                          # the frames of a block do not depend on each other
        t = np.arange(b, min(b + lo, F))
        at = t[:, None] - lags[None, :]
        through = np.where(at >= 0, C[np.maximum(at, 0)] - pen[None, :], lowest)
        arg = np.argmax(through, axis=1)                               # the first: the lowest l
        best = through[np.arange(len(t)), arg]
        taken = best > 0                                               # (no admissible l: best is `lowest`)
        C[t] = S[t] + np.where(taken, best, 0)
        back[t] = np.where(taken, lags[arg], 0)
    first = max(F - p, 0)
    t = first + int(np.argmax(C[first:]))
    score, beats = int(C[t]), [t]
    while back[t]:
        t -= int(back[t])
        beats.append(t)
    return p, np.array(beats[::-1], np.int32), score


def _beats(period: int, frames: np.ndarray, score: int) -> Beats:
    frames = np.ascontiguousarray(frames, np.int32)
    return Beats(frames.astype(np.float64) / float(FPS), frames, int(period),
                 60.0 * FPS / period if period else 0.0, int(score))


def track_reference(sequences, prior_bpm: float = DEFAULT_PRIOR_BPM, tightness: float = DEFAULT_TIGHTNESS,
                    width: float = DEFAULT_WIDTH) -> List[Beats]:
    """`track` in numpy alone: the same arguments, checks and results, bit for bit"""
    prior, penalties = prior_table(prior_bpm, width), penalty_table(tightness)
    packed = pack(sequences)
    return [_beats(*track_frames(packed.frames(f), int(packed.files["n_frames"][f]), prior, penalties))
            for f in range(len(packed.files))]


@functools.lru_cache(maxsize=4)
def _device_tables(prior_bpm: float, width: float, tightness: float):
    """W and pen as one int64 CUDA tensor (W first), uploaded once per choice of parameters"""
    return note_arrays.to_device(np.concatenate([prior_table(prior_bpm, width), penalty_table(tightness).reshape(-1)]))


def run(packed: Packed, prior_bpm: float, width: float, tightness: float):
    """one upload, one mt3_op_track_beats call, one copy back -> (score i64 [files], period i32 [files], n_beats i32
    [files], beat frames i32 [total_beats]: a file's beats from its `beat0` on)"""
    import torch
    n_files = len(packed.files)
    tables = _device_tables(float(prior_bpm), float(width), float(tightness))
    period_at, count_at, beats_at = 8 * n_files, 12 * n_files, 16 * n_files
    out = torch.empty(beats_at + 4 * packed.total_beats, device="cuda", dtype=torch.uint8)
    counts = torch.empty(max(2 * packed.total_frames, 1), device="cuda", dtype=torch.int32)
    back = torch.empty(max(packed.total_frames, 1), device="cuda", dtype=torch.int16)
    notes, (frames,) = note_arrays.upload(packed.column, packed.n_notes, ("<i4",))      # the one upload
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_track_beats(
        frames, packed.n_notes, packed.files.ctypes.data, n_files, tables.data_ptr(), N_LAGS,
        tables.data_ptr() + 8 * N_LAGS, N_LAGS * PEN_STRIDE, counts.data_ptr(), back.data_ptr(), packed.total_frames,
        out.data_ptr() + period_at, out.data_ptr() + count_at, out.data_ptr() + beats_at, packed.total_beats,
        out.data_ptr(), stream.cuda_stream))
    for t in (counts, back, tables):
        t.record_stream(stream)
    host = out.cpu().numpy()                                               # the one copy back
    return (host[:period_at].view("<i8"), host[period_at: count_at].view("<i4"), host[count_at: beats_at].view("<i4"),
            host[beats_at:].view("<i4"))


def track(sequences, prior_bpm: float = DEFAULT_PRIOR_BPM, tightness: float = DEFAULT_TIGHTNESS,
          width: float = DEFAULT_WIDTH) -> List[Beats]:
    """The beats of every file of a job, on the device.  sequences: one NoteSequence (or metrics_utils.NOTE_DTYPE record
    array) per file; the order of a file's notes does not matter.  prior_bpm, width: the tempo prior's centre and its width
    in octaves; tightness: what a step that is not the period pays.  -> one `Beats` per file.  One upload, one op call, one
    copy back; there is no host fallback (`track_reference` is the yardstick, not a substitute).  ValueError, before
    anything is uploaded: not a list of sequences; a time that is not finite or is negative; a file of 2^20 frames or
    more; a bad prior_bpm, width or tightness.  An empty job gives an empty list."""
    prior_table(prior_bpm, width), penalty_table(tightness)                # their checks
    packed = pack(sequences)
    if not len(packed.files):
        return []
    score, period, count, frames = run(packed, prior_bpm, width, tightness)
    return [_beats(period[f], frames[int(b): int(b) + int(count[f])], score[f])
            for f, b in enumerate(packed.files["beat0"])]


# ---- snapping

def _check_snap(sequences, beats, subdivisions):
    sequences = _check_sequences(sequences, "snap", records=False)
    beats = list(beats)
    if len(beats) != len(sequences):
        raise ValueError("beats has %d entries for %d sequences" % (len(beats), len(sequences)))
    if isinstance(subdivisions, bool) or not isinstance(subdivisions, (int, np.integer)) or \
            not 1 <= subdivisions <= MAX_SUBDIVISIONS:
        raise ValueError("subdivisions must be 1 .. %d, got %r" % (MAX_SUBDIVISIONS, subdivisions))
    columns, frames = [], []
    for f, (seq, b) in enumerate(zip(sequences, beats)):
        start, end = note_arrays.fields(seq)[:2]
        note_arrays.check_times(start, end, not_negative=True, prefix="file %d: " % f)
        fr = np.ascontiguousarray(b.frames if isinstance(b, Beats) else b, np.int64).reshape(-1)
        if len(fr) and (fr[0] < 0 or fr[-1] >= MAX_FRAMES or (np.diff(fr) <= 0).any()):
            raise ValueError("file %d: beat frames must be strictly ascending, 0 .. %d" % (f, MAX_FRAMES - 1))
        columns.append((start, end))
        frames.append(fr.astype(np.int32))
    return sequences, columns, frames, int(subdivisions)


def snap_times(start: np.ndarray, end: np.ndarray, beat_frames: np.ndarray, subdivisions: int):
    """THE SNAPPING RULE for one file's columns -> (start', end'), float64"""
    if len(beat_frames) < 2:
        return start.copy(), end.copy()
    b = beat_frames.astype(np.float64) / float(FPS)
    sub = float(subdivisions)

    def step(t):
        i = np.clip(np.searchsorted(b, t, side="right") - 1, 0, len(b) - 2)
        return i, np.ceil(((t - b[i]) / (b[i + 1] - b[i])) * sub - 0.5)

    def point(i, k):
        return np.where(k == sub, b[i + 1], b[i] + (k / sub) * (b[i + 1] - b[i]))

    i, k = step(start)
    new_start, new_end = point(i, k), point(*step(end))
    return new_start, np.where(new_end <= new_start, point(i, k + 1.0), new_end)


def _snapped(sequences, starts, ends):
    out = []
    for seq, start, end in zip(sequences, starts, ends):
        notes = [dataclasses.replace(n, start_time=float(a), end_time=float(b)) for n, a, b in zip(seq.notes, start, end)]
        out.append(dataclasses.replace(seq, notes=notes, total_time=float(end.max()) if len(end) else 0.0,
                                       control_changes=list(seq.control_changes)))
    return out


def snap_reference(sequences, beats, subdivisions: int = 4):
    """`snap` in numpy alone, bit for bit"""
    sequences, columns, frames, subdivisions = _check_snap(sequences, beats, subdivisions)
    moved = [snap_times(s, e, fr, subdivisions) for (s, e), fr in zip(columns, frames)]
    return _snapped(sequences, [m[0] for m in moved], [m[1] for m in moved])


def snap(sequences: Sequence[note_sequences.NoteSequence], beats, subdivisions: int = 4):
    """The notes of every file of a job on the grid of its beats, `subdivisions` steps per beat (1 .. 48), on the device.
    beats: per file a `Beats` (or its beat frames).  -> new NoteSequences: the starts and ends moved (THE SNAPPING RULE
    above), every other field copied, total_time the largest end; the inputs are not touched.  A file with fewer than two
    beats keeps its times.  One upload, one op call, one copy back."""
    import torch
    sequences, columns, frames, subdivisions = _check_snap(sequences, beats, subdivisions)
    if not sequences:
        return []
    files = np.zeros(len(sequences), SNAP_FILE_DTYPE)
    files["n_notes"], files["n_beats"] = [len(s) for s, _ in columns], [len(fr) for fr in frames]
    files["first"] = note_arrays.offsets(files["n_notes"])[:-1]
    files["beat0"] = note_arrays.offsets(files["n_beats"])[:-1]
    n, n_beats = int(files["n_notes"].sum()), int(files["n_beats"].sum())
    if n == 0:
        return _snapped(sequences, [s for s, _ in columns], [e for _, e in columns])
    # the one upload: start f64 [n] | end f64 [n] | beat frames i32 [n_beats]
    data = note_arrays.to_device(np.concatenate(
        [np.concatenate([s for s, _ in columns]).astype("<f8").view(np.uint8),
         np.concatenate([e for _, e in columns]).astype("<f8").view(np.uint8),
         np.concatenate(frames).astype("<i4").view(np.uint8)]))
    out = torch.empty(2 * n, device="cuda", dtype=torch.float64)
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_snap_notes(
        data.data_ptr(), data.data_ptr() + 8 * n, n, data.data_ptr() + 16 * n if n_beats else None, n_beats,
        files.ctypes.data, len(files), subdivisions, out.data_ptr(), out.data_ptr() + 8 * n, stream.cuda_stream))
    host = out.cpu().numpy()                                               # the one copy back
    at = note_arrays.offsets(files["n_notes"])
    return _snapped(sequences, [host[at[f]: at[f + 1]] for f in range(len(files))],
                    [host[n + at[f]: n + at[f + 1]] for f in range(len(files))])
