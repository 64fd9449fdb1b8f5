"""Note preparation: known notes as the reference prepares them before tokenizing (mt3_op_prepare_notes; the rule:
include/mt3_hip.h, "note preparation", derived in DESIGN 6p).

  prepare(sequences, sustain=True, trim=False)   every file of a job on the device: per mode one pack, one upload, one op
                                                 call (a launch per 64 files) and one copy back

sustain: the sustain pedal (controller 64 of `NoteSequence.control_changes`) applied to the notes' ends, as
`note_sequences.apply_sustain_control_changes` does it event by event -- what the reference tokenizes for piano
(mt3/preprocessors.py:154); trim: `note_sequences.trim_overlapping_notes` (mt3/preprocessors.py:541).  Those two host
functions are the yardstick, bit for bit: no end is computed, each is a note start, a pedal time or the last event's time.
There is no host fallback: `prepare` needs the library and a device.
"""
from __future__ import annotations

import dataclasses
import operator
from typing import List

import numpy as np

from . import _lib, metrics_utils, note_arrays, note_sequences

SUSTAIN, TRIM = _lib.NOTE_PREP_SUSTAIN, _lib.NOTE_PREP_TRIM
MAX_INSTRUMENT = 65535                                # key = instrument << 7 | pitch stays far inside int32
NOTE_LAYOUT = ("<f8", "<f8", "<i4", "<i4")            # start | end | key | pos: what pack lays out, sorted
PEDAL_LAYOUT = ("<f8", "<i4")                         # time | instrument << 1 | (1: OFF)
FILE_DTYPE = np.dtype([("first", "<i8"), ("pedal_first", "<i8"), ("n_notes", "<i4"), ("n_pedal", "<i4"),
                       ("t_last", "<f8"), ("total_time", "<f8")])                              # mt3_note_prep_file


@dataclasses.dataclass
class Columns:
    """one file between the modes: its surviving notes as columns, `src` their positions in the caller's `ns.notes`"""
    start: np.ndarray
    end: np.ndarray
    pitch: np.ndarray
    program: np.ndarray
    drum: np.ndarray
    instrument: np.ndarray
    src: np.ndarray
    total_time: float
    pedal_time: np.ndarray              # the controller-64 events, in the caller's order
    pedal_instrument: np.ndarray
    pedal_off: np.ndarray               # 1: value < 64


@dataclasses.dataclass
class Packed:
    """the host side of one op call"""
    mode: int
    notes: np.ndarray                   # uint8: the NOTE_LAYOUT columns back to back, each file's notes sorted
    n_notes: int
    pedal: np.ndarray                   # uint8: the PEDAL_LAYOUT columns (sustain), each file's events sorted
    n_pedal: int
    files: np.ndarray                   # FILE_DTYPE [n_files]


def columns(ns, index: int = 0) -> Columns:
    """every check of `prepare` on one NoteSequence, and its columns"""
    prefix = "file %d: " % index
    start, end, pitch, _, drum, program = note_arrays.fields(ns, program=True)
    instrument = np.fromiter(map(operator.attrgetter("instrument"), ns.notes), np.int64, len(ns.notes))
    note_arrays.check_times(start, end, prefix=prefix)
    note_arrays.check_range(prefix + "pitches are 0 .. 127", pitch)
    note_arrays.check_range(prefix + "programs are 0 .. 127", program)
    if (end < start).any():
        raise ValueError(prefix + "a note ends before it starts")
    pedal = [cc for cc in ns.control_changes if cc.control_number == note_sequences.SUSTAIN_CONTROL_NUMBER]
    time = np.array([cc.time for cc in pedal], np.float64)
    pedal_instrument = np.array([cc.instrument for cc in pedal], np.int64)
    off = np.array([cc.control_value < 64 for cc in pedal], np.int64)
    note_arrays.check_times(time, prefix=prefix + "control changes: ")
    for who in (instrument, pedal_instrument):
        bad = (who < 0) | (who > MAX_INSTRUMENT)
        if bad.any():
            raise ValueError(prefix + "instruments are 0 .. %d, got %d" % (MAX_INSTRUMENT, who[bad][0]))
    if not np.isfinite(ns.total_time):
        raise ValueError(prefix + "total_time must be finite")
    return Columns(start, end, pitch, program, (drum != 0).astype(np.int64), instrument, np.arange(len(start)),
                   float(ns.total_time), time, pedal_instrument, off)


def pack(files: List[Columns], mode: int) -> Packed:
    """the keys, each file's notes sorted by (key, start, position) and its pedal by (instrument, time, ON before OFF)"""
    if mode not in (SUSTAIN, TRIM):
        raise ValueError("mode must be SUSTAIN or TRIM, got %r" % (mode,))
    note_cols, pedal_cols = [[] for _ in NOTE_LAYOUT], [[] for _ in PEDAL_LAYOUT]
    table = np.zeros(len(files), FILE_DTYPE)
    for f, c in enumerate(files):
        pos = np.arange(len(c.start))
        key = (c.instrument << 7) | c.pitch if mode == SUSTAIN else (c.drum << 14) | (c.program << 7) | c.pitch
        by = np.lexsort((pos, c.start, key))                            # the last key is the primary one
        for col, a in zip(note_cols, (c.start, c.end, key, pos)):
            col.append(a[by])
        n_pedal = len(c.pedal_time) if mode == SUSTAIN else 0
        if n_pedal:
            by = np.lexsort((c.pedal_off, c.pedal_time, c.pedal_instrument))
            pedal_cols[0].append(c.pedal_time[by])
            pedal_cols[1].append((c.pedal_instrument[by] << 1) | c.pedal_off[by])
        times = np.concatenate([c.start, c.end, c.pedal_time[:n_pedal]])
        t_last = float(times.max()) if len(times) else 0.0
        table[f] = (0, 0, len(pos), n_pedal, t_last, c.total_time)
    first, pedal_first = note_arrays.offsets(table["n_notes"]), note_arrays.offsets(table["n_pedal"])
    table["first"], table["pedal_first"] = first[:-1], pedal_first[:-1]
    return Packed(mode, note_arrays.pack(note_cols, NOTE_LAYOUT), int(first[-1]), note_arrays.pack(pedal_cols, PEDAL_LAYOUT),
                  int(pedal_first[-1]), table)


def _output_layout(packed: Packed):
    """byte offsets in the op's one output buffer: end f64 [n] | total_time f64 [files] | src i32 [n] | counts i32 [files]"""
    n, n_files = packed.n_notes, len(packed.files)
    return 0, 8 * n, 8 * (n + n_files), 12 * n + 8 * n_files


def launch(packed: Packed):
    """one upload and one mt3_op_prepare_notes call -> the op's output buffer on the device (`fetch` reads it)"""
    import torch
    n, n_pedal, n_files = packed.n_notes, packed.n_pedal, len(packed.files)
    end_at, total_at, src_at, counts_at = _output_layout(packed)
    out = torch.empty(counts_at + 4 * n_files, device="cuda", dtype=torch.uint8)
    scratch = torch.empty(3 * n + n_pedal, device="cuda", dtype=torch.int32)
    data, ptr = note_arrays.upload(np.concatenate([packed.notes, packed.pedal]), n + n_pedal, ("u1",))   # the one upload
    note_at = note_arrays.column_offsets([np.dtype(dt).itemsize for dt in NOTE_LAYOUT], n)
    pedal_at = note_arrays.column_offsets([np.dtype(dt).itemsize for dt in PEDAL_LAYOUT], n_pedal)
    note_ptr = [ptr[0] + a if n else None for a in note_at]
    pedal_ptr = [ptr[0] + len(packed.notes) + a if n_pedal else None for a in pedal_at]
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_prepare_notes(
        packed.mode, *note_ptr, n, *pedal_ptr, n_pedal, packed.files.ctypes.data, n_files,
        *[out.data_ptr() + a if n else None for a in (end_at, src_at)], out.data_ptr() + counts_at,
        out.data_ptr() + total_at, scratch.data_ptr() if scratch.numel() else None, scratch.numel(), stream.cuda_stream))
    scratch.record_stream(stream)
    return out


def fetch(packed: Packed, out):
    """the one copy back -> (end f64, src i32: a file's survivors from its `first` on, entries past its count are whatever
    the buffer held; counts int64 [n_files]; total_time f64 [n_files])"""
    end_at, total_at, src_at, counts_at = _output_layout(packed)
    host = out.cpu().numpy()
    return (host[end_at: total_at].view("<f8"), host[src_at: counts_at].view("<i4"),
            host[counts_at:].view("<i4").astype(np.int64), host[total_at: src_at].view("<f8"))


def run(packed: Packed):
    """one upload, one op call, one copy back"""
    return fetch(packed, launch(packed))


def apply(files: List[Columns], mode: int) -> List[Columns]:
    """one mode over the job: the survivors of every file, in its order, with their new ends and the new total_time"""
    packed = pack(files, mode)
    end, src, counts, total = run(packed)
    out = []
    for c, f, n, t in zip(files, packed.files, counts, total):
        a = int(f["first"])
        keep = src[a: a + n].astype(np.int64)
        out.append(Columns(c.start[keep], end[a: a + n].copy(), c.pitch[keep], c.program[keep], c.drum[keep],
                           c.instrument[keep], c.src[keep], float(t), c.pedal_time, c.pedal_instrument, c.pedal_off))
    return out


def prepare(sequences, sustain: bool = True, trim: bool = False, as_arrays: bool = False) -> list:
    """The notes of every file of a job, prepared on the device.  sequences: NoteSequences.  sustain: apply each file's
    sustain pedal (`note_sequences.apply_sustain_control_changes`); trim: then trim overlapping notes of one (pitch,
    program, is_drum) and drop the empty ones (`note_sequences.trim_overlapping_notes`).  -> one new NoteSequence per file:
    the surviving notes in their order, copies with the new `end_time`, the new `total_time`, `control_changes` cleared; or,
    as_arrays, one `metrics_utils.NOTE_DTYPE` record array per file (what `pianoroll.pianorolls` and `note_matching.match`
    take).  Per mode one upload, one op call, one copy back.  ValueError, before anything is uploaded: a time that is not
    finite, a note that ends before it starts, a pitch or program outside 0 .. 127, an instrument outside 0 .. 65535.
    Limit: a pedal holds the notes of its own `instrument` number only (the MIDI reader numbers every non-drum channel 0)."""
    sequences = list(sequences)
    files = [columns(ns, f) for f, ns in enumerate(sequences)]
    if sequences:
        for wanted, mode in ((sustain, SUSTAIN), (trim, TRIM)):
            if wanted:
                files = apply(files, mode)
    out = []
    for ns, c in zip(sequences, files):
        if as_arrays:
            notes = np.zeros(len(c.src), metrics_utils.NOTE_DTYPE)
            notes["start_time"], notes["end_time"], notes["pitch"] = c.start, c.end, c.pitch
            notes["velocity"] = [ns.notes[i].velocity for i in c.src]
            notes["program"], notes["is_drum"], notes["instrument"] = c.program, c.drum, c.instrument
            out.append(notes)
        else:
            out.append(note_sequences.NoteSequence(
                notes=[dataclasses.replace(ns.notes[i], end_time=float(e)) for i, e in zip(c.src, c.end)],
                total_time=c.total_time, ticks_per_quarter=ns.ticks_per_quarter))
    return out
