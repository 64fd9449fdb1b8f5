"""The target tokenizer: known notes -> the id rows the model is trained on (the rule: include/mt3_hip.h, "target tokenizer").

The target side of the reference's data pipeline (mt3/preprocessors.py:93-226 tokenize_transcription_example, then
mt3/tasks.py:160-180) for the segments the inference path cuts, so that (audio, notes) pairs can be scored: per segment the
tie section, the run-length encoded events, the program granularity, redundant state changes removed, EOS.  Three
statements of it, compared row for row by the tests:
  target_rows_reference   the host mirror, event by event in Python (run_length_encoding.encode_and_index_events,
                          segment_targets, remove_redundant_state_changes): the recipe, stated once;
  target_rows_host        mt3_notes_tokenize: the C rule on host arrays, one row per call;
  target_rows             mt3_op_tokenize_notes: a whole job of files in ONE upload of the packed events and ONE launch; the
                          rows stay on the device, where `InferenceModel.score_notes` scores them.  No host fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from . import note_arrays
from . import note_sequences
from . import run_length_encoding
from . import vocabularies

FILE_DTYPE = np.dtype([("event0", "<i8"), ("n_events", "<i4"), ("row0", "<i4"), ("n_rows", "<i4"),
                       ("reserved", "<i4")])                                                     # mt3_tokenize_file
ROW_DTYPE = np.dtype([("file", "<i4"), ("step_lo", "<i4"), ("step_hi", "<i4"), ("reserved", "<i4")])   # mt3_tokenize_row
INT32_MAX = 2 ** 31 - 1
FRAMES_PER_SECOND = 125.0                # spectrograms.SpectrogramConfig: 16000 / 128


def _spec_id(spec) -> int:
    spec_id = int(getattr(spec, "spec_id", spec))
    if spec_id not in (_lib.SPEC_NOTES, _lib.SPEC_TIES):
        raise ValueError("the target tokenizer takes NoteEncodingSpec or NoteEncodingWithTiesSpec, got %r" % (spec,))
    return spec_id


def segment_frames_of(spec) -> int:
    """the segment length of the preset that uses `spec`: 256 frames for `mt3`, 512 for `ismir2021`"""
    return 256 if _spec_id(spec) == _lib.SPEC_TIES else 512


def tokenize_rule(codec, spec, vocab_size: Optional[int] = None, granularity: str = "full") -> _lib.TokenizeRule:
    """The rule descriptor of `codec` (`mt3_codec_tokenize_rule`).  ValueError for what the library refuses: the
    onsets-only spec, an unknown granularity, a codec without the ranges the rule writes."""
    if granularity not in _lib.GRANULARITIES:
        raise ValueError("granularity must be one of %s, got %r" % (sorted(_lib.GRANULARITIES), granularity))
    if vocab_size is None:
        vocab_size = vocabularies.num_embeddings(vocabularies.vocabulary_from_codec(codec))
    rule, lib = _lib.TokenizeRule(), _lib.load()
    rc = lib.mt3_codec_tokenize_rule(C.byref(codec.desc), int(getattr(spec, "spec_id", spec)), int(vocab_size),
                                     _lib.GRANULARITIES[granularity], C.byref(rule))
    if rc != 0:
        raise ValueError(lib.mt3_last_error().decode())
    return rule


def segment_steps(n_frames: int, codec, segment_frames: int, frames_per_second: float = FRAMES_PER_SECOND) -> np.ndarray:
    """int32 [n_segments, 2]: (step_lo, step_hi) of the segments [s * segment_frames, ...) of a file of `n_frames` frames:
    k[first frame] - 1 with k = `run_length_encoding._first_step_after`, the reference's own float comparison; the last
    segment's step_hi is INT32_MAX (it takes every later event).  A file always has one segment."""
    n_frames = max(int(n_frames), 1)
    first = np.arange(0, n_frames, int(segment_frames))
    k = run_length_encoding._first_step_after(first / frames_per_second, codec.steps_per_second)
    lo = (k - 1).astype(np.int64)
    hi = np.concatenate([lo[1:], [INT32_MAX]])
    return np.stack([lo, hi], axis=1).astype(np.int32)


@dataclasses.dataclass
class Packed:
    """the host side of one op call"""
    events: np.ndarray                  # int32 [6, n_events]: step | pitch | program | velbin | is_drum | note
    event0: np.ndarray                  # int64 [n_files + 1]: file i's events are [event0[i], event0[i + 1])


def pack(sequences: Sequence[note_sequences.NoteSequence], codec, spec, shifts: Optional[Sequence[float]] = None) -> Packed:
    """The events of every file in the reference's order.  Ties spec: notes sorted by (is_drum, program, pitch), the
    offsets of the non-drum notes, then all onsets (note_sequence_to_onsets_and_offsets_and_programs); notes spec: sorted
    by pitch, an offset for every note, drums not told apart (note_sequence_to_onsets_and_offsets); then a stable sort by
    float64 time (numpy's).  step = rint(time * steps_per_second) on the float64 product, Python's round.  shifts: every
    file once per shift, file-major (file i under shift j is entry i * len(shifts) + j): the shift is added to every note
    time and the sum clamped at 0."""
    ties = _spec_id(spec) == _lib.SPEC_TIES
    bins = vocabularies.num_velocity_bins_from_codec(codec)
    sps = float(codec.steps_per_second)
    chunks, event0 = [], [0]
    for ns in sequences:
        start, end, pitch, velocity, drum, program = note_arrays.fields(ns, program=True)
        drum = drum != 0
        if not ties:                                                    # the notes spec: program 0, drums not told apart
            program, drum = np.zeros_like(program), np.zeros_like(drum)
        note_arrays.check_times(start, end)
        note_arrays.check_range("pitches, programs and velocities must be in 0 .. 127", pitch, program, velocity, got=False)
        order = np.lexsort((pitch, program, drum))                      # stable, like sorted(): last key first
        off = order[~drum[order]]
        who = np.concatenate([off, order])
        velbin = np.concatenate([np.zeros(len(off), np.int64),
                                 np.ceil(bins * velocity[order] / vocabularies.MAX_MIDI_VELOCITY).astype(np.int64)])
        times = np.concatenate([end[off], start[order]])
        for shift in ([None] if shifts is None else shifts):
            t = times if shift is None else np.maximum(times + float(shift), 0.0)
            by_time = np.argsort(t, kind="stable")
            step = np.clip(np.rint(t[by_time] * sps), 0, INT32_MAX - 1)
            w = who[by_time]
            chunks.append(np.stack([step, pitch[w], program[w], velbin[by_time], drum[w].astype(np.int64), w]).astype(np.int32))
            event0.append(event0[-1] + len(w))
    events = np.ascontiguousarray(np.concatenate(chunks, axis=1)) if chunks else np.zeros((6, 0), np.int32)
    return Packed(events, np.asarray(event0, np.int64))


@dataclasses.dataclass
class Job:
    """`pack` plus the two tables of the op call"""
    packed: Packed
    files: np.ndarray                   # FILE_DTYPE [n_files * n_shifts]
    rows: np.ndarray                    # ROW_DTYPE [n_rows]
    rule: _lib.TokenizeRule
    stride: int
    rows_of_file: np.ndarray            # int64 [n_files, n_shifts or 1, 2]: first row and number of rows


def plan(sequences, n_frames, codec, spec, granularity="full", stride=1024, shifts=None, segment_frames=None,
         frames_per_second=FRAMES_PER_SECOND, vocab_size=None) -> Job:
    """the host work of `target_rows`: events, tables and rule"""
    if len(n_frames) != len(sequences):
        raise ValueError("n_frames has %d entries for %d files" % (len(n_frames), len(sequences)))
    if not 2 <= int(stride) <= _lib.TOKENIZE_MAX_STRIDE:
        raise ValueError("stride must be in [2, 2^20], got %r" % (stride,))
    rule = tokenize_rule(codec, spec, vocab_size, granularity)
    seg = segment_frames_of(spec) if segment_frames is None else int(segment_frames)
    if seg < 1:
        raise ValueError("segment_frames must be at least 1")
    packed = pack(sequences, codec, spec, shifts)
    per = 1 if shifts is None else len(shifts)
    files = np.zeros(len(sequences) * per, FILE_DTYPE)
    tables, row0 = [], 0
    for i, frames in enumerate(n_frames):
        steps = segment_steps(frames, codec, seg, frames_per_second)
        for j in range(per):
            f = i * per + j
            files[f] = (packed.event0[f], packed.event0[f + 1] - packed.event0[f], row0, len(steps), 0)
            t = np.zeros(len(steps), ROW_DTYPE)
            t["file"], t["step_lo"], t["step_hi"] = f, steps[:, 0], steps[:, 1]
            tables.append(t)
            row0 += len(steps)
    rows = np.concatenate(tables) if tables else np.zeros(0, ROW_DTYPE)
    rows_of_file = np.stack([files["row0"], files["n_rows"]], axis=1).astype(np.int64).reshape(len(sequences), per, 2)
    return Job(packed, files, rows, rule, int(stride), rows_of_file)


@dataclasses.dataclass
class TargetRows:
    """What `target_rows` / `target_rows_host` return: torch CUDA tensors / numpy arrays.  ids int32 [rows, stride],
    0-padded; lengths int32 [rows], EOS included; truncated int32 [rows]; note_of int32 [rows, stride]: the index in the
    file's `ns.notes` of the note whose pitch or drum id stands there in the event part, else -1; is_onset uint8
    [rows, stride]; rows_of_file int64 [n_files, n_shifts or 1, 2]: (first row, rows) of each file under each shift."""
    ids: object
    lengths: object
    truncated: object
    note_of: object
    is_onset: object
    rows_of_file: np.ndarray

    def __iter__(self):
        return iter((self.ids, self.lengths, self.truncated, self.note_of, self.is_onset, self.rows_of_file))


def run(job: Job) -> TargetRows:
    """upload + mt3_op_tokenize_notes; nothing is copied back and nothing is waited for"""
    import torch
    n_rows, stride, n_ev = len(job.rows), job.stride, job.packed.events.shape[1]
    dev = dict(device="cuda", dtype=torch.int32)
    ids = torch.empty((n_rows, stride), **dev)
    note_of = torch.empty((n_rows, stride), **dev)
    is_onset = torch.empty((n_rows, stride), device="cuda", dtype=torch.uint8)
    lengths, truncated = torch.empty(n_rows, **dev), torch.empty(n_rows, **dev)
    if n_rows:
        events, ptr = note_arrays.upload(job.packed.events, n_ev, ("<i4",) * 6)
        files = note_arrays.to_device(job.files.view(np.uint8))
        rows = note_arrays.to_device(job.rows.view(np.uint8))
        _lib.check(_lib.load().mt3_op_tokenize_notes(
            C.byref(job.rule), *ptr, n_ev, files.data_ptr(), len(job.files), rows.data_ptr(), n_rows, stride,
            ids.data_ptr(), lengths.data_ptr(), truncated.data_ptr(), note_of.data_ptr(), is_onset.data_ptr(),
            torch.cuda.current_stream().cuda_stream))
    return TargetRows(ids, lengths, truncated, note_of, is_onset, job.rows_of_file)


def target_rows(sequences, n_frames, codec, spec, granularity="full", stride=1024, shifts=None, *, segment_frames=None,
                frames_per_second=FRAMES_PER_SECOND, vocab_size=None) -> TargetRows:
    """The target rows of a job of files on the device: `sequences[i]` against audio of `n_frames[i]` spectrogram frames,
    cut into segments of `segment_frames` (default: the preset's, 256 for the ties spec and 512 for the notes spec).
    granularity: 'full', 'midi_class' or 'flat' (mt3/vocabularies.py PROGRAM_GRANULARITIES, the token side).  stride: the
    row length; a segment that does not fit is cut, ends without EOS and has truncated = 1.  shifts: tokenize every file
    once per global time shift (seconds, added to every note time, clamped at 0): an offset search in one launch."""
    return run(plan(sequences, n_frames, codec, spec, granularity, stride, shifts, segment_frames, frames_per_second,
                    vocab_size))


def target_rows_host(sequences, n_frames, codec, spec, granularity="full", stride=1024, shifts=None, *,
                     segment_frames=None, frames_per_second=FRAMES_PER_SECOND, vocab_size=None) -> TargetRows:
    """`target_rows` through mt3_notes_tokenize, row by row on the host (numpy arrays): the kernel's yardstick"""
    job = plan(sequences, n_frames, codec, spec, granularity, stride, shifts, segment_frames, frames_per_second, vocab_size)
    n_rows, lib = len(job.rows), _lib.load()
    ids, note_of = np.zeros((n_rows, job.stride), np.int32), np.zeros((n_rows, job.stride), np.int32)
    is_onset = np.zeros((n_rows, job.stride), np.uint8)
    lengths, truncated = np.zeros(n_rows, np.int32), np.zeros(n_rows, np.int32)
    for i, row in enumerate(job.rows):
        f = job.files[row["file"]]
        ev = np.ascontiguousarray(job.packed.events[:, f["event0"]: f["event0"] + f["n_events"]])
        ptr = [ev[k].ctypes.data for k in range(6)] if ev.shape[1] else [None] * 6
        length, cut = C.c_int32(), C.c_int32()
        _lib.check(lib.mt3_notes_tokenize(C.byref(job.rule), *ptr, ev.shape[1], int(row["step_lo"]), int(row["step_hi"]),
                                          job.stride, ids[i].ctypes.data, note_of[i].ctypes.data, is_onset[i].ctypes.data,
                                          C.byref(length), C.byref(cut)))
        lengths[i], truncated[i] = length.value, cut.value
    return TargetRows(ids, lengths, truncated, note_of, is_onset, job.rows_of_file)


def target_rows_reference(ns, n_frames: int, codec, spec, granularity="full", stride=1024, *, segment_frames=None,
                          frames_per_second=FRAMES_PER_SECOND):
    """The recipe in the host mirror's own functions, for ONE file: (rows, truncated) -- a list of int32 id arrays (event
    index + 3, EOS appended, cut to `stride`) and a list of 0 / 1.  mt3/tasks.py:160-180 in order: the tie section and the
    segment's events (`segment_targets`: extract_target_sequence_with_indices + run_length_encode_shifts; the program
    map in between touches no shift, so it commutes with the run-length step), the granularity's token map, then
    `remove_redundant_state_changes(['velocity', 'program'])`, trim, EOS."""
    ties = _spec_id(spec) == _lib.SPEC_TIES
    if granularity not in _lib.GRANULARITIES:
        raise ValueError("granularity must be one of %s, got %r" % (sorted(_lib.GRANULARITIES), granularity))
    seg = segment_frames_of(spec) if segment_frames is None else int(segment_frames)
    n_frames = max(int(n_frames), 1)
    NS = note_sequences
    if ties:
        times, values = NS.note_sequence_to_onsets_and_offsets_and_programs(ns)
        state, state_fn = NS.NoteEncodingState(), NS.note_encoding_state_to_events
    else:
        times, values = NS.note_sequence_to_onsets_and_offsets(ns)
        state, state_fn = None, None
    frame_times = np.arange(n_frames) / frames_per_second
    ev, start, end, state_ev, state_idx = run_length_encoding.encode_and_index_events(
        state, times, values, NS.note_event_data_to_events, codec, frame_times, state_fn)
    lo, hi = codec.event_type_range("program")
    rows, truncated = [], []
    for f_lo in range(0, n_frames, seg):
        t = run_length_encoding.segment_targets(ev, start, end, state_ev, state_idx, f_lo, min(f_lo + seg, n_frames), codec,
                                                ties).astype(np.int64)
        is_program = (t >= lo) & (t <= hi)
        if granularity == "flat":
            t = t[~is_program]
        elif granularity == "midi_class":
            t = np.where(is_program, lo + 8 * ((t - lo) // 8), t)
        t = run_length_encoding.remove_redundant_state_changes(t, codec, ("velocity", "program"))
        full = np.concatenate([t.astype(np.int32) + 3, np.array([1], np.int32)])
        rows.append(full[:stride])
        truncated.append(int(len(full) > stride))
    return rows, truncated
