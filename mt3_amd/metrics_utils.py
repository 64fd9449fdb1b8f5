"""Prediction combiner (mirror of mt3/metrics_utils.py:38-146) over libmt3hip.so."""
from __future__ import annotations

import collections
import ctypes as C
from typing import Any, Mapping, Optional, Sequence

import numpy as np

from . import _lib
from . import event_codec
from . import note_arrays
from . import note_sequences


# mt3_note of include/mt3_hip.h as a numpy record: the host stage's output without one Python object per note
NOTE_DTYPE = np.dtype([("start_time", "<f8"), ("end_time", "<f8"), ("pitch", "<i4"), ("velocity", "<i4"),
                       ("program", "<i4"), ("is_drum", "<i4"), ("instrument", "<i4"), ("reserved", "<i4")])
assert NOTE_DTYPE.itemsize == C.sizeof(_lib.NoteStruct)


def _decode(codec, spec_id, flat, offs, start_times, max_times=None):
    """mt3_notes_decode on a flat token array: (notes as a NOTE_DTYPE array, invalid, dropped, total_time)"""
    return _decode_full(codec, spec_id, flat, offs, start_times, max_times, False)[:4]


def _decode_full(codec, spec_id, flat, offs, start_times, max_times, trace):
    """always five items: `_decode`'s four and the trace -- with `trace` (mt3_notes_decode_traced) int64 [n_notes, 2], the
    flat indices of each note's onset and end tokens; None otherwise (mt3_notes_decode)"""
    lib = _lib.load()
    n = len(offs) - 1
    flat = np.ascontiguousarray(flat, np.int32) if n and offs[-1] else np.zeros(1, np.int32)
    offs = np.ascontiguousarray(offs, np.int64)
    st = np.ascontiguousarray(np.asarray(start_times, np.float64).reshape(-1)) if n else np.zeros(1)
    has_p = mt_p = None
    if max_times is not None:
        has = np.array([0 if m is None else 1 for m in max_times], np.int32)
        mts = np.array([0.0 if m is None else float(m) for m in max_times], np.float64)
        has_p, mt_p = has.ctypes.data, mts.ctypes.data
    cap = max(64, int(offs[-1]) + 8)          # a token emits at most one note
    notes = np.empty(cap, NOTE_DTYPE)
    n_notes, inv, drop, total = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
    args = (C.byref(codec.desc), spec_id, n, flat.ctypes.data, offs.ctypes.data, st.ctypes.data, has_p, mt_p,
            C.c_void_p(notes.ctypes.data), cap, C.byref(n_notes), C.byref(inv), C.byref(drop), C.byref(total))
    if not trace:
        _lib.check(lib.mt3_notes_decode(*args))
        return notes[: n_notes.value], inv.value, drop.value, total.value, None
    note_tokens = np.full((cap, 2), -1, np.int64)
    _lib.check(lib.mt3_notes_decode_traced(*args, C.c_void_p(note_tokens.ctypes.data)))
    return notes[: n_notes.value], inv.value, drop.value, total.value, note_tokens[: n_notes.value]


def decode_token_rows(codec, encoding_spec, rows, start_times, lengths=None):
    """The host stage of a JOB (bench.py, distributed.ShardedTranscriber): `decode_tf`-form token rows int32 [n, L] of the
    consecutive segments of ONE file -> (notes as a NOTE_DTYPE record array, invalid events, dropped events, total_time),
    with no per-row and no per-note Python work (event_predictions_to_ns builds a NoteSequence of Note objects: 2-3 us per
    note under the GIL, which is what bounded rank 0 at N = 8 -- DESIGN.md section 6).  lengths: tokens per row; None = up
    to the first -1 (`_trim_eos`, NB:346-352).  Same combiner rule as event_predictions_to_ns (max_time = the next
    segment's start, mt3/metrics_utils.py:92-116); rows must be in start-time order."""
    rows = np.ascontiguousarray(rows, np.int32)
    if rows.ndim != 2:
        raise ValueError("rows must be [segments, length]")
    if lengths is None:
        eos = rows == -1
        lengths = np.where(eos.any(1), eos.argmax(1), rows.shape[1])
    lengths = np.asarray(lengths, np.int64)
    offs = note_arrays.offsets(lengths)
    flat = rows[np.arange(rows.shape[1])[None, :] < lengths[:, None]]
    return _decode(codec, encoding_spec.spec_id, flat, offs, start_times)


def note_sequence_from_records(rec, total_time: float):
    ns = note_sequences.NoteSequence(total_time=total_time)
    Note = note_sequences.Note
    ns.notes = [Note(a, b, p, v, g, bool(d), i) for a, b, p, v, g, d, i, _ in rec.tolist()]
    return ns


def _run(codec, spec_id, tokens_list, start_times, max_times=None):
    """(NoteSequence, invalid events, dropped events) of the segments"""
    return _run_full(codec, spec_id, tokens_list, start_times, max_times, False)[:3]


def _run_full(codec, spec_id, tokens_list, start_times, max_times, trace):
    """always four items: `_run`'s three and, with `trace`, int64 [n_notes, 2, 2] (segment, position) pairs of each note's
    onset and end token ((-1, -1): none); None otherwise"""
    n = len(tokens_list)
    toks = [np.asarray(t, np.int32).reshape(-1) for t in tokens_list]
    offs = note_arrays.offsets([t.size for t in toks])
    flat = np.concatenate(toks) if n and offs[-1] else np.zeros(1, np.int32)
    rec, inv, drop, total, flat_idx = _decode_full(codec, spec_id, flat, offs, start_times, max_times, trace)
    if flat_idx is None:
        return note_sequence_from_records(rec, total), inv, drop, None
    # flat index -> (segment, position in that segment's row); -1 -> (-1, -1)
    seg = np.searchsorted(offs, flat_idx, side="right") - 1
    note_tokens = np.stack([seg, flat_idx - offs[np.clip(seg, 0, max(n - 1, 0))]], axis=-1).astype(np.int64)
    note_tokens[flat_idx < 0] = -1
    return note_sequence_from_records(rec, total), inv, drop, note_tokens


def event_predictions_to_ns(predictions: Sequence[Mapping[str, Any]], codec: event_codec.Codec,
                            encoding_spec: note_sequences.NoteEncodingSpecType) -> Mapping[str, Any]:
    """predictions: dicts with 'est_tokens', 'start_time' (and optionally 'raw_inputs')."""
    return _predictions_to_ns(predictions, codec, encoding_spec, False)


def event_predictions_to_ns_traced(predictions: Sequence[Mapping[str, Any]], codec: event_codec.Codec,
                                   encoding_spec: note_sequences.NoteEncodingSpecType) -> Mapping[str, Any]:
    """`event_predictions_to_ns` plus 'note_tokens': int64 [n_notes, 2, 2], for each note of est_ns.notes the (index into
    `predictions`, position in that prediction's 'est_tokens') of the token that started it ([:, 0]: the PITCH / DRUM
    onset, possibly in an earlier segment) and of the token that ended it ([:, 1]: a note-off PITCH, a re-onset or the
    TIE that closed an undeclared note; (-1, -1) where no token did) -- mt3_notes_decode_traced (include/mt3_hip.h)."""
    return _predictions_to_ns(predictions, codec, encoding_spec, True)


def _predictions_to_ns(predictions, codec, encoding_spec, trace):
    ns, inv, drop, note_tokens = _run_full(codec, encoding_spec.spec_id, [p["est_tokens"] for p in predictions],
                                           [p["start_time"] for p in predictions], None, trace)
    order = sorted(range(len(predictions)), key=lambda i: predictions[i]["start_time"])
    raws = [np.asarray(predictions[i].get("raw_inputs", [])) for i in order]
    raws = [r for r in raws if r.size]
    return {
        "raw_inputs": np.concatenate(raws, axis=0) if raws else np.zeros((0,), np.float32),
        "start_times": [predictions[i]["start_time"] for i in order],
        "est_ns": ns,
        "est_invalid_events": inv,
        "est_dropped_events": drop,
        **({"note_tokens": note_tokens} if trace else {}),
    }


def decode_events_single(tokens, start_time, max_time: Optional[float], codec: event_codec.Codec,
                         encoding_spec: note_sequences.NoteEncodingSpecType):
    """One call of run_length_encoding.decode_events on a fresh state + flush."""
    return _run(codec, encoding_spec.spec_id, [tokens], [start_time], [max_time])


def combine_predictions_by_id(predictions, combine_predictions_fn):
    by_id = collections.defaultdict(list)
    for p in predictions:
        by_id[p["unique_id"]].append(p)
    return {k: combine_predictions_fn(v) for k, v in by_id.items()}


# --------------------------------------------------------------- frame-level: mt3/metrics_utils.py:149-196 by their names
def get_prettymidi_pianoroll(ns: note_sequences.NoteSequence, fps: float, is_drum: bool) -> np.ndarray:
    """mt3/metrics_utils.py:149-171: the piano roll pretty_midi would render from `ns`, float64 numpy [128, F] as the
    reference returns it.  Rasterised on the device (mt3_amd.pianoroll.pianorolls, one call; there is no host path) and
    copied back; callers with many sequences, or who want the roll to stay on the device, call `pianorolls` itself.
    Unlike the reference, `ns` is left as it is: the 0.05 s minimum length is applied to a copy of the times."""
    from . import pianoroll
    return pianoroll.pianorolls([ns], fps, is_drum)[0].cpu().numpy().astype(np.float64)


def frame_metrics(ref_pianoroll, est_pianoroll, velocity_threshold: int):
    """mt3/metrics_utils.py:174-196: (precision, recall, f1) of the frames, Python floats.  The rolls are numpy arrays or
    CUDA tensors [128, F_ref], [128, F_est]; the narrower counts as zero-padded, a reference cell is on above
    `velocity_threshold`, an estimated cell above 0, and the cells are counted on the device (mt3_op_frame_counts)."""
    from . import pianoroll
    return pianoroll.precision_recall_f1(*pianoroll.roll_pair_counts(ref_pianoroll, est_pianoroll, velocity_threshold))
