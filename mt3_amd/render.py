"""NoteSequences rendered to audio on the device (mt3_op_render_notes; the rule: include/mt3_hip.h, "rendering notes to
audio"): the way to LISTEN to a transcription, and to put a reference and a prediction side by side as
mt3/summaries.py:111-161 does for every evaluation.

One voice for every program -- the harmonic tone of `synthetic.render_notes` (six partials at 1/k, 4 ms attack,
exp(-t / 0.7 s) decay, 40 ms release) with zero phases and a fixed summation order, and a 150 ms noise burst for a drum
note -- so the same notes give the same bits on every run and every device.  It is this project's own voice: parity with
fluidsynth, pretty_midi or any other synthesiser is not claimed.  All the audio of a job comes from ONE upload of the packed
notes and ONE call.  There is no host fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

from . import _lib, note_arrays

TILE = _lib.RENDER_TILE                           # samples per workgroup of the render kernel
MAX_SAMPLE_RATE = _lib.RENDER_MAX_SAMPLE_RATE
RELEASE_SECONDS = _lib.RENDER_RELEASE_SECONDS
DRUM_SECONDS = _lib.RENDER_DRUM_SECONDS
DEFAULT_SAMPLE_RATE = 16000
LAYOUT = ("<f8", "<f8", "<f8", "<i4", "<i4", "<i4")   # the types of the columns that _pack lays out


def _rate(sample_rate) -> int:
    if isinstance(sample_rate, bool) or not 1 <= sample_rate <= MAX_SAMPLE_RATE or int(sample_rate) != sample_rate:
        raise ValueError("sample_rate must be an integer 1 .. %d, got %r" % (MAX_SAMPLE_RATE, sample_rate))
    return int(sample_rate)


def sounding_instants(start: np.ndarray, end: np.ndarray, drum: np.ndarray) -> np.ndarray:
    """float64 [n]: when each note falls silent -- end + 0.04 (the release), start + 0.15 for a drum note whatever its end"""
    return np.where(np.asarray(drum).astype(bool), start + DRUM_SECONDS, end + RELEASE_SECONDS)


def render_length(start: np.ndarray, end: np.ndarray, drum: np.ndarray, sample_rate: int = DEFAULT_SAMPLE_RATE) -> int:
    """n_samples of one sequence when the caller gives none: ceil(sample_rate * latest sounding instant) in float64; no
    notes: 0.  The one place lengths come from."""
    if len(start) == 0:
        return 0
    return int(math.ceil(float(_rate(sample_rate)) * float(sounding_instants(start, end, drum).max())))


def _pack(sequences, sample_rate: int, lengths):
    """the job's notes, each sequence's sorted by (start, end, pitch, velocity, is_drum), as one byte buffer (start f64 |
    end f64 | reach f64 | pitch i32 | velocity i32 | is_drum i32, each [n]; reach = the running maximum of the sounding
    instants within the sequence) and the host tables: note offsets int64 [n_seq + 1], lengths int64 [n_seq]"""
    parts = [note_arrays.fields(s) for s in sequences]
    if lengths is not None:
        lengths = [int(v) for v in lengths]
        if len(lengths) != len(parts):
            raise ValueError("%d lengths for %d sequences" % (len(lengths), len(parts)))
    offs = note_arrays.offsets([len(p[0]) for p in parts])
    n_samples = np.zeros(len(parts), np.int64)
    cols = [[] for _ in range(6)]
    for i, (start, end, pitch, velocity, drum) in enumerate(parts):
        note_arrays.check_range("sequence %d: pitches are 0 .. 127" % i, pitch)
        note_arrays.check_range("sequence %d: velocities are 0 .. 127" % i, velocity)
        note_arrays.check_times(start, end, not_negative=True, prefix="sequence %d: " % i)
        if (end < start).any():
            raise ValueError("sequence %d: a note ends before it starts" % i)
        n = render_length(start, end, drum, sample_rate) if lengths is None else lengths[i]
        if not 0 <= n <= _lib.RENDER_MAX_SAMPLES:
            raise ValueError("sequence %d: %d samples: a length is 0 .. 2^40" % (i, n))
        n_samples[i] = n
        drum = (drum != 0).astype(np.int64)
        order = np.lexsort((drum, velocity, pitch, end, start))        # the last key is the primary one
        start, end, pitch, velocity, drum = (a[order] for a in (start, end, pitch, velocity, drum))
        reach = np.maximum.accumulate(sounding_instants(start, end, drum)) if len(start) else start
        for c, a in zip(cols, (start, end, reach, pitch, velocity, drum)):
            c.append(a)
    return note_arrays.pack(cols, LAYOUT), int(offs[-1]), offs, n_samples


def render(sequences: Sequence, sample_rate: int = DEFAULT_SAMPLE_RATE, lengths: Optional[Sequence[int]] = None,
           normalize: bool = True) -> list:
    """The audio of `sequences` (NoteSequences; NOTE_DTYPE record arrays are taken too): a list of float32 CUDA tensors
    [n_i] at `sample_rate`, views of one buffer written by one mt3_op_render_notes call after one upload of the packed
    notes.  n_i = lengths[i], or `render_length` of the sequence's notes (its last note's release included).  With
    `normalize` every sequence is scaled to a peak of 0.9 (mt3/mixing.py:71-75); a silent one stays zeros.  Programs are
    ignored: one timbre.  The sequences are not modified, and the order of their notes does not matter.  ValueError, before
    anything is uploaded, for a pitch or velocity outside 0 .. 127, a negative or non-finite time, a note that ends before
    it starts, or a sample rate outside 1 .. 384000.  An empty list gives an empty list."""
    import torch
    sample_rate = _rate(sample_rate)
    sequences = list(sequences)
    if not sequences:
        return []
    packed, n, offs, n_samples = _pack(sequences, sample_rate, lengths)
    first = note_arrays.offsets(n_samples)
    total = int(first[-1])
    out = torch.empty(total, device="cuda", dtype=torch.float32)
    if total:
        peaks = torch.empty(len(n_samples), device="cuda", dtype=torch.float32)
        notes, ptr = note_arrays.upload(packed, n, LAYOUT)         # the one upload
        _lib.check(_lib.load().mt3_op_render_notes(*ptr, n, len(n_samples), offs.ctypes.data, first.ctypes.data,
                                                   n_samples.ctypes.data, sample_rate, 1 if normalize else 0,
                                                   out.data_ptr(), total, peaks.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream))
    return [out[int(a): int(a) + int(c)] for a, c in zip(first, n_samples)]


def render_wav_data(ns, sample_rate: int = DEFAULT_SAMPLE_RATE) -> bytes:
    """`ns` as the bytes of a mono int16 WAV file at `sample_rate`: `render([ns], sample_rate)`, normalised to a peak of
    0.9, through `audio_io.samples_to_wav_data`"""
    from . import audio_io
    return audio_io.samples_to_wav_data(render([ns], sample_rate)[0].cpu().numpy(), _rate(sample_rate))
