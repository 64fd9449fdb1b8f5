"""The rendering rule of include/mt3_hip.h ("rendering notes to audio") as a plain float64 numpy loop: per note, per
sample of its span.  Nothing here is shared with mt3_amd/render.py or the kernel; tests/test_render_ref.py pins it by
values worked out without it.

A note is a tuple (start, end, pitch, velocity) or (start, end, pitch, velocity, is_drum); NoteSequences are taken too.
Sums are float64, so the order of the notes does not matter here (the rule fixes it for the float32 sums of the device).
"""
import math

import numpy as np

RELEASE, DRUM, ATTACK, DECAY, DRUM_DECAY = 0.04, 0.15, 0.004, 0.7, 0.03


def tuples(seq):
    if hasattr(seq, "notes"):
        return [(n.start_time, n.end_time, n.pitch, n.velocity, bool(n.is_drum)) for n in seq.notes]
    return [tuple(n) + (False,) * (5 - len(n)) for n in seq]


def sounding_instant(note):
    start, end, _, _, drum = note
    return start + DRUM if drum else end + RELEASE


def length(seq, sample_rate=16000):
    """ceil(sample_rate * latest sounding instant); 0 without notes"""
    notes = tuples(seq)
    return int(math.ceil(sample_rate * max(sounding_instant(n) for n in notes))) if notes else 0


def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def first_sounding(start, sample_rate):
    """the least n with n / sample_rate - start >= 0, by trying the integers around start * sample_rate"""
    c = max(0, int(math.floor(start * sample_rate)) - 2)
    while c / sample_rate - start < 0:
        c += 1
    return c


def partials(pitch, sample_rate):
    f0 = 440.0 * 2.0 ** ((pitch - 69) / 12)
    return [k for k in range(1, 7) if k * f0 < 0.475 * sample_rate]


def note_samples(note, sample_rate, n0, n1):
    """(first index, float64 samples) of one note inside [n0, n1): g * env * tone, or g * x for a drum note"""
    start, end, pitch, velocity, drum = note
    g = velocity / 127
    first = first_sounding(start, sample_rate)
    lo = max(n0, first)
    hi = min(n1, int(math.ceil((sounding_instant(note) + 1e-6) * sample_rate)) + 2)
    if hi <= lo or velocity == 0:
        return lo, np.zeros(0)
    n = np.arange(lo, hi, dtype=np.int64)
    t = n.astype(np.float64) / sample_rate - start
    if drum:
        on = (t >= 0) & (t < DRUM)
        u = np.array([(mix32(pitch * 2 ** 20 + int(m)) >> 8) * 2.0 ** -23 - 1.0 for m in n - first])
        return lo, np.where(on, g * u * np.exp(-t / DRUM_DECAY), 0.0)
    d = end - start
    on = (t >= 0) & (t < d + RELEASE)
    env = np.minimum(t / ATTACK, 1.0) * np.exp(-t / DECAY) * np.clip(1.0 - (t - d) / RELEASE, 0.0, 1.0)
    f0 = 440.0 * 2.0 ** ((pitch - 69) / 12)
    tone = np.zeros(len(n))
    for k in partials(pitch, sample_rate):
        turns = (k * f0) * t
        tone += np.sin(2 * np.pi * (turns - np.floor(turns))) / k
    return lo, np.where(on, g * env * tone, 0.0)


def raw(seq, sample_rate=16000, n_samples=None, window=None):
    """the un-normalised float64 samples [n0, n1) of a sequence of `n_samples` (default: `length`) samples; window =
    (n0, n1) is cut to the sequence.  Only the notes' own spans are computed."""
    notes = tuples(seq)
    n_samples = length(notes, sample_rate) if n_samples is None else int(n_samples)
    n0, n1 = (0, n_samples) if window is None else (max(0, window[0]), min(n_samples, window[1]))
    out = np.zeros(max(0, n1 - n0))
    for note in notes:
        lo, x = note_samples(note, sample_rate, n0, n1)
        out[lo - n0: lo - n0 + len(x)] += x
    return out


def peak(seq, sample_rate=16000, n_samples=None):
    """max |sample| over the whole sequence: nothing sounds outside the hull of the notes' spans"""
    notes = tuples(seq)
    n_samples = length(notes, sample_rate) if n_samples is None else int(n_samples)
    if not notes:
        return 0.0
    lo = min(first_sounding(n[0], sample_rate) for n in notes)
    x = raw(notes, sample_rate, n_samples, (lo, n_samples))
    return float(np.abs(x).max()) if len(x) else 0.0


def scale(peak_value):
    """the float32 0.9f / peak of the rule (1 for a silent sequence), as a Python float"""
    return float(np.float32(0.9) / np.float32(peak_value)) if peak_value > 0 else 1.0


def render(seq, sample_rate=16000, n_samples=None, normalize=True, window=None):
    """float64 samples of `seq` (of its window); normalised: the raw samples times the float32 scale, as the rule says"""
    x = raw(seq, sample_rate, n_samples, window)
    return x * scale(peak(seq, sample_rate, n_samples)) if normalize else x


def wav_samples(x):
    """the int16 samples audio_io.samples_to_wav_data writes for float samples x"""
    return (np.clip(x, -1, 1) * 32767.0).astype(np.int16)
