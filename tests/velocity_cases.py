"""What the velocity tests share: file tables, a small hand table, and the six-note piece of the end-to-end cases."""
import numpy as np

from mt3_amd import velocity


def files(*rows):
    """FILE_DTYPE records from (first, row0, n_notes, n_pitched, n_frames) tuples"""
    table = np.zeros(len(rows), velocity.FILE_DTYPE)
    for i, r in enumerate(rows):
        table[i] = tuple(r) + (0,)
    return table


def hand_table(n_mel=4):
    """key 0: bins 0, 1, 2, 3 in that order; key 1: bin 3; key 2: bins 1, 1, 0 (a duplicate is a weighting); key 128 (the
    drums): bins 0, 2; every other row is empty"""
    rows = {0: [0, 1, 2, 3], 1: [3], 2: [1, 1, 0], 128: [0, 2]}
    lengths = [len(rows.get(k, [])) for k in range(velocity.N_KEYS)]
    first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return first, np.array([b for k in sorted(rows) for b in rows[k]], np.int32)


SIX_VELOCITIES = (20, 40, 60, 80, 100, 120)
SIX_KW = dict(gamma=1.0, anchor_velocity=60, quantile=0.4)


def six_notes(sample_rate=16000, n_samples=2 * 32768):
    """(onsets, float32 samples): six notes of pitch 60, 0.2 s long, onsets k * 0.512 s = 64 hops apart, so every onset
    sits at the same place in its frames; a plain additive synth, six partials at 1 / h, every note the same waveform
    times its gain v / 127"""
    f0 = 440.0 * 2.0 ** ((60 - 69) / 12.0)
    t = np.arange(int(0.2 * sample_rate)) / sample_rate
    tone = sum(np.sin(2 * np.pi * h * f0 * t) / h for h in range(1, 7)) * 0.25
    out = np.zeros(n_samples, np.float64)
    onsets = [k * 0.512 for k in range(len(SIX_VELOCITIES))]
    for onset, v in zip(onsets, SIX_VELOCITIES):
        a = int(round(onset * sample_rate))
        out[a: a + len(tone)] += tone * (v / 127.0)
    return onsets, out.astype(np.float32)
