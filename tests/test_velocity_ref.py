"""The velocity rule in numpy (mt3_amd/velocity.py: levels_reference, velocities_reference, harmonic_bins) on arrays whose
answers are worked out by hand, and end to end on the oracle's log-mel of six notes of known gain."""
import math

import numpy as np
import pytest

from mt3_amd import velocity
from oracle import frontend
from tests import velocity_cases as cases

NAN = float("nan")


def levels(logmel, table, frame, key, window=8, n_frames=None):
    logmel = np.asarray(logmel, np.float32)
    n = len(logmel) if n_frames is None else n_frames
    return velocity.levels_reference(logmel, cases.files((0, 0, len(frame), len(frame), n)), np.array(frame, np.int32),
                                     np.array(key, np.int32), *table, window=window)


def test_the_sum_runs_left_to_right_in_float64():
    big = 2.0 ** 60                                  # a float32 value
    logmel = [[big, 1.0, -big, 1.0], [0.5, 0.25, 0.125, 8.0], [-1.0, -2.0, -3.0, -4.0]]
    left_to_right, pairwise = ((big + 1.0) + -big) + 1.0, (big + 1.0) + (-big + 1.0)
    assert left_to_right == 1.0 and pairwise == 0.0
    got = levels(logmel, cases.hand_table(), [0, 0, 1, 2, 0], [0, 1, 0, 0, 2], window=1)
    assert got.tolist() == [0.25, 1.0, 8.875 / 4, -2.5, (1.0 + 1.0 + big) / 3]
    # the max over the window: frame 0's 0.25, frame 1's 2.21875, frame 2's -2.5
    assert levels(logmel, cases.hand_table(), [0, 1, 2], [0, 0, 0], window=2).tolist() == [8.875 / 4, 8.875 / 4, -2.5]
    assert got.dtype == np.float64


def test_the_window_is_cut_to_the_files_frames():
    logmel = np.arange(10, dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)       # frame g holds g in every bin
    logmel[7:] = 1e30                                 # rows past n_frames = 7: never read
    table = cases.hand_table()
    got = levels(logmel, table, [0, 3, 5, 6, 7, -1, -3, 2 ** 31 - 1], [1] * 8, window=3, n_frames=7)
    assert np.array_equal(got, [2.0, 5.0, 6.0, 6.0, NAN, NAN, NAN, NAN], equal_nan=True)
    # two files back to back: the second file's frame 0 is row 7, and the first never reads it
    two = cases.files((0, 0, 1, 1, 7), (1, 7, 2, 2, 3))
    logmel[7:] = [[100.0] * 4, [50.0] * 4, [25.0] * 4]
    got = velocity.levels_reference(logmel, two, np.array([6, 0, 2], np.int32), np.array([1, 1, 1], np.int32), *table,
                                    window=8)
    assert got.tolist() == [6.0, 100.0, 25.0]
    # an empty bin row, and a key outside the table
    assert np.isnan(levels(logmel, table, [0, 0, 0], [3, 129, -1])).all()
    assert levels(logmel, table, [1], [128], window=1).tolist() == [1.0]


def test_nan_frames_are_skipped():
    logmel = np.zeros((5, 4), np.float32)
    logmel[:, 3] = [1.0, NAN, 3.0, NAN, NAN]
    logmel[2, 0] = NAN                               # key 0 sums bin 0 too: frame 2 is NaN for it, not for key 1
    table = cases.hand_table()
    assert np.array_equal(levels(logmel, table, [0, 1, 3], [1, 1, 1], window=3), [3.0, 3.0, NAN], equal_nan=True)
    assert np.array_equal(levels(logmel, table, [0, 2], [0, 0], window=3), [0.25, NAN], equal_nan=True)
    logmel[0, 3], logmel[0, 0] = np.inf, -np.inf      # inf - inf inside a sum is a NaN frame as well
    assert np.array_equal(levels(logmel, table, [0], [0], window=1), [NAN], equal_nan=True)


def velocities(level, quantile=0.5, th=None, n_pitched=None, velocity_in=None):
    level = np.asarray(level, np.float64)
    n = len(level)
    th = velocity.thresholds() if th is None else th
    table = cases.files((0, 0, n, n if n_pitched is None else n_pitched, 1))
    return velocity.velocities_reference(level, np.full(n, 100) if velocity_in is None else velocity_in, table, th,
                                         quantile)


def test_the_anchor_is_the_member_at_the_quantile_rank():
    for level, quantile, want in [([3.0], 0.5, 3.0), ([3.0], 1.0, 3.0), ([5.0, 3.0], 0.5, 3.0), ([5.0, 3.0], 1.0, 5.0),
                                  ([5.0, 3.0], 0.99, 3.0), ([9.0, 1.0, 7.0, 3.0, 5.0], 0.5, 5.0),
                                  ([9.0, 1.0, 7.0, 3.0, 5.0], 0.0, 1.0), ([9.0, 1.0, 7.0, 3.0, 5.0], 0.74, 5.0),
                                  ([9.0, 1.0, 7.0, 3.0, 5.0], 0.75, 7.0), ([9.0, 1.0, 7.0, 3.0, 5.0], 1.0, 9.0),
                                  ([-2.0, 2.0, -1.0, NAN, 1.0], 0.5, -1.0), ([4.0] * 5, 0.3, 4.0)]:
        _, anchor, measured = velocities(level, quantile)
        assert anchor[0, 0] == want and measured[0, 0] == np.sum(~np.isnan(level)), (level, quantile)
        assert np.isnan(anchor[0, 1]) and measured[0, 1] == 0
    # all levels equal: d = 0 for every note, and 0 >= th[v] exactly for v - 0.5 <= 80
    got, _, _ = velocities([4.0] * 5)
    assert got.tolist() == [80] * 5
    # the drums are ranked on their own; an unmeasured note keeps what it came with
    got, anchor, measured = velocities([1.0, 2.0, 3.0, 10.0, NAN, 30.0], n_pitched=3, velocity_in=[11, 12, 13, 14, 15, 16])
    assert anchor.tolist() == [[2.0, 10.0]] and measured.tolist() == [[3, 2]]
    assert got[1] == 80 and got[3] == 80 and got[4] == 15 and got[5] == 127 and got[0] < 80 < got[2]
    got, anchor, measured = velocities([NAN, NAN], velocity_in=[7, 9])
    assert got.tolist() == [7, 9] and np.isnan(anchor).all() and measured.tolist() == [[0, 0]]


def test_a_threshold_is_reached_exactly_at_its_value():
    th = velocity.thresholds(2.0, 80)
    assert th.shape == (126,) and th.dtype == np.float64 and (np.diff(th) > 0).all()
    assert th[0] == 2.0 * math.log(1.5 / 80) and th[125] == 2.0 * math.log(126.5 / 80)
    for v in (2, 50, 81, 127):
        at = th[v - 2]
        # anchor 0.0 (the lowest of two with quantile 0): d is the level itself
        got, _, _ = velocities([0.0, at, np.nextafter(at, -np.inf)], quantile=0.0 if at > 0 else 1.0)
        assert got.tolist()[1:] == [v, v - 1], v
    assert velocities([0.0, -1e9], quantile=1.0)[0].tolist() == [80, 1]
    assert velocities([0.0, 1e9], quantile=0.0)[0].tolist() == [80, 127]
    assert velocities([np.inf, np.inf])[0].tolist() == [1, 1]           # inf - inf: no threshold is reached
    for bad in (dict(gamma=0.0), dict(gamma=NAN), dict(anchor_velocity=0), dict(anchor_velocity=float("inf"))):
        with pytest.raises(ValueError):
            velocity.thresholds(**bad)


@pytest.fixture(scope="module")
def mel():
    return frontend.mel_weight_matrix_tf32()


def test_harmonic_bins_on_the_oracles_mel_matrix(mel):
    first, bins = velocity.harmonic_bins(mel)
    assert first.dtype == bins.dtype == np.int32 and first.shape == (130,) and first[0] == 0 and first[-1] == len(bins)
    assert (mel[:, bins] != 0).any(0).all()                             # no listed bin is an empty mel column
    # pitch 127: 12543.85 Hz, FFT bin 1606 and up: past fft_size / 2, every harmonic is dropped
    assert first[128] - first[127] == 0
    # pitch 0: 8.18 Hz; harmonics 1 and 2 fall on FFT bins 1 and 2 (7.8 and 15.6 Hz), below the mel matrix's 20 Hz: their
    # rows are all zero and are dropped; harmonics 3 .. 6 fall on bins 3, 4, 5, 6
    assert not mel[1].any() and not mel[2].any()
    assert bins[first[0]: first[1]].tolist() == [int(np.argmax(mel[k])) for k in (3, 4, 5, 6)]
    # pitch 69: 440 Hz * h -> FFT bins 56, 113, 169, 225, 282, 338
    assert bins[first[69]: first[70]].tolist() == [int(np.argmax(mel[k])) for k in (56, 113, 169, 225, 282, 338)]
    assert first[70] - first[69] == 6 and (np.diff(first)[:128] <= 6).all()
    # low pitches: several harmonics share a mel bin, and the duplicates stay
    row = bins[first[0]: first[1]].tolist()
    assert velocity.harmonic_bins(mel, harmonics=12)[0][1] >= len(row)
    assert bins[first[128]:].tolist() == list(range(0, 512, 8)) and first[129] - first[128] == 64
    # the largest weight, the lowest index on a tie
    w = np.zeros((1025, 8), np.float32)
    w[56, 2] = w[56, 5] = 0.5
    w[56, 1] = 0.25
    f, b = velocity.harmonic_bins(w, harmonics=1)
    assert b[f[69]: f[70]].tolist() == [2] and b[f[128]:].tolist() == [0]
    with pytest.raises(ValueError):
        velocity.harmonic_bins(mel[:-1])


def test_six_notes_of_known_gain_come_back_exactly(mel):
    """levels differ by ln of the gain ratio up to float32 rounding (~1e-6); the nearest threshold is ln(120.5 / 120) ~
    4e-3 away"""
    onsets, samples = cases.six_notes()
    logmel = frontend.compute_logmel_tf32(samples)
    assert logmel.dtype == np.float32 and logmel.shape == (512, 512)
    table = velocity.harmonic_bins(mel)
    frame = velocity.frames_of(onsets, 125.0)
    assert frame.tolist() == [0, 64, 128, 192, 256, 320]
    one = cases.files((0, 0, 6, 6, len(logmel)))
    level = velocity.levels_reference(logmel, one, frame, np.full(6, 60, np.int32), *table, window=8)
    gains = np.log(np.array(cases.SIX_VELOCITIES) / 60.0)
    print("level - level[2] - ln(v / 60):", (level - level[2] - gains).tolist())
    assert np.abs(level - level[2] - gains).max() < 1e-4
    th = velocity.thresholds(cases.SIX_KW["gamma"], cases.SIX_KW["anchor_velocity"])
    got, anchor, measured = velocity.velocities_reference(level, np.full(6, 100), one, th, cases.SIX_KW["quantile"])
    assert anchor[0, 0] == level[2] and measured.tolist() == [[6, 0]]
    assert got.tolist() == list(cases.SIX_VELOCITIES)
