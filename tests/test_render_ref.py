"""tests/render_ref.py pinned by values worked out WITHOUT it: closed forms evaluated with `math` at single samples, the
integer mix of the drum noise done step by step (the literals below), and counts that follow from the rule's text in
include/mt3_hip.h ("rendering notes to audio").  The device tests compare against render_ref; this file is what makes
that a comparison against the rule."""
import math

import numpy as np

from tests import render_ref as ref

RATE = 16000


def _closed_form(n, pitch_hz, partials, velocity=127, rate=RATE):
    """a tonal note from t = 0, long before its release: (t / 0.004) e^(-t / 0.7) sum sin(2 pi k f t) / k, in its attack"""
    t = n / rate
    assert t < 0.004
    return (velocity / 127) * (t / 0.004) * math.exp(-t / 0.7) * sum(math.sin(2 * math.pi * k * pitch_hz * t) / k
                                                                      for k in partials)


def test_a4_starts_at_zero_and_follows_the_closed_form():
    x = ref.raw([(0.0, 0.3, 69, 127)], RATE)
    assert x[0] == 0.0                                              # t = 0: the attack starts at nothing
    # the first samples, from 440 Hz and its five overtones (6 * 440 < 7600): computed once with math.sin
    for n, want in ((1, 0.015019676787206216), (2, 0.04791408434524034), (3, 0.07441444311959099)):
        assert abs(want - _closed_form(n, 440.0, range(1, 7))) < 1e-15
        assert abs(x[n] - want) < 1e-12, (n, x[n], want)
    half = ref.raw([(0.0, 0.3, 69, 64)], RATE)
    assert np.allclose(half, x * (64 / 127), rtol=0, atol=1e-15)   # g = velocity / 127


def test_partials_stop_below_0_475_of_the_rate():
    assert ref.partials(108, RATE) == [1]                           # 2 * 4186.01 Hz > 7600 Hz
    assert ref.partials(69, RATE) == [1, 2, 3, 4, 5, 6]
    assert ref.partials(100, 8000) == [1]                           # 2637.02 Hz; twice that is past 3800 Hz
    assert ref.partials(88, 8000) == [1, 2]                         # 1318.51, 2637.02 | 3955.5
    assert ref.partials(60, 8000) == [1, 2, 3, 4, 5, 6]             # 6 * 261.63 = 1569.8
    f108, f100 = 440 * 2 ** (39 / 12), 440 * 2 ** (31 / 12)
    assert abs(f108 - 4186.009044809578) < 1e-9 and abs(f100 - 2637.02045530296) < 1e-9
    for n in (1, 5, 11):
        assert abs(ref.raw([(0.0, 0.3, 108, 127)], RATE)[n] - _closed_form(n, f108, [1])) < 1e-12
        assert abs(ref.raw([(0.0, 0.3, 100, 127)], 8000)[n] - _closed_form(n, f100, [1], rate=8000)) < 1e-12
        two = _closed_form(n, f100 / 2, [1, 2], rate=8000)
        assert abs(ref.raw([(0.0, 0.3, 88, 127)], 8000)[n] - two) < 1e-12


def test_the_last_sounding_sample():
    """end 0.10003 s: the note sounds for t < 0.14003 s = 2240.48 samples, so sample 2240 is the last and 2241 is silent"""
    note = [(0.0, 0.10003, 60, 127)]
    assert ref.length(note, RATE) == 2241
    x = ref.raw(note, RATE, 2300)
    assert len(x) == 2300 and x[2240] != 0.0 and abs(x[2240]) < 1e-3 and not x[2241:].any()
    release = 1 - (2240 / RATE - 0.10003) / 0.04                    # 0.03 ms before the end: 0.00075 of full level left
    assert abs(release - 0.00075) < 1e-9
    t = 2240 / RATE
    tone = sum(math.sin(2 * math.pi * k * 440 * 2 ** (-9 / 12) * t) / k for k in range(1, 7))
    assert abs(x[2240] - math.exp(-t / 0.7) * release * tone) < 1e-12
    # the same note half a sample later: every index moves by one where the shifted time crosses a sample
    y = ref.raw([(0.5 / RATE, 0.10003 + 0.5 / RATE, 60, 127)], RATE, 2300)
    assert y[0] == 0.0 and y[1] != 0.0 and y[2240] != 0.0 and not y[2241:].any()


def test_a_zero_length_note_is_a_blip():
    x = ref.raw([(0.5, 0.5, 69, 127)], RATE, 12000)
    on = np.flatnonzero(x)
    assert 8000 < on[0] <= 8002 and on[-1] < 8000 + 640             # inside the 40 ms release, nothing else
    assert 500 < len(on) < 640 and np.abs(x).max() > 0.3
    assert ref.length([(0.5, 0.5, 69, 127)], RATE) == 8640


def test_drum_noise_from_the_integer_mix():
    """pitch 38, m = 0 .. 3: h(38 * 2^20 + m) = f55daa69, 1d7d0ff7, 8ed26003, 7f5e9a56 (worked through the five steps of
    the mix); >> 8 and * 2^-23 - 1 give the u below"""
    assert [ref.mix32(38 * 2 ** 20 + m) for m in range(4)] == [0xF55DAA69, 0x1D7D0FF7, 0x8ED26003, 0x7F5E9A56]
    u = [16080298 * 2.0 ** -23 - 1, 1932559 * 2.0 ** -23 - 1, 9359968 * 2.0 ** -23 - 1, 8347290 * 2.0 ** -23 - 1]
    assert u[0] == 0.9169209003448486 and u[3] == -0.00492548942565918
    x = ref.raw([(0.0, 5.0, 38, 127, True)], RATE)
    assert len(x) == 2400 and x[2399] != 0.0                         # 0.15 s whatever the end
    for m in range(4):
        assert abs(x[m] - u[m] * math.exp(-(m / RATE) / 0.03)) < 1e-15
    # m counts from the note's first sounding sample, not from the sequence's: the same noise one second later
    late = ref.raw([(1.0, 1.0, 38, 127, True)], RATE)
    assert np.allclose(late[16000:16000 + 2400], x, rtol=0, atol=1e-12) and not late[:16000].any()
    off_grid = ref.raw([(1.00001, 1.0, 38, 127, True)], RATE)        # first sounding sample 16001, t = 0.0000525 s there
    assert off_grid[16000] == 0.0
    assert abs(off_grid[16001] - u[0] * math.exp(-(16001 / RATE - 1.00001) / 0.03)) < 1e-12


def test_velocity_zero_is_silent():
    assert not ref.raw([(0.0, 0.3, 69, 0), (0.1, 0.2, 38, 0, True)], RATE).any()
    assert not ref.render([(0.0, 0.3, 69, 0)], RATE).any()


def test_lengths():
    assert ref.length([], RATE) == 0
    assert ref.length([(1.0, 1.01, 38, 100, True)], RATE) == 18400   # start + 0.15, not end + 0.04
    assert ref.length([(1.0, 1.01, 38, 100, False)], RATE) == 16800
    assert ref.length([(1.0, 1.01, 38, 100, True), (0.0, 1.2, 60, 100)], RATE) == 19840
    assert ref.length([(0.0, 1.0, 60, 1)], 44100) == math.ceil(44100 * 1.04)
    assert ref.first_sounding(1.0, RATE) == 16000 and ref.first_sounding(1.00001, RATE) == 16001
    assert ref.first_sounding(0.0, RATE) == 0


def test_windows_are_cuts_of_the_whole():
    notes = [(0.01, 0.2, 60, 100), (0.05, 0.1, 38, 90, True), (0.15, 0.4, 72, 127)]
    whole = ref.raw(notes, RATE)
    assert len(whole) == ref.length(notes, RATE) == 7040
    for a, b in ((0, 100), (700, 2500), (3000, 9000)):
        assert np.array_equal(ref.raw(notes, RATE, None, (a, b)), whole[a:b])
    assert np.array_equal(ref.raw(notes, RATE, 1000), whole[:1000])  # a given length cuts the notes short


def test_normalising():
    notes = [(0.0, 0.3, 60, 127), (0.0, 0.3, 64, 127), (0.1, 0.3, 67, 127)]
    x, y = ref.raw(notes, RATE), ref.render(notes, RATE)
    pk = np.abs(x).max()
    assert pk == ref.peak(notes, RATE) and pk > 1.0
    assert abs(np.abs(y).max() - 0.9) < 1e-7                         # the float32 scale: 0.9 to float32 precision
    assert np.array_equal(y, x * float(np.float32(0.9) / np.float32(pk)))
    assert np.array_equal(ref.render(notes, RATE, normalize=False), x)
    silent = ref.render([(0.0, 0.3, 60, 0)], RATE)
    assert len(silent) == 5440 and not silent.any() and ref.scale(0.0) == 1.0
    assert np.array_equal(ref.wav_samples(np.array([0.9, -0.9, 0.00004, -0.00004, 2.0])), [29490, -29490, 1, -1, 32767])
