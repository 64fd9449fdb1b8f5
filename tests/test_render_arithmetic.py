"""The evaluation order mt3_amd/csrc/render.hip uses, restated in numpy -- float64 up to the fractional phase, float32
after: the phase folded to [-1/4, 1/4] turns, the degree-9 odd polynomial for sin(2 pi q), the envelope, the products and
the running sum in float32 -- against the float64 rule (tests/render_ref.py), on the six-note case and the late-note case.

It must stay within a QUARTER of the device tolerance (2^-16 on normalised output, half a step of the int16 file), so that
the device's own differences from this restatement (fused multiply-adds, its expf) have three quarters left.  If it does
not, the arithmetic changes, not the bound.  Measured: 2.3e-7 (six notes) and 2.1e-7 (late note), against 3.8e-6."""
import numpy as np

from tests import render_cases as cases
from tests import render_ref as ref

F = np.float32
QUARTER = 2.0 ** -18
SIN_COEFFS = (6.283185159611163, -41.341654929343406, 81.60099819260891, -76.54965682052698, 39.53581371073427)


def sin_turns(p):
    r = (p - np.rint(p)).astype(F)
    q = np.where(np.abs(r) > F(0.25), np.copysign(F(0.5), r) - r, r).astype(F)
    z = q * q
    y = F(SIN_COEFFS[4])
    for c in SIN_COEFFS[3::-1]:
        y = (z * y + F(c)).astype(F)
    return (y * q).astype(F)


def restated(notes, sample_rate, n_samples, window):
    """float32 samples of [n0, n1), un-normalised, the notes in the rule's order"""
    n0, n1 = window
    n = np.arange(n0, n1, dtype=np.int64)
    T = n.astype(np.float64) / sample_rate
    acc = np.zeros(len(n), F)
    for start, end, pitch, velocity, drum in sorted(ref.tuples(notes)):
        assert not drum
        g = F(velocity) / F(127)
        t = T - start
        d = end - start
        on = (t >= 0) & (t < d + 0.04)
        tf, past = t.astype(F), (t - d).astype(F)
        env = np.minimum(tf * F(250), F(1)) * np.exp(tf * F(-1 / 0.7)).astype(F) \
            * np.minimum(np.maximum(F(1) - past * F(25), F(0)), F(1))
        f0 = 440.0 * 2.0 ** ((pitch - 69) / 12)
        tone = np.zeros(len(n), F)
        for k in ref.partials(pitch, sample_rate):
            turns = (k * f0) * t
            tone = (tone + sin_turns((turns - np.floor(turns)).astype(F)) * (F(1) / F(k))).astype(F)
        acc = np.where(on, (acc + (g * env.astype(F)) * tone).astype(F), acc)
    assert acc.dtype == F
    return acc


def _worst(notes, n_samples, window):
    raw32 = restated(notes, cases.RATE, n_samples, window)
    want = ref.render(notes, cases.RATE, n_samples, True, window)
    pk = F(np.abs(restated(notes, cases.RATE, n_samples, (0, n_samples) if n_samples < 10 ** 6 else window)).max())
    got = raw32 * (F(0.9) / pk)
    assert got.dtype == F and np.abs(want).max() > 0.89
    return float(np.abs(got.astype(np.float64) - want).max())


def test_sine_polynomial_alone():
    p = np.linspace(0.0, 1.0, 200001).astype(F)
    err = np.abs(sin_turns(p).astype(np.float64) - np.sin(2 * np.pi * p.astype(np.float64))).max()
    print("sine polynomial, float32 Horner: max error %.3g" % err)
    assert err < 4e-7


def test_six_notes_within_a_quarter_of_the_bound():
    n = ref.length(cases.SIX, cases.RATE)
    worst = _worst(cases.SIX, n, (0, n))
    print("six notes: max |float32 restatement - rule| = %.3g (quarter bound %.3g)" % (worst, QUARTER))
    assert worst <= QUARTER


def test_late_note_within_a_quarter_of_the_bound():
    worst = _worst(cases.LATE, cases.LATE_SAMPLES, cases.LATE_WINDOW)
    print("late note: max |float32 restatement - rule| = %.3g (quarter bound %.3g)" % (worst, QUARTER))
    assert worst <= QUARTER
