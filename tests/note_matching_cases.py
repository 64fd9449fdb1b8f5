"""Shared generators for the note-matching tests: the cases of tests/test_note_matching_ref.py (host only) and
tests/test_gpu_note_matching.py (device against host).  A case is (ref_intervals [n, 2], ref_pitches [n], est_intervals,
est_pitches) plus, where it matters, the rule's keyword arguments for `metrics.match_notes`."""
import numpy as np

ONSET_ONLY = dict(offset_ratio=None)
DEFAULT = dict()
SWEEP_WIDE = dict(onset_tolerance=0.5, offset_min_tolerance=0.5)
SWEEP_NARROW = dict(onset_tolerance=0.01, offset_min_tolerance=0.01)
RULES = (ONSET_ONLY, DEFAULT, SWEEP_WIDE, SWEEP_NARROW)


def hz(note_numbers):
    return 440.0 * 2.0 ** ((np.asarray(note_numbers, np.float64) - 69.0) / 12.0)


def dense(rng, n, span, jitter, pitches):
    """sorted random reference notes over `span` seconds on note numbers 60 .. 60 + pitches; the estimates are the
    references with 15 % dropped, onsets and offsets jittered (normal, sd `jitter`), and 15 % random notes added"""
    on = np.sort(rng.uniform(0.0, span, n))
    ref_iv = np.stack([on, on + rng.uniform(0.05, 0.6, n)], axis=1)
    ref_p = rng.integers(60, 60 + pitches + 1, n).astype(np.float64)
    keep = rng.random(n) >= 0.15
    est_iv = ref_iv[keep] + rng.normal(0.0, jitter, (int(keep.sum()), 2))
    est_iv[:, 0] = np.maximum(est_iv[:, 0], 0.0)
    est_iv[:, 1] = np.maximum(est_iv[:, 1], est_iv[:, 0] + 0.01)
    est_p = ref_p[keep]
    extra = int(round(0.15 * n))
    x_on = rng.uniform(0.0, span, extra)
    est_iv = np.concatenate([est_iv, np.stack([x_on, x_on + rng.uniform(0.05, 0.6, extra)], axis=1)])
    est_p = np.concatenate([est_p, rng.integers(60, 60 + pitches + 1, extra).astype(np.float64)])
    shuffle = rng.permutation(len(est_p))                  # the caller's order is not the onset order
    return ref_iv, ref_p, est_iv[shuffle], est_p[shuffle]


def dense_draws(n, draws, seed=0, span=None):
    """`draws` dense cases of n notes at the density of n = 200 over 6 s, jitter 0.03, 4 pitches"""
    rng = np.random.default_rng([seed, n])
    return [dense(rng, n, 6.0 * n / 200 if span is None else span, 0.03, 4) for _ in range(draws)]


CHAIN_RULE = dict(onset_tolerance=0.05, offset_ratio=None)


def chain(L, moved=False):
    """One pitch, onset-only rule, tolerance 0.05.  References r_k at 0.1 k, estimates e_k at 0.1 k + 0.05: every distance
    |r_k - e_k| and |r_k - e_{k-1}| is 0.05 up to float noise, which the 6-decimal rounding makes an edge, so the graph is
    the path r_0 - e_0 - r_1 - e_1 - ... - r_{L-1} - e_{L-1} and nothing else (tests/test_note_matching_ref.py pins that
    with the dense predicate).  -> (ref_iv, ref_p, est_iv, est_p, warm) with warm[k] = k - 1: every r_k, k >= 1, matched
    to e_{k-1}, r_0 and e_{L-1} free.  The maximum L is reachable from the warm start only along ONE augmenting path,
    through all 2 L vertices.
    moved=True puts the last reference at 0.1 (L - 1) + 0.02.  The dense predicate says that this takes the edge
    r_{L-1} - e_{L-2} away (distance 0.07), so the warm start's last entry is then not an edge and the long path ends at
    e_{L-2}, through 2 L - 2 vertices, beside the one-edge path r_{L-1} - e_{L-1}; the maximum is still L.  Both forms are
    tested; the unmoved one is the one with the single full-length path."""
    k = np.arange(L, dtype=np.float64)
    r_on = 0.1 * k
    if moved:
        r_on[L - 1] = 0.1 * (L - 1) + 0.02
    e_on = 0.1 * k + 0.05
    ref_iv = np.stack([r_on, r_on + 0.5], axis=1)
    est_iv = np.stack([e_on, e_on + 0.5], axis=1)
    pitch = np.full(L, 60.0)
    warm = np.arange(L, dtype=np.int64) - 1
    return ref_iv, pitch, est_iv, pitch.copy(), warm


# the literals of tests/test_io_and_metrics.py::test_mir_eval_boundary_comparisons:
# (reference (on, off, pitch), estimate (on, off, pitch), rule, expected matches)
_HZ = 440.0
BOUNDARY = [
    ((1.0, 2.0, _HZ), (1.05, 2.0, _HZ), dict(offset_ratio=None), 1),
    ((1.0, 2.0, _HZ), (1.05, 2.0, _HZ), dict(offset_ratio=None, strict=True), 0),
    ((1.0, 2.0, _HZ), (1.0500004, 2.0, _HZ), dict(offset_ratio=None), 1),
    ((1.0, 2.0, _HZ), (1.050001, 2.0, _HZ), dict(offset_ratio=None), 0),
    ((1.0, 2.0, _HZ), (0.95, 2.0, _HZ), dict(offset_ratio=None), 1),
    ((0.0, 2.0, _HZ), (0.0, 2.4, _HZ), dict(), 1),
    ((0.0, 2.0, _HZ), (0.0, 2.400001, _HZ), dict(), 0),
    ((0.0, 2.0, _HZ), (0.0, 1.6, _HZ), dict(), 1),
    ((0.0, 2.0, _HZ), (0.0, 2.4, _HZ), dict(strict=True), 0),
    ((0.0, 0.1, _HZ), (0.0, 0.15, _HZ), dict(), 1),
    ((0.0, 0.1, _HZ), (0.0, 0.151, _HZ), dict(), 0),
    ((0.0, 2.0, _HZ), (0.0, 2.3, _HZ), dict(offset_ratio=0.1), 0),
    ((0.0, 0.2, _HZ), (0.0, 1.0, _HZ), dict(), 0),
    ((0.0, 0.2, _HZ), (0.0, 1.0, _HZ), dict(offset_ratio=None), 1),
    ((0.0, 1.0, _HZ), (0.0, 1.0, _HZ * 2 ** (50 / 1200)), dict(offset_ratio=None), 1),
    ((0.0, 1.0, _HZ), (0.0, 1.0, _HZ * 2 ** (51 / 1200)), dict(offset_ratio=None), 0),
]


def boundary_cases():
    """-> [(ref_iv, ref_p, est_iv, est_p, rule, expected)]"""
    one = lambda note: (np.array([[note[0], note[1]]], np.float64), np.array([note[2]], np.float64))     # noqa: E731
    return [one(r) + one(e) + (rule, expected) for r, e, rule, expected in BOUNDARY]


def zero_length_cases():
    """problems in which a side holds ONLY zero-length notes (onset == offset).  For the matcher these are notes like
    any other -- the offset tolerance of a zero-length reference is max(0.2 * 0, 0.05) -- it is the score layer that drops
    them (`sequence_to_valued_intervals`).  -> [(ref_iv, ref_p, est_iv, est_p)]: zero-length references against real
    estimates (offsets 0.03 and 0.2 away: one inside the 0.05 floor, one outside), real references against zero-length
    estimates, and zero-length notes on both sides (two references share one estimate)"""
    point = lambda *on: np.array([[t, t] for t in on], np.float64)                                      # noqa: E731
    real_iv, real_p = np.array([[0.0, 0.03], [1.0, 1.2], [2.0, 2.5]], np.float64), np.array([60.0, 62.0, 64.0])
    zero_iv, zero_p = point(0.0, 1.0, 2.04, 3.0), np.array([60.0, 62.0, 64.0, 65.0])
    both_ref, both_est = point(0.0, 0.02, 1.0), point(0.01, 1.05, 5.0)
    return [(zero_iv, zero_p, real_iv, real_p), (real_iv, real_p, zero_iv, zero_p),
            (both_ref, np.full(3, 60.0), both_est, np.full(3, 60.0))]


def zero_length_sequences():
    """NoteSequence note lists for the score layer, where zero-length notes are dropped BEFORE n_ref and n_est are
    counted: (start, end, pitch) triples of only zero-length notes"""
    return [(0.0, 0.0, 60), (1.0, 1.0, 62), (2.5, 2.5, 64)]


def empty_cases():
    """problems with an empty side (also what the score layer is left with when a side holds only zero-length notes,
    which it drops before matching): (ref_iv, ref_p, est_iv, est_p)"""
    none_iv, none_p = np.zeros((0, 2), np.float64), np.zeros(0, np.float64)
    some_iv, some_p = np.array([[0.0, 1.0], [0.5, 1.5]], np.float64), np.array([60.0, 62.0])
    return [(none_iv, none_p, some_iv, some_p), (some_iv, some_p, none_iv, none_p), (none_iv, none_p, none_iv, none_p)]
