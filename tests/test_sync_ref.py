"""The numpy rules of mt3_amd/sync.py against independent statements, and the end-to-end case on the CPU rule that fixes
the synchronisation's constants.  No GPU."""
import itertools

import numpy as np
import pytest

from mt3_amd import note_sequences as N
from mt3_amd import sync
from oracle import frontend as F
from tests import sync_cases as SC


def brute_force(a, s):
    """full-matrix DTW, every predecessor listed with its rank in the rule's order: (value, rank) pairs compared as tuples"""
    a, s = a.astype(int), s.astype(int)
    n, m = len(a), len(s)
    D, back = {}, {}
    for i, j in itertools.product(range(n), range(m)):
        cost = sum(abs(int(x) - int(y)) for x, y in zip(a[i], s[j]))
        options = [(D[q], rank, q) for rank, q in enumerate(((i - 1, j - 1), (i - 1, j), (i, j - 1))) if q in D]
        if not options:
            D[i, j] = cost
            continue
        value, _, q = min(options)                                      # the lowest value, then the lowest rank
        D[i, j], back[i, j] = cost + value, q
    cell, path = (n - 1, m - 1), []
    while True:
        path.append(cell)
        if cell == (0, 0):
            break
        cell = back[cell]
    path.reverse()
    return np.array([c[0] for c in path]), np.array([c[1] for c in path]), D[n - 1, m - 1]


@pytest.mark.parametrize("kind", ["random", "zeros", "extremes", "coarse"])
def test_paths_reference_is_the_brute_force(kind):
    rng = np.random.default_rng(5)
    for n, m in [(1, 1), (1, 7), (7, 1), (2, 2), (3, 12), (12, 3), (12, 12), (9, 11)]:
        if kind == "coarse":                                             # few levels: many equal sums
            a, s = rng.integers(0, 3, (n, 12)).astype(np.uint8), rng.integers(0, 3, (m, 12)).astype(np.uint8)
        else:
            a, s = SC.features(rng, n, kind), SC.features(rng, m, kind)
        pi, pj, total = sync.paths_reference(a, s)
        bi, bj, btotal = brute_force(a, s)
        assert total == btotal and np.array_equal(pi, bi) and np.array_equal(pj, bj), (kind, n, m)
        fi, fj, ftotal = SC.fast_paths(a, s)
        assert ftotal == total and np.array_equal(fi, pi) and np.array_equal(fj, pj), (kind, n, m)
        steps = set(zip(np.diff(pi).tolist(), np.diff(pj).tolist()))
        assert (pi[0], pj[0]) == (0, 0) and (pi[-1], pj[-1]) == (n - 1, m - 1) and steps <= {(1, 1), (1, 0), (0, 1)}
        assert len(pi) <= n + m - 1
    assert sync.paths_reference(np.zeros((0, 12)), np.zeros((3, 12)))[2] == 0
    assert len(sync.paths_reference(np.zeros((3, 12)), np.zeros((0, 12)))[0]) == 0


def test_all_zero_features_walk_the_diagonal_first():
    pi, pj, total = sync.paths_reference(np.zeros((3, 12), np.uint8), np.zeros((5, 12), np.uint8))
    assert total == 0 and pi.tolist() == [0, 0, 0, 1, 2] and pj.tolist() == [0, 1, 2, 3, 4]


def test_a_sequence_against_its_copy_is_the_diagonal():
    a = SC.features(np.random.default_rng(2), 40)
    pi, pj, total = sync.paths_reference(a, a.copy())
    assert total == 0 and np.array_equal(pi, np.arange(40)) and np.array_equal(pj, np.arange(40))


def test_note_chroma_reference_is_a_loop_over_frames_and_notes():
    rng = np.random.default_rng(3)
    n = 60
    j0 = rng.integers(0, 30, n).astype(np.int32)
    j1 = (j0 + rng.integers(1, 12, n)).astype(np.int32)
    pitch = rng.integers(0, 128, n).astype(np.int32)
    pitch[:25] = 60                                                      # one class stacked: the clip
    files = sync.file_table([0, 0], [40, 20], [int(j1[:40].max()), int(j1[40:].max())], 5)
    for weights in ((255,), (255, 128, 64, 32, 16, 8), (7, 0, 3)):
        got = sync.note_chroma_reference(j0, j1, pitch, files, weights)
        want = np.zeros_like(got, dtype=np.int64)
        for f in files:
            for j in range(int(f["m"])):
                for i in range(int(f["first"]), int(f["first"]) + int(f["n_notes"])):
                    if j0[i] <= j < j1[i]:
                        for h, w in enumerate(weights):
                            want[int(f["s0"]) + j, (int(pitch[i]) + sync.OFFSETS[h]) % 12] += w
        assert np.array_equal(got, np.minimum(want, 255)) and (want.max() > 255) == (weights[0] == 255)


def test_note_frames_and_the_score_length():
    j0, j1 = sync.note_frames([0.0, 0.039, 0.04, 1.0, 2.0], [0.0, 0.04, 0.041, 1.2, 2.01], 25.0)
    assert j0.tolist() == [0, 0, 1, 25, 50] and j1.tolist() == [1, 1, 2, 30, 51]
    ns = N.NoteSequence(notes=[N.Note(1.0, 1.2, 60, 90), N.Note(0.5, 0.5, 36, 90, is_drum=True)])
    packed = sync.pack([ns, N.NoteSequence()], [100, 7], [256, 256], 5, 25.0)
    assert packed.n_notes == 1 and packed.files["m"].tolist() == [30, 0] and packed.files["n"].tolist() == [20, 2]
    assert packed.files["row0"].tolist() == [0, 256] and packed.files["path0"].tolist() == [0, 49]


def test_chroma_bins_and_the_audio_rule_find_every_pure_tone():
    bins = sync.chroma_bins(F.mel_weight_matrix_tf32())
    assert bins.dtype == np.int8 and bins.shape == (512,) and set(np.unique(bins)) == set(range(-1, 12))
    t = np.arange(int(0.6 * 16000)) / 16000.0
    for pitch in range(60, 97):
        f0 = 440.0 * 2.0 ** ((pitch - 69) / 12.0)
        wav = np.concatenate([np.zeros(3200), 0.5 * np.sin(2 * np.pi * f0 * t), np.zeros(3200)]).astype(np.float32)
        logmel = F.compute_logmel(wav, np.float32, "tf32")
        files = sync.file_table([len(logmel)], [0], [0], 5)
        q = sync.logmel_chroma_reference(logmel, files, bins)
        inside = q[int(0.2 * 25) + 4: int(0.8 * 25) - 4]                 # frames whose whole window lies in the tone
        assert len(inside) >= 5 and (inside.argmax(1) == pitch % 12).all() and (inside.max(1) == 255).all(), pitch
        assert not q[:1].any()                                           # digital silence: a silent frame


def test_the_audio_rule_on_edge_values():
    bins = np.array([0, 0, 5, -1, 11, 12, 5, 3], np.int8)                # 12 and -1: unused
    lm = np.full((7, 8), -np.inf, np.float32)
    lm[0] = [1.0, 2.0, np.nan, 9.0, -1.0, 9.0, -2.0, 2.0]
    lm[1] = np.nan
    lm[5] = 3.0
    files = sync.file_table([7], [0], [0], 1)
    q = sync.logmel_chroma_reference(lm, files, bins, 1, 4.0, 0.0)
    assert q[0].tolist() == [255, 0, 0, 255, 0, 0, 0, 0, 0, 0, 0, 63]    # floor((-1 - 2 + 4) * 63.75) = 63; class 5: -2 - 2 + 4 = 0
    assert not q[1].any() and not q[2].any()                             # nothing measured; all -inf: below the floor
    assert q[5].tolist() == [255, 0, 0, 255, 0, 255, 0, 0, 0, 0, 0, 255]
    pooled = sync.logmel_chroma_reference(lm, sync.file_table([7], [0], [0], 5), bins, 5, 4.0, 0.0)
    assert len(pooled) == 2 and pooled[0, 0] == 255 and pooled[1].tolist() == q[5].tolist()


def test_warp_times_is_the_identity_on_the_diagonal_and_monotone_on_any_path():
    d = np.arange(50)
    t = np.linspace(-1.0, 4.0, 101)
    assert np.allclose(sync.warp_times(t, d, d, 25.0), t, rtol=0, atol=1e-12)
    rng = np.random.default_rng(4)
    for _ in range(20):
        steps = rng.integers(0, 3, 200)
        pi = np.concatenate([[0], np.cumsum(steps != 2)])
        pj = np.concatenate([[0], np.cumsum(steps != 1)])
        out = sync.warp_times(np.sort(rng.uniform(-2.0, 12.0, 300)), pi, pj, 25.0)
        assert (np.diff(out) >= 0).all()
    ns = N.NoteSequence(notes=[N.Note(0.5, 1.0, 60, 90, 3, False, 2)], ticks_per_quarter=480,
                        control_changes=[N.ControlChange(0.75, 64, 127, 2)])
    moved = sync.warp_notes(ns, d * 2, d, 25.0)                          # every score frame takes two audio frames
    note, cc = moved.notes[0], moved.control_changes[0]
    assert (note.pitch, note.velocity, note.program, note.instrument) == (60, 90, 3, 2) and moved.ticks_per_quarter == 480
    assert note.start_time < cc.time < note.end_time and abs(note.end_time - note.start_time - 1.0) < 1e-9
    assert (cc.control_number, cc.control_value, cc.instrument) == (64, 127, 2)


def test_end_to_end_on_the_numpy_rule_fixes_the_constants():
    """A 16 s synth_music-style piece (random_music seed 7), performed under a smooth tempo curve between 0.8x and 1.25x
    after a 0.5 s lead-in and rendered by synthetic.render_notes; the UNWARPED score synchronised to that audio by the
    numpy rules on the oracle's float32 log-mel, default constants (pool 5, range 4.0, floor 0.0, fmin 250, fmax 4400,
    harmonic_weights (255,)).  Measured 2026-10-21: maximum onset error 0.2544 s, median 0.0508 s (sync_cases.py holds
    the two figures; the bound is the maximum plus one feature frame, 0.04 s)."""
    score, played, wav = SC.piece()
    assert 15.0 < score.total_time <= 16.0 and len(score.notes) > 50
    ratio = np.diff(SC.performed(np.linspace(0, 16, 200))) / np.diff(np.linspace(0, 16, 200))
    assert 0.79 < ratio.min() < 0.82 and 1.22 < ratio.max() < 1.26
    logmel = F.compute_logmel(wav.astype(np.float32), np.float32, "tf32")
    rec = SC.numpy_synchronize(logmel, score, sync.chroma_bins(F.mel_weight_matrix_tf32()))
    err = SC.onset_errors(rec["notes"], played)
    print("onset error: max %.4f s, median %.4f s; mean cost %.1f, tempo ratio %.3f"
          % (err.max(), np.median(err), rec["mean_cost"], rec["tempo_ratio"]))
    assert err.max() <= SC.MEASURED_MAX <= err.max() + 1e-4 and abs(np.median(err) - SC.MEASURED_MEDIAN) < 1e-4
    assert err.max() <= SC.BOUND
    unsynced = SC.onset_errors(score, played)
    assert unsynced.max() > 0.5 and np.median(err) < 0.5 * np.median(unsynced)      # it is the synchronisation that does it
    assert all(b.end_time >= b.start_time for b in rec["notes"].notes)
    assert 0.9 < rec["tempo_ratio"] < 1.1 and rec["mean_cost"] == rec["total"] / len(rec["path"][0])
