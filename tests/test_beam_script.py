"""The scripted cases of tests/beam_script.py are what they claim to be (no GPU): every decision is separated by GAP or
is an exact tie in a case flagged for it, the float64 mirror the cases were drawn against is the reference's own state,
and the set covers the widths, vocabularies, ties and outcomes tests/test_gpu_token_rules.py is meant to exercise.
No GPU test skips or filters a case: the share of cases left out is zero by construction."""
import numpy as np
import pytest

from tests import beam_script as bs
from tests.beam_search_ref import EOS, NEG_INF

ALL = bs.beam_cases() + bs.token_cases()


def test_no_redraw_cap_was_hit():
    for c in ALL:
        assert 1 <= c.max_tries < bs.MAX_TRIES, c.name
    assert max(c.max_tries for c in ALL) <= 12           # the ladder rows separate within a dozen draws


def test_every_gap_is_separated_or_an_exact_tie_in_a_tie_case():
    for c in ALL:
        zero = 0
        assert c.gaps, c.name
        for d, s, _ in c.gaps:
            assert d >= bs.GAP(s) or (d == 0.0 and c.tie), (c.name, d, s)
            zero += d == 0.0
        assert (zero > 0) == c.tie, c.name               # a tie case holds ties, no other case does


def test_mirror_is_the_reference():
    """The scores the cases were drawn against are bit for bit those of beam_search: live log-probs after every step,
    the retirement step, and the finished set at the end (with max_len: the rows past it changed no finished set)."""
    for c in ALL:
        r = c.ref
        for t in range(r.steps_run):
            for b in range(c.elems):
                if not np.isnan(c.mirror_live[t, b, 0]):
                    assert np.array_equal(c.mirror_live[t, b], r.live_lp[t][b]), (c.name, t, b)
        for b in range(c.elems):
            if c.retired_at[b] >= 0:
                assert r.retired[c.retired_at[b]][b] and not (c.retired_at[b] and r.retired[c.retired_at[b] - 1][b]), c.name
            if c.n_fin[b]:
                want = [NEG_INF] * (c.k - c.n_fin[b]) + sorted(c.mirror_fin[b])
                assert np.array_equal(r.scores[b], np.array(want)), (c.name, b)
            else:
                assert (r.scores[b] > NEG_INF / 2).all(), (c.name, b)       # its live beams


def test_every_width_sees_eos_forks_and_retirement():
    cases = bs.beam_cases()
    for k in range(1, 9):
        mine = [c for c in cases if c.k == k]
        assert sum(c.n_eos.sum() for c in mine) > 0
        assert sum((c.retired_at >= 0).sum() for c in mine) > 0
        # one beam never forks (k - #parents = 0); every other width does
        assert (sum(c.forks.sum() for c in mine) > 0) == (k > 1)
        fin = np.concatenate([c.n_fin for c in mine])
        assert (fin == 0).any() and (fin == k).any()
        if k > 1:
            assert ((fin > 0) & (fin < k)).any(), k


def test_the_shapes_of_the_issue_are_covered():
    cases = bs.beam_cases()
    seen = {(c.k, c.V) for c in cases}
    for k in range(1, 9):
        assert (k, 2 * k) in seen and (k, 2 * k + 1) in seen
    for V in bs.V_EDGES:
        assert len({k for k, v in seen if v == V}) >= 2, V
    assert {(8, 2048), (8, 2047), (8, 64), (5, 1536), (7, 130), (6, 12), (8, 16)} <= seen    # (the 512-thread block)
    for c in cases:
        assert 2 <= c.elems <= 4 and 12 <= c.num_steps <= 24 and c.V >= 2 * c.k, c.name
    assert {c.n_ss for c in cases} == {0, 1, 32, 64}
    assert any(c.max_len and c.max_len < c.num_steps for c in cases)
    # some elements retire early while others never finish and return their live beams
    assert any((c.retired_at >= 0).any() and (c.n_fin == 0).any() and c.ref.steps_run == c.num_steps for c in cases)
    # k = 8: all 128 candidate slots, seven forks at step 0 somewhere
    assert any(c.k == 8 and (c.ref.index[0].reshape(c.elems, 8) % 8 == 0).all() for c in cases)
    tok = bs.token_cases()
    assert {c.V for c in tok} == set(bs.TOKEN_V) and sum(c.V > 2048 for c in tok) >= 3
    assert any(c.n_ss for c in tok) and any(c.max_len for c in tok) and any(c.tie for c in tok)


def test_the_tie_cases_hold_the_ties_they_are_named_for():
    by = {c.name: c for c in bs.beam_cases()}
    for k in (2, 3, 8):
        a = by["tie_ab_k%d" % k]
        row = a.logits[0, 0]
        top = np.sort(row)[::-1]
        assert (top[:2 * k] == top[0]).all() and row[EOS] == top[0] and top[2 * k] < top[0] - 0.4        # (a)
        assert a.step_eos[0, 0] == 1
        assert (a.logits[1, :k] == a.logits[1, 0]).all()                                                  # (b)
        assert np.unique(a.ref.live_lp[0][0]).size == 1 and np.unique(a.ref.live_lp[1][0]).size == 1
        assert (a.ref.index[1][:k] == np.arange(k)).all()              # k-fold ties at every rank go by beam index
        c = by["tie_c_k%d" % k]
        assert (c.logits[1, :k] == c.logits[1, 0]).all() and c.logits[1, 0].argmax() == EOS
        assert c.step_eos[1, 0] == k                                   # (c) k equal new finished scores in one step
    for k in (2, 4, 8):
        d = by["eos_all_k%d" % k]
        assert d.V == 2 * k and (d.step_eos[1] == k).all()             # (d) exactly k of the 2k do not end in EOS
        assert (d.logits[1].argmax(-1) == EOS).all()
    for name in ("extreme_k2", "extreme_k3"):
        x = by[name].logits[0]
        assert (x == 80).any(-1).all() and (x == -1e4).any(-1).all() and ((x <= -80) & (x > -82)).any(-1).all()   # (e)
        assert np.isfinite(x).all()


def test_token_tie_rows_hit_the_thread_and_wave_seams():
    by = {c.name: c for c in bs.token_cases()}
    big = by["tok_tie_v4100"].logits
    peaks = {tuple(np.flatnonzero(r == r.max())) for r in big.reshape(-1, big.shape[-1])}
    assert {(0, 255, 256), (255, 256), (2047, 2048), (0, EOS), (EOS, 5), (2048, 4099)} <= peaks
    ids, done = by["tok_tie_v4100"].greedy()
    assert (ids == EOS).any() and done[-1].all()


@pytest.mark.parametrize("case", [c for c in ALL if c.max_len], ids=lambda c: c.name)
def test_max_len_reference_freezes_what_the_kernels_freeze(case):
    r, M = case.ref, case.max_len
    assert r.steps_run <= M and len(r.retired) == r.steps_run and r.retired[-1].all()
    assert (r.decodes[:, :, M:] == 0).all()
    assert (case.n_fin == 0).any() and (case.n_fin > 0).any()
