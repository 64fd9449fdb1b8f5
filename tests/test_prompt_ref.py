"""tests/prompt_ref.py on the CPU: without prompts it IS tests/beam_search_ref.py, k = 1 is the beam-1 rule, and inside a
prompt nothing but the token moves."""
import numpy as np
import pytest

from tests import beam_script as bs
from tests import prompt_ref as pr
from tests.beam_search_ref import EOS, NEG_INF, beam_search, brevity_penalty

PLAIN = [c for c in bs.beam_cases() if c.name in ("v2k_k3", "retire_k4", "table_v130_k7", "scale32_retire_k4", "tie_ab_k2",
                                                  "maxlen_k4", "eos_all_k4")]


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: c.name)
def test_without_prompts_the_reference_is_beam_search_ref_bit_for_bit(case):
    want = beam_search(lambda tok, t: case.scaled(t), lambda index: None, case.elems, case.k, case.num_steps)
    for prompts in (None, [None] * case.elems, [[]] * case.elems):
        got = pr.beam_search(lambda tok, t: case.scaled(t), lambda index: None, case.elems, case.k, case.num_steps,
                             prompts=prompts)
        assert np.array_equal(got[0], want[0]) and got[2] == want[2]
        assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64))            # the scores: the same bits
    ref, mine = case.ref, pr.run_reference(case)
    assert np.array_equal(mine.decodes, ref.decodes) and mine.steps_run == ref.steps_run
    assert np.array_equal(mine.scores.view(np.int64), ref.scores.view(np.int64))
    for a, b in zip(mine.retired, ref.retired):
        assert np.array_equal(a, b)


def _beam1(logits, num_steps):
    """The beam-1 rule of SURVEY.md A.5 / argmax_step_kernel<true>, written out on its own for one row: top 2 of
    log_softmax, the live hypothesis follows the best non-EOS candidate, an EOS candidate finishes live + EOS."""
    import torch
    live, best, blen, seq = 0.0, 0.0, -1, np.zeros(num_steps, np.int32)
    bp_max = brevity_penalty(num_steps + 1)
    for t in range(num_steps):
        lp = torch.log_softmax(torch.as_tensor(logits[t]).double(), -1).numpy()
        i1, i2 = np.argsort(-lp, kind="stable")[:2]
        eos = 1 if i1 == EOS else (2 if i2 == EOS else 0)
        if eos:
            score = (live + lp[i1 if eos == 1 else i2]) / brevity_penalty(t + 1)
            if blen < 0 or score > best:
                best, blen = score, t
        tok = i2 if eos == 1 else i1
        live += lp[tok]
        seq[t] = tok
        if blen >= 0 and best > live / bp_max:
            break
    if blen >= 0:
        seq[blen:] = 0
        seq[blen] = EOS
    return seq


@pytest.mark.parametrize("name", ("tok_v255", "tok_v1536", "tok_scale1_v257"))
def test_k1_without_prompts_is_the_beam1_rule(name):
    case = next(c for c in bs.token_cases() if c.name == name)
    got = pr.run_reference(case).decodes[:, 0]
    for b in range(case.elems):
        x = np.stack([case.scaled(t)[b] for t in range(case.num_steps)])
        assert np.array_equal(got[b], _beam1(x, case.num_steps)), (name, b)


@pytest.mark.parametrize("case", pr.beam_prompt_cases() + pr.token_prompt_cases(), ids=lambda c: c.name)
def test_inside_a_prompt_only_the_token_moves(case):
    ref, k = case.ref, case.k
    assert ref.steps_run >= 1
    for b in range(case.elems):
        p = case.plen(b)
        for t in range(min(p, ref.steps_run)):
            assert (ref.live_seq[t][b, :, t] == case.prompts[b][t]).all()
            assert np.array_equal(ref.live_lp[t][b], [0.0] + [NEG_INF] * (k - 1))     # not scored
            assert not ref.fin_valid[t][b].any() and (ref.fin_score[t][b] == NEG_INF).all()
            assert np.array_equal(ref.index[t][b * k:(b + 1) * k], np.arange(b * k, (b + 1) * k))   # no fork
            assert not ref.retired[t][b] or (case.max_len and t + 1 >= case.max_len)
        # every returned decode with a token in it starts with the prompt (as far as the element ran)
        ran = min(case.max_len or case.num_steps, case.num_steps)
        for d in ref.decodes[b]:
            if d.any():
                assert list(d[:min(p, ran)]) == (case.prompts[b] or [])[:ran], (case.name, b)
    # the first free step expands beam 0 only: all k children of step p have parent 0
    for b in range(case.elems):
        p = case.plen(b)
        if p and p < ref.steps_run and not ref.retired[p - 1][b]:
            assert (ref.index[p][b * k:(b + 1) * k] == b * k).all()


def test_the_absolute_length_is_what_the_brevity_penalty_sees():
    """One row, one prompt token, EOS certain at the first free step: the finished score is logp_eos / bp(2)."""
    V = 8
    logits = np.full((3, 1, V), -5.0, np.float32)
    logits[:, 0, EOS] = 5.0
    dec, sc, ran = pr.beam_search(lambda tok, t: logits[t], lambda i: None, 1, 1, 3, prompts=[[4]])
    lp = float(np.log(np.exp(5.0) / (np.exp(5.0) + (V - 1) * np.exp(-5.0))))
    assert list(dec[0, 0]) == [4, EOS, 0] and ran == 2
    assert abs(sc[0, 0] - lp / brevity_penalty(2)) < 1e-12


def test_greedy_reference():
    logits = np.zeros((4, 2, 6), np.float32)
    logits[:, :, EOS] = 1.0                              # EOS is every step's arg-max
    ids, done = pr.greedy(logits, [[5, 3], None])
    assert ids.tolist() == [[5, 3, EOS, 0], [EOS, 0, 0, 0]]
    assert done.T.tolist() == [[0, 0, 1, 1], [1, 1, 1, 1]]
    ids, done = pr.greedy(logits, [[5, 3, 4], None], max_len=2)
    assert ids.tolist() == [[5, 3, 0, 0], [EOS, 0, 0, 0]] and done.T.tolist() == [[0, 1, 1, 1], [1, 1, 1, 1]]
