"""The CPU reference of k-beam search (tests/beam_search_ref.py): at k = 1 it is the oracle's beam-1 emulation, and
a scripted logits table pins each part of the rule include/mt3_hip.h states for mt3_engine_decode_beams."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import beam_search_ref as BR  # noqa: E402
import tiny_model as TM  # noqa: E402

from oracle import frontend as OF  # noqa: E402
from oracle import network as ON  # noqa: E402

V = 8
BIG = 30.0          # a logit that dominates the row


def _run(table, batch, k, num_steps):
    """scripted model: table(t) -> logits [batch*k, V] (a function of the step and the row only)"""
    calls = []

    def step(tok, t):
        calls.append(tok.numpy().copy())
        return torch.as_tensor(table(t), dtype=torch.float64)

    out = BR.beam_search(step, lambda index: None, batch, k, num_steps)
    return out + (calls,)


def _lp(row):
    return torch.log_softmax(torch.as_tensor(row, dtype=torch.float64), -1).numpy()


def test_k1_equals_oracle_beam1_on_the_tiny_model():
    x, _ = TM.inputs()
    orc = ON.Oracle(TM.params(), ON.T5Config(input_depth=TM.INPUT_DEPTH, **TM.CFG))
    with torch.no_grad():
        enc = orc.encode(x)
    ref = orc.beam1_decode(enc, TM.L)
    got, _, _ = BR.oracle_beam_search(orc, enc, 1, TM.L)
    assert np.array_equal(got[:, 0], ref)


def test_k1_equals_oracle_beam1_on_the_boosted_eos_set():
    """the case set of test_gpu_engine.py::test_beam1_decode_matches_oracle (MT3 shape, flat logits, boosted EOS)"""
    from mt3_amd import network
    cfg = network.T5Config(dtype="float32")
    params = network.init_random_params(cfg, seed=1, norm_scale_jitter=0.2)
    kern = params["decoder/logits_dense/kernel"].copy() * 0.3
    kern[:, 1] *= 1.5
    params["decoder/logits_dense/kernel"] = kern
    audio = OF.synth_audio(6, seed=3)
    x = np.stack([OF.compute_logmel(a, np.float64).astype(np.float32) for a in audio])
    x[2, 100:] = 0.0
    orc = ON.Oracle(params, ON.T5Config())
    with torch.no_grad():
        enc = orc.encode(x)
    ref = orc.beam1_decode(enc, 32)
    got, _, _ = BR.oracle_beam_search(orc, enc, 1, 32)
    assert np.array_equal(got[:, 0], ref)


def test_step0_expands_beam0_only():
    k = 2

    def table(t):
        z = np.zeros((k, V))
        z[:, 1] = -BIG                # no EOS
        z[0, 3] = 1.0                 # beam 0 prefers 3, then the rest
        z[1, 4] = BIG                 # beam 1 would dominate if it were live at step 0
        return z

    dec, scores, _, calls = _run(table, 1, k, 1)
    # both live beams descend from beam 0: tokens 3 and (lowest id among the tied rest) 0
    assert sorted(dec[0, :, 0].tolist()) == [0, 3]
    assert 4 not in dec[0, :, 0]
    assert np.isclose(scores[0, -1], _lp(table(0)[0])[3])


def test_eos_in_top_2k_finishes_and_brevity_penalty_applies():
    k = 2

    def table(t):
        z = np.full((k, V), -BIG)
        z[:, 3] = 0.0
        z[:, 5] = -0.5
        z[:, 1] = -1.0                # EOS third best of beam 0 at step 0: inside the top 2k = 4
        return z

    dec, scores, _, _ = _run(table, 1, k, 1)
    lp = _lp(table(0)[0])
    # a finished entry exists, so the result is the finished set: [unfilled, EOS]
    assert dec[0, -1, 0] == 1 and (dec[0, -1, 1:] == 0).all()
    assert np.isclose(scores[0, -1], lp[1] / BR.brevity_penalty(1))
    assert scores[0, 0] == BR.NEG_INF and (dec[0, 0] == 0).all()


def test_live_beams_are_the_top_k_non_eos():
    k = 2
    seen = []

    def table(t):
        z = np.full((k, V), -BIG)
        if t == 0:
            z[0, 1] = 0.0             # EOS best: finishes, does not become live
            z[0, 6] = -0.2
            z[0, 2] = -0.4
        else:
            z[:, 7] = 0.0
        return z

    def step(tok, t):
        seen.append(tok.numpy().copy())
        return torch.as_tensor(table(t))

    BR.beam_search(step, lambda i: None, 1, k, 2)
    assert seen[1].tolist() == [6, 2]     # the new live beams' tokens, best first


def test_ties_go_to_the_lower_flattened_index():
    k = 2

    def table(t):
        z = np.full((k, V), -BIG)
        z[:, 1] = -2 * BIG            # no EOS
        if t == 0:
            z[0, 2] = z[0, 3] = 0.0   # two beams with equal log-probs
        else:
            z[:, 5] = z[:, 6] = 0.0   # equal candidates in both beams: beam 0 (token 5, then 6) first
        return z

    seen = []

    def step(tok, t):
        seen.append(tok.numpy().copy())
        return torch.as_tensor(table(t))

    dec, _, _ = BR.beam_search(step, lambda i: None, 1, k, 2)
    assert seen[1].tolist() == [2, 3]
    best = dec[0, -1]
    assert best.tolist() == [2, 5] and dec[0, 0].tolist() == [2, 6]


def test_retirement_stops_the_search():
    k = 2

    def table(t):
        z = np.full((k, V), -BIG)
        z[:, 1] = 0.0                 # EOS with probability ~1 from every beam
        z[:, 4] = -3.0
        return z

    dec, scores, ran, calls = _run(table, 1, k, 50)
    assert ran < 50                   # two finished entries beat every live continuation
    assert (dec[0, :, :] == 1).any(axis=1).all()


def test_nothing_finished_returns_the_live_beams_in_ascending_order():
    k = 3

    def table(t):
        z = np.full((2 * k, V), -BIG)
        z[:, 1] = -2 * BIG            # no EOS
        z[:, 3] = 0.0
        z[:, 4] = -0.1
        z[:, 5] = -0.2
        return z

    dec, scores, ran, _ = _run(table, 2, k, 4)
    assert ran == 4 and not (dec == 1).any()
    assert (np.diff(scores, axis=1) >= 0).all()
    assert (dec[:, -1] == 3).all()    # the best live beam: token 3 at every step, last
    assert scores[0, -1] == pytest.approx(4 * _lp(table(0)[0])[3])


def test_finished_decodes_come_back_in_ascending_order():
    k = 3

    def table(t):
        z = np.full((k, V), -BIG)
        z[:, 1] = -0.5 - 0.3 * t      # EOS gets worse with depth
        z[:, 3] = 0.0
        z[:, 4] = -0.05
        return z

    dec, scores, _, _ = _run(table, 1, k, 12)
    assert (np.diff(scores[0]) >= 0).all()
    assert all((row == 1).sum() == 1 for row in dec[0])
