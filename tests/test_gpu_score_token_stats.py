"""score_token_stats_kernel alone (mt3_op_score_token_stats, include/mt3_hip.h) on scripted logits against numpy in
float64: the arg-max with its tie rule (lowest id; ties inside a thread's stride, across lanes, across waves), the
top-1 and token log-probabilities, padding rows, weights, vocabularies that are no multiple of the 256-thread stride --
and, on the engine's own logits, the bits of mt3_engine_score's token scores.

Tolerance 1e-5 absolute: the f32 rounding of a log-sum over <= 1664 terms.  The rows keep |score| below 32 (f32 spacing
1.9e-6 there, two roundings in x - max - log(sum)): the "+80 and -80 in one row" case scores a target of the +80 group,
because a -160 result has an f32 spacing of 1.5e-5 by itself, which is the format's resolution and not the kernel's error."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, network  # noqa: E402

VOCABS = (2, 255, 256, 257, 1536, 1664)
TOL = 1e-5


def _rows(V, seed):
    """(logits f32 [n, V], targets int32 [n], name of each row, expected arg-max where the row scripts one or None)"""
    rng = np.random.default_rng(seed)
    rows, tgts, names, want = [], [], [], []

    def add(name, x, tgt, top=None):
        rows.append(np.asarray(x, np.float32))
        tgts.append(int(tgt))
        names.append(name)
        want.append(top)

    def rnd():
        return (rng.standard_normal(V) * 3.0).astype(np.float32)

    x = rnd()
    add("target_is_argmax", x, int(x.argmax()) if x.argmax() else 1)
    add("target_0_padding", rnd(), 0)
    add("target_last_id", rnd(), V - 1)
    add("equal_logits", np.full(V, 1.5, np.float32), V - 1, top=0)
    add("near_plus_80", 80.0 + rng.uniform(-1, 1, V), rng.integers(1, V))
    add("near_minus_80", -80.0 + rng.uniform(-1, 1, V), rng.integers(1, V))
    x = np.where(np.arange(V) % 2 == 0, -80.0, 80.0) + rng.uniform(-1, 1, V)
    add("plus_and_minus_80", x, 1)                               # odd ids are the +80 group
    if V > 300:
        x = rnd()
        x[[5, 300]] = x.max() + 1.0                              # lane 5 of wave 0 against lane 44 of wave 0, second stride
        add("tie_5_300", x, rng.integers(1, V), top=5)
    if V > 256:
        x = rnd()
        x[[255, 256]] = x.max() + 1.0                            # last lane of wave 3 against thread 0's second element
        add("tie_255_256", x, rng.integers(1, V), top=255)
        x = rnd()
        x[[63, 64, 200]] = x.max() + 0.5                         # across waves 0 / 1 / 3
        add("tie_63_64_200", x, 200, top=63)
    return np.stack(rows), np.array(tgts, np.int32), names, want


def _reference(x, tgt, w):
    x64 = x.astype(np.float64)
    m = x64.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(x64 - m).sum(-1, keepdims=True)))[:, 0]
    idx = np.arange(len(x))
    top = x64.argmax(-1)                                         # numpy: the first maximum
    live = tgt != 0
    ww = np.ones(len(x)) if w is None else w.astype(np.float64)
    return (np.where(live, (x64[idx, tgt] - lse) * ww, 0.0), np.where(live, top, 0),
            np.where(live, x64[idx, top] - lse, 0.0))


def _op(x, tgt, w, outputs=(True, True, True)):
    lib = _lib.load()
    n, V = x.shape
    dx, dt = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(tgt)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(w)).cuda() if w is not None else None
    tok = torch.full((n,), 7.0, device="cuda") if outputs[0] else None
    tid = torch.full((n,), -7, device="cuda", dtype=torch.int32) if outputs[1] else None
    tsc = torch.full((n,), 7.0, device="cuda") if outputs[2] else None
    ptr = (lambda t: t.data_ptr() if t is not None else None)
    _lib.check(lib.mt3_op_score_token_stats(dx.data_ptr(), dt.data_ptr(), ptr(dw), n, V, ptr(tok), ptr(tid), ptr(tsc),
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (tok, tid, tsc))


def _compare(x, tgt, w, names, want):
    tok, tid, tsc = _op(x, tgt, w)
    r_tok, r_top, r_tsc = _reference(x, tgt, w)
    for i, name in enumerate(names):
        print(f"V={x.shape[1]} rows={len(x)} {name}: top1 {tid[i]} (ref {r_top[i]}) "
              f"|token err| {abs(tok[i] - r_tok[i]):.2e} |top1 err| {abs(tsc[i] - r_tsc[i]):.2e}")
    assert np.array_equal(tid, r_top), (names, tid, r_top)
    for i, t in enumerate(want):
        if t is not None and tgt[i] != 0:
            assert tid[i] == t, (names[i], tid[i], t)
    assert np.abs(tok - r_tok).max() <= TOL
    assert np.abs(tsc - r_tsc).max() <= TOL
    assert np.all(tsc <= 0) and np.all(tok[tgt == 0] == 0) and np.all(tsc[tgt == 0] == 0)
    return tok, tid, tsc


@pytest.mark.parametrize("weighted", [False, True], ids=["weights_null", "weights_given"])
@pytest.mark.parametrize("V", VOCABS)
def test_scripted_rows(V, weighted):
    x, tgt, names, want = _rows(V, seed=V)
    w = np.random.default_rng(1).uniform(0.25, 1.0, len(x)).astype(np.float32) if weighted else None
    all_tok, all_tid, all_tsc = _compare(x, tgt, w, names, want)                 # every row in one launch
    for i in range(len(x)):                                                      # rows = 1: each row alone, same bits
        tok, tid, tsc = _compare(x[i:i + 1], tgt[i:i + 1], None if w is None else w[i:i + 1], names[i:i + 1], want[i:i + 1])
        assert tok.view(np.uint32) == all_tok[i:i + 1].view(np.uint32) and tid == all_tid[i]
        assert tsc.view(np.uint32) == all_tsc[i:i + 1].view(np.uint32)
    for s in (0, len(x) - 5):                                                    # rows = 5
        sl = slice(s, s + 5)
        _compare(x[sl], tgt[sl], None if w is None else w[sl], names[sl], want[sl])


def test_target_at_the_argmax_has_no_margin_and_ids_are_clamped():
    x, tgt, names, want = _rows(1664, seed=3)
    tgt = x.astype(np.float64).argmax(-1).astype(np.int32)
    tgt[tgt == 0] = 1
    tok, tid, tsc = _op(x, tgt, None)
    same = tid == tgt
    assert same.sum() >= len(x) - 2                              # (an arg-max at id 0 cannot be a target: 0 is padding)
    assert np.array_equal(tok[same].view(np.uint32), tsc[same].view(np.uint32))
    # ids outside [0, vocab) are clamped as mt3_engine_score clamps them: -4 -> 0 (padding), 5000 -> vocab - 1
    bad = np.array([-4, 5000] + [1] * (len(x) - 2), np.int32)
    tok_b, tid_b, _ = _op(x, bad, None)
    ref = _op(x, np.array([0, 1663] + [1] * (len(x) - 2), np.int32), None)
    assert np.array_equal(tok_b.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(tid_b, ref[1])


def test_each_output_may_be_null():
    x, tgt, _, _ = _rows(257, seed=4)
    full = _op(x, tgt, None)
    for k in range(3):
        only = _op(x, tgt, None, outputs=tuple(j == k for j in range(3)))
        assert np.array_equal(only[k], full[k]) and all(only[j] is None for j in range(3) if j != k)


def test_token_scores_have_the_bits_of_engine_score():
    """vocabulary 1536: the logits of one Transformer.score(..., return_logits=True) call fed back through the op"""
    cfg = network.T5Config(dtype="float32", num_encoder_layers=1, num_decoder_layers=1)
    params = network.init_random_params(cfg, seed=0, norm_scale_jitter=0.2)
    eng = network.Transformer(cfg, input_length=256, max_decode_length=64, max_batch=2)
    eng.load_params(params)
    g = torch.Generator().manual_seed(0)
    eng.encode((torch.randn(2, 256, 512, generator=g) * 2.0 - 4.0).cuda())
    rng = np.random.default_rng(2)
    tgt = rng.integers(1, 1536, size=(2, 40)).astype(np.int32)
    tgt[0, 30:] = 0
    tgt[1, 7] = 0
    w = rng.uniform(0.25, 1.0, size=tgt.shape).astype(np.float32)
    for weights in (None, w):
        _, ts, lg = eng.score(tgt, weights=weights, return_token_scores=True, return_logits=True)
        lg = lg.cpu().numpy().reshape(-1, 1536)
        assert lg.shape[1] == 1536
        tok, tid, tsc = _op(lg, tgt.reshape(-1), None if weights is None else weights.reshape(-1))
        assert np.array_equal(tok.view(np.uint32), ts.cpu().numpy().reshape(-1).view(np.uint32))
        live = tgt.reshape(-1) != 0
        assert np.array_equal(tid[live], lg.astype(np.float64).argmax(-1)[live]) and np.all(tid[~live] == 0)
        r_tok, _, r_tsc = _reference(lg, tgt.reshape(-1), None if weights is None else weights.reshape(-1))
        assert np.abs(tsc - r_tsc).max() <= TOL and np.abs(tok - r_tok).max() <= TOL
