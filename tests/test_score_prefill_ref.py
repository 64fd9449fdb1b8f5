"""tests/score_prefill_ref.py on the CPU: the prefill-attention reference (masked keys SELECTED away) against a second
formulation -- a dense additive -inf mask through torch.softmax in float64 --, the zero-row rule, the error model without
rounding, the numpy forms of the embed row, the scores and the planes on hand-made cases, and the three-plane product's
error model: on every shape of test_gemm_x6 six products stay under a quarter of the bound and no five reach it."""
import math

import numpy as np
import pytest
import torch

from tests import score_prefill_ref as R


def _inputs(B, Lq, n_keys, H, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Lq, H, 64, generator=g, dtype=torch.float64) * 0.35
    k = torch.randn(B, n_keys, H, 64, generator=g, dtype=torch.float64)
    v = torch.randn(B, n_keys, H, 64, generator=g, dtype=torch.float64)
    return q, k, v


def _dense(q, k, v, causal, key_tgt):
    """additive mask + torch.softmax; rows without a visible key come out as NaN there and are set to 0"""
    B, Lq, H, _ = q.shape
    vis = R.visible_keys(Lq, k.shape[1], causal, key_tgt, B)
    bias = torch.where(vis, 0.0, -math.inf).double()[:, None]
    w = torch.softmax(torch.einsum("bihd,bjhd->bhij", q, k) + bias, -1)
    w = torch.where(vis.any(-1)[:, None, :, None], w, torch.zeros_like(w))
    return torch.einsum("bhij,bjhd->bihd", w, v)


def _masks(Lq):
    one = torch.ones(Lq, dtype=torch.int32)
    tail, first, seam, chunk = one.clone(), one.clone(), one.clone(), one.clone()
    tail[min(70, Lq - 1):] = 0
    first[0] = 0
    seam[[Lq // 2 - 1, Lq // 2, Lq // 2 + 1]] = 0
    chunk[Lq // 3: 2 * Lq // 3] = 0
    return {"all": one, "tail": tail, "first": first, "seam": seam, "chunk": chunk, "none": torch.zeros_like(one)}


def test_reference_equals_the_dense_mask_formulation():
    B, Lq, H = 3, 192, 2
    q, k, v = _inputs(B, Lq, Lq, H, 0)
    masks = _masks(Lq)
    names = list(masks)
    for i in range(0, len(names), B):
        tgt = torch.stack([masks[n] for n in names[i:i + B]])
        ref, dense = R.prefill_attention_ref(q, k, v, True, tgt), _dense(q, k, v, True, tgt)
        assert torch.isfinite(ref).all()
        assert float((ref - dense).abs().max()) < 1e-13, names[i:i + B]
    # causal without targets, and the cross form (more keys than queries, nothing masked)
    assert float((R.prefill_attention_ref(q, k, v, True) - _dense(q, k, v, True, None)).abs().max()) < 1e-13
    q2, k2, v2 = _inputs(2, 64, 256, H, 1)
    assert float((R.prefill_attention_ref(q2, k2, v2, False) - _dense(q2, k2, v2, False, None)).abs().max()) < 1e-13


def test_visibility_is_causal_and_by_target():
    vis = R.visible_keys(4, 4, True, torch.tensor([[1, 0, 5, 1]]))[0]
    assert vis.tolist() == [[True, False, False, False], [True, False, False, False], [True, False, True, False],
                            [True, False, True, True]]
    assert R.visible_keys(2, 3, False)[0].all()


def test_query_without_a_visible_key_gives_a_zero_row_and_single_key_rows_are_v():
    B, Lq, H = 1, 64, 2
    q, k, v = _inputs(B, Lq, Lq, H, 2)
    tgt = torch.ones(B, Lq, dtype=torch.int32)
    tgt[0, :3] = 0
    out = R.prefill_attention_ref(q, k, v, True, tgt)
    assert (out[0, :3] == 0).all()
    assert torch.equal(out[0, 3], v[0, 3])                          # one visible key: its V row, exactly
    # a hidden key holds NaN: the reference never multiplies it in
    k[0, 1], v[0, 1] = math.nan, math.inf
    assert torch.equal(R.prefill_attention_ref(q, k, v, True, tgt), out)
    assert (R.prefill_attention_ref(q, k, v, True, torch.zeros(B, Lq, dtype=torch.int32)) == 0).all()


def test_error_model_without_rounding_is_the_reference_and_with_rounding_is_close():
    q, k, v = _inputs(2, 128, 128, 2, 3)
    tgt = torch.ones(2, 128, dtype=torch.int32)
    tgt[1, 64:100] = 0
    ref = R.prefill_attention_ref(q, k, v, True, tgt)
    assert torch.equal(R.prefill_attention_ref(q, k, v, True, tgt, p_dtype=None, out_dtype=None), ref)
    for ct, lo, hi in ((torch.bfloat16, 5e-4, 4e-3), (torch.float32, 1e-9, 2e-7)):
        model = R.prefill_attention_ref(q, k, v, True, tgt, p_dtype=ct, out_dtype=ct)
        err = float((model - ref).norm() / ref.norm())
        assert lo < err < hi, (ct, err)                            # half an ulp of the format per element, more or less


def test_embed_rows_scores_and_planes_on_small_cases():
    rng = np.random.default_rng(0)
    vocab, dim, Lp, length = 7, 8, 64, 3
    table, pos = rng.standard_normal((vocab, dim)).astype(np.float32), rng.standard_normal((Lp, dim)).astype(np.float32)
    targets = np.array([[9, 9, 9], [2, -4, 5000], [3, 0, 1]], np.int32)
    y, tgt = R.embed_rows_ref(table, pos, targets, None, 2, Lp, length, 1, vocab)
    assert tgt.reshape(2, Lp)[:, :4].tolist() == [[2, 0, 6, 0], [3, 0, 1, 0]]
    y = y.reshape(2, Lp, dim)
    assert np.array_equal(y[0, 0], table[0] + pos[0]) and np.array_equal(y[0, 1], table[2] + pos[1])
    assert np.array_equal(y[0, 2], table[0] + pos[2]) and np.array_equal(y[1, 3], table[0] + pos[3])
    y2, _ = R.embed_rows_ref(table, pos, targets, targets, 1, Lp, length, 1, vocab)
    assert np.array_equal(y2[2], table[6] + pos[2]) and np.array_equal(y2[5], table[0] + pos[5])
    # scores: a uniform row of V logits scores -log V; padding scores 0
    ts = R.token_scores_ref(np.zeros((2, 5)), [3, 0], np.array([2.0, 1.0]))
    assert abs(ts[0] + 2 * math.log(5)) < 1e-15 and ts[1] == 0
    seq = R.sequence_scores_ref(np.array([1.0, 2.0 ** -30, 5.0, 7.0] * 16 * 2, np.float32), 2, 64, 2)
    assert seq.tolist() == [1.0, 1.0]                                              # length 2 of Lp 64: 1 + 2^-30 -> f32
    hi, mid, lo = R.planes_ref(np.float32([1 + 2.0 ** -17, -0.0, 16 - 2.0 ** -20, 1 + 2.0 ** -9 + 2.0 ** -18]))
    assert hi.tolist() == [0x3F80, 0x8000, 0x4180, 0x3F80] and mid[1] == 0 and lo[1] == 0
    assert mid[0] == 0x3700 and lo[0] == 0 and mid[2] == 0xB580                   # 2^-17; 16 - 2^-20: hi carries to 16
    assert mid[3] == 0x3B00 and lo[3] == 0x3680                                  # 2^-9, 2^-18


# ------------------------------------------------------------------------------- the three-plane product's error model
X6_TODAY = {"STORE": 2e-5, "RESID": 2e-5, "POS": 2e-5, "HEADS": 2e-5, "GEGLU": 3e-5}
X6_CASES = [(epi, M, N, K) for epi in ("STORE", "RESID", "POS", "HEADS") for M in (1, 64, 130, 192)
            for N, K in ((128, 64), (1152, 512), (512, 1024))] + [("GEGLU", M, 256, 512) for M in (1, 64, 130, 192)]


def test_plane_product_is_the_product_up_to_the_three_products_it_leaves_out():
    g = torch.Generator().manual_seed(5)
    A, W = torch.randn(7, 64, generator=g), torch.randn(128, 64, generator=g)
    exact = A.double() @ W.double().T
    scale = A.double().abs() @ W.double().abs().T
    assert float(((R.plane_product(A, W) - exact).abs() / scale).max()) < 3 * 2.0 ** -24 + 2.0 ** -25
    for name in R.X6_DROPS:                                 # a 2^-16-sized term per element is missing
        e = float(((R.plane_product(A, W, name) - exact).abs() / scale).max())
        assert 2.0 ** -22 < e < 2.0 ** -15, (name, e)
    for got, want in zip(R.planes64(A), R.planes_ref(A.numpy().ravel())):
        assert np.array_equal(R.bf16_bits(got.float().numpy().ravel()), want)


@pytest.mark.parametrize("epi,M,N,K", X6_CASES)
def test_x6_bound_lets_six_products_through_and_no_five(epi, M, N, K):
    """the shapes, epilogues and operand distributions of test_gemm_x6 (tests/test_gpu_three_plane_ops.py), which applies
    the same rule to its own operands"""
    g = torch.Generator().manual_seed(M * 7 + N + K)
    seq = {1: 1, 64: 64, 130: 65, 192: 64}[M] if epi == "HEADS" else 64 if epi == "POS" else 0
    A = torch.randn(M, K, generator=g) * (1 + 3 * torch.rand(M, 1, generator=g))
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    aux = torch.randn(seq, N, generator=g) if epi == "POS" else None
    res = torch.randn(M, N, generator=g)
    finish = lambda prod: R.x6_epilogue(epi, prod, A, res, aux, seq)
    ref = finish(A.double() @ W.double().T)
    rel = lambda got: float((got - ref).norm() / ref.norm())
    tol, tells, six, five = R.x6_bound(X6_TODAY[epi], lambda drop: rel(finish(R.plane_product(A, W, drop))))
    print(f"gemm_x6 {epi} M {M} N {N} K {K}: bound {tol:.2e} (today's {X6_TODAY[epi]:.0e}), six products {six:.2e}, without "
          + ", ".join(f"{n} {e:.2e}" for n, e in five.items()))
    assert tells and tol <= X6_TODAY[epi] and six < tol / 4
    assert all(e >= 2 * tol for e in five.values()), five
