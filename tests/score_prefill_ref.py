"""Float64 references of the scoring path's kernels (csrc/score.hip; the rules are stated in include/mt3_hip.h next to
mt3_op_score_attention, mt3_op_score_embed, mt3_op_score_reduce and mt3_op_planes), independent of any kernel's tiling.

  prefill attention   per (segment b, head h, query i): the VISIBLE keys are {j <= i and key_tgt[b][j] != 0} with `causal`,
                      all keys without; unscaled logits q . k_j; out = sum_j softmax_j v_j over the visible keys only (a
                      masked key is left out of the maximum and of the sum, it is not given a large negative logit); a
                      query with no visible key gives a row of zeros.
  its error model     the same evaluation with the unnormalised probabilities exp(s - max) rounded to `p_dtype` before
                      P V (the kernel feeds them to the matrix instruction in the compute type) and the result rounded to
                      `out_dtype`: it sizes the per-row bounds of tests/test_gpu_score_attention.py.  With both None it IS
                      the reference.
  embed rows          table[tok] + pos[t] in f32 with the shift-right / caller-input / padding / clamping rules.
  scores              (logits[target] - logsumexp) * weight in float64, 0 where the target is 0; per-segment sums.
  planes              the hi / mid / lo bf16 split (tests/test_three_plane_arithmetic.py: split3), as bf16 bit patterns.
  three-plane product its error model: A W^T as the kernel's six plane products summed in float64, and with each of the
                      three small products (mid.mid, hi.lo, lo.hi) left out in turn; x6_bound turns them into the bound of
                      a case of tests/test_gpu_three_plane_ops.py: half of what the best five-product kernel would show.
"""
import math

import numpy as np
import torch

from tests.test_three_plane_arithmetic import split3


def round_ct(x, ct):
    """float64 -> ct (round to nearest even) -> float64; ct None: unchanged"""
    return x if ct is None else x.to(ct).double()


def visible_keys(Lq, n_keys, causal, key_tgt=None, B=1):
    """bool [B][Lq][n_keys]"""
    vis = torch.ones(B, Lq, n_keys, dtype=torch.bool)
    if causal:
        vis &= (torch.arange(n_keys)[None, :] <= torch.arange(Lq)[:, None])[None]
        if key_tgt is not None:
            vis &= (torch.as_tensor(key_tgt).cpu().reshape(B, 1, n_keys) != 0)
    return vis


def prefill_attention_ref(q, k, v, causal, key_tgt=None, p_dtype=None, out_dtype=None):
    """q [B][Lq][H][64], k / v [B][n_keys][H][64] (any float dtype: the values as the kernel reads them), key_tgt [B][Lq]
    or None -> out float64 [B][Lq][H][64] on the CPU."""
    q, k, v = (t.detach().cpu().double() for t in (q, k, v))
    B, Lq, H, _ = q.shape
    n_keys = k.shape[1]
    vis = visible_keys(Lq, n_keys, causal, key_tgt, B)[:, None]                     # [B][1][Lq][n_keys]
    never = ~vis.any(2)[:, 0, :, None, None]                                        # keys no query sees: not read at all
    k, v = torch.where(never, torch.zeros_like(k), k), torch.where(never, torch.zeros_like(v), v)
    s = torch.einsum("bihd,bjhd->bhij", q, k)
    lowest = torch.full_like(s, -math.inf)
    m = torch.where(vis, s, lowest).amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))                      # no visible key: any finite value
    p = torch.where(vis, torch.exp(s - m), torch.zeros_like(s))                     # masked: selected away, exactly 0
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhij,bjhd->bhid", round_ct(p, p_dtype), v)
    o = torch.where(l > 0, o / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(o))
    return round_ct(o.permute(0, 2, 1, 3).contiguous(), out_dtype)


# ------------------------------------------------------------------------------------------------ embed rows, scores
def clamp_ids(x, vocab):
    return np.clip(np.asarray(x, np.int64), 0, vocab - 1)


def embed_rows_ref(table, pos, targets, dec_in, segments, Lp, length, seg0, vocab):
    """-> (y f32 [segments * Lp][dim], tgt_pad int32 [segments * Lp]) for the chunk of `segments` segments that starts at
    segment seg0 of the caller arrays targets / dec_in [batch][length]"""
    table, pos = np.asarray(table, np.float32), np.asarray(pos, np.float32)
    tgt = np.zeros((segments, Lp), np.int64)
    tok = np.zeros((segments, Lp), np.int64)
    rows = slice(seg0, seg0 + segments)
    tgt[:, :length] = clamp_ids(np.asarray(targets)[rows], vocab)
    if dec_in is not None:
        tok[:, :length] = clamp_ids(np.asarray(dec_in)[rows], vocab)
    else:
        tok[:, 1:length] = tgt[:, :length - 1]                                     # shift right, BOS = 0 at t = 0
    y = (table[tok] + pos[np.arange(Lp)][None]).astype(np.float32)
    return y.reshape(segments * Lp, -1), tgt.reshape(-1).astype(np.int32)


def token_scores_ref(logits, tgt_pad, weights=None):
    """logits [rows][vocab], tgt_pad [rows], weights [rows] or None -> float64 [rows]"""
    x = np.asarray(logits, np.float64)
    tgt = np.asarray(tgt_pad, np.int64)
    m = x.max(-1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[:, 0]
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float64)
    return np.where(tgt != 0, (x[np.arange(len(x)), tgt] - lse) * w, 0.0)


def sequence_scores_ref(token_scores, segments, Lp, length):
    """float32(exactly rounded sum) of the first `length` entries of every segment's Lp token scores"""
    ts = np.asarray(token_scores).reshape(segments, Lp)[:, :length]
    return np.array([np.float32(math.fsum(float(x) for x in row)) for row in ts], np.float32)


# ------------------------------------------------------------------------------------------------------------ planes
def bf16_bits(x):
    """f32 values that are exactly representable in bf16 -> their 16-bit patterns"""
    u = np.asarray(x, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def planes_ref(w):
    """f32 [n] -> (hi, mid, lo) as uint16 bf16 bit patterns: the host split rule"""
    hi, mid, lo, _, _ = split3(w)
    return bf16_bits(hi), bf16_bits(mid), bf16_bits(lo)


# ------------------------------------------------------------------------------- the three-plane product's error model
X6_SIX = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))         # mm, hl, lh, hm, mh, hh: gemm_x6_kernel's order
X6_DROPS = {"mid.mid": (1, 1), "hi.lo": (0, 2), "lo.hi": (2, 0)}   # the three small products; first factor A, second W


def planes64(x):
    """torch f32 values -> their (hi, mid, lo) bf16 planes as float64 (the rule of planes_ref, on any device)"""
    x = x.float()
    hi = x.bfloat16().float()
    r1 = x - hi
    mid = r1.bfloat16().float()
    lo = (r1 - mid).bfloat16().float()
    return hi.double(), mid.double(), lo.double()


def plane_product(A, W, drop=None):
    """A f32 [M][K], W f32 [N][K] -> float64 [M][N]: A W^T as the sum over X6_SIX (without X6_DROPS[drop]) of the plane
    products, each summed in float64 -- what gemm_x6_kernel forms, without its f32 accumulation"""
    a, w = planes64(A), planes64(W)
    return sum(a[i] @ w[j].T for i, j in X6_SIX if drop is None or (i, j) != X6_DROPS[drop])


def x6_bound(today, errors_of):
    """The bound of one three-plane case: the smaller of `today` and HALF the smallest error among the three five-product
    emulations, provided the six-product emulation stays under a QUARTER of that; else `today`.  errors_of(drop) -> the
    error figure of the emulation without that product (None: all six) against the case's float64 reference, taken the way
    the test takes the kernel's.  -> (bound, distinguishes, six, {name: five-product error})"""
    six = errors_of(None)
    five = {name: errors_of(name) for name in X6_DROPS}
    tight = min(today, 0.5 * min(five.values()))
    ok = six < tight / 4
    return (tight if ok else today), ok, six, five


def gelu_tanh(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def x6_epilogue(epi, prod, A, res=None, aux=None, seq=0):
    """float64 prod [M][N] = A W^T (exact, or an emulation of it) -> what mt3_op_gemm_x6 stores for epilogue `epi`
    ("STORE", "GEGLU": with the row's 1 / rms of A in float64; "RESID": res + prod; "POS": prod + aux[row % seq]; "HEADS":
    [2][M / seq][N / 128][seq][64])"""
    M, N = prod.shape
    if epi in ("STORE", "GEGLU"):
        prod = prod * torch.rsqrt((A.double() ** 2).mean(-1, keepdim=True) + 1e-6)
    if epi == "STORE":
        return prod
    if epi == "GEGLU":                                     # rows [32q, 32q + 16) gate columns 16q .., the next 16 linear
        p4 = prod.view(M, N // 32, 2, 16)
        return (gelu_tanh(p4[:, :, 0]) * p4[:, :, 1]).reshape(M, N // 2)
    if epi == "RESID":
        return res.double() + prod
    if epi == "POS":
        return prod + aux.double()[torch.arange(M, device=prod.device) % seq]
    return prod.view(M // seq, seq, 2, N // 128, 64).permute(2, 0, 3, 1, 4).contiguous()
