"""Float64 reference, scripted input cases and error models of the encoder self-attention (csrc/attention.hip:
enc_attn_kernel, enc_attn_split_kernel; csrc/enc_attention_x6.hip: enc_attn_x6_kernel), independent of any kernel's
tiling.  Everything is torch on whatever device the inputs live on (the CPU test runs it on the CPU, the GPU file on the
GPU), one small group of heads at a time, so nothing larger than a few MB is ever allocated.

The reference: per (batch b, head h) out = softmax_k(q . k) V over ALL T keys, logits unscaled (no 1/sqrt(d)), in float64
on the values exactly as the kernel reads them (already rounded to its input type).

Input cases (make_case -> qkv f32 [B][T][3][H][64]); what each one catches:
  random    i.i.d. normal, Q scaled by 0.35 (the inputs of test_encoder_attention): the plain arithmetic, and the only case
            in which all six plane products of BOTH matrix products carry weight -- the five-product bounds bite here.
  rising    q_i = a_i u + noise, k_j = c_j u + noise, u a unit vector, c_j increasing in j, the sign of a_i alternating
  falling   between neighbouring queries (|a_i| varies too, |a_i c_j| <= 4.5: the f32 instruction accumulates a logit of
            magnitude 8 to ulp(8) = 9.5e-7, which alone is half the row bound); falling: c_j decreasing.  In a query with a_i c_j rising the
            running maximum moves at EVERY 64-key chunk (alpha < 1 each time), in its neighbour it is fixed in the first
            chunk (alpha = 1 from then on).  An alpha or a 1/l fetched from the wrong lane (the kernels take both from lane
            fg * 4 + r), or a rescale that is skipped, shows in alternate rows.
  one_hot   K rows are +-1 sign vectors, q_i = 2 k_pi(i): the logit of key pi(i) is 128, every other at least 27.8 below
            (weight < 2^-40), so out[i] = V[pi(i)].  pi (permutation()) sends neighbouring queries to different halves of
            the keys -- hence to different 64-key chunks and different staged parts in every kernel.  Catches a key order
            that differs between the score product and the P V product, the V^T pair packing, a key part staged twice.
  uniform   Q = 0: every output row of a head is the mean of the head's T V rows.  V[k][d] = m_d + z_k with z_k a
            zero-sum ramp visited in a scattered order, |m_d| ~ 0.03: a key dropped (or counted twice) moves every
            element of the row by (mean_d - V[k][d]) / (T - 1) (resp. / (T + 1)), i.e. by ~|z_k| / T against 0.03.
  large     logits of standard deviation ~30; in the odd heads dimension 0 of q and k adds -384 to every logit, so that
            every logit of a query is below -200.  q and k sit on a grid of 1/4 (|x| <= 8; 16 and -24 in dimension 0):
            every logit is an exact f32 (and bf16-plane) sum in any order, so the case measures the exponential's domain
            -- the -3.0e38f start value, exp2 of a large negative argument, the bf16 kernel's base-2 maximum -- and not
            the rounding of a product at magnitude 400, which no f32 accumulation could hold to 3e-5.  V sits on bf16
            values: with P this close to one-hot the small plane products of a generic V would be worth 3e-7 of the
            output, and half of that is less than any f32 accumulation can deliver; single-plane V makes the case say
            openly that it cannot tell five products from six (below) and keep 3e-5.

Error models:
  bf16      model_bf16: the reference with exp(s - max) rounded to bf16 before P V (the kernel feeds the matrix instruction
            bf16 probabilities; the row sum is taken over the unrounded ones) and the result rounded to bf16.
  x6        plane_attention: Q, K, P and V as three bf16 planes each (hi = rne(x), mid = rne(x - hi), lo = rne(x - hi - mid)),
            each matrix product as the sum of the listed plane products in float64; P = f32(exp(s - max)).  SIX is the
            kernel's product set; DROPS names the three small products (mid.mid, hi.lo, lo.hi; first factor K resp. P,
            second Q resp. V, as mfma_x6 is called) whose loss a bound must not let through.

Bounds (x6_bounds) for the f32 kernels, three-plane and f32-instruction alike: whole tensor and worst row, each the smaller
of 3e-5 (test_encoder_attention's f32 figure) and HALF the smallest error among the three five-product emulations on the
case's own inputs.  A case `distinguishes` if the six-product emulation is under a QUARTER of both bounds (and each
five-product emulation is then at least twice its bound).  A case that does not keeps 3e-5 and is listed in
CANNOT_TELL_FIVE_FROM_SIX: uniform (P = 1: its mid and lo planes are zero, two of the three small products vanish),
one_hot (P is one-hot, Q and K are single-plane values: likewise) and large (Q, K and V are single-plane values: only
lo.hi of P V is left, mid.mid and hi.lo vanish).
"""
import math

import torch

CASES = ("random", "rising", "falling", "one_hot", "uniform", "large")
CANNOT_TELL_FIVE_FROM_SIX = ("one_hot", "uniform", "large")
F32_TOL = 3e-5                                           # tests/test_gpu_kernels.py: test_encoder_attention, f32
BF16_TOL = 1e-2                                          # the same test, bf16
SIX = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))   # mm, hl, lh, hm, mh, hh: the kernels' order
DROPS = {"mid.mid": (1, 1), "hi.lo": (0, 2), "lo.hi": (2, 0)}
GEOMETRIES = [(B, T, H) for T in (256, 512) for H in (1, 6, 12) for B in (1, 3)]       # random
SCRIPTED_GEOMETRIES = [(B, T, H) for T in (256, 512) for B, H in ((3, 6), (1, 12))]     # every other case
ONE_HOT_LOGIT = 128.0


def permutation(T):
    """pi: query -> preferred key.  Even queries go to the first half of the keys, odd ones to the second; inside a half
    the key index is an odd multiple of the query pair's number, so a tile of 16 queries is spread over the half."""
    i = torch.arange(T)
    return (i & 1) * (T // 2) + ((i >> 1) * 37 + 11) % (T // 2)


def make_case(name, B, T, H, seed=0):
    """-> qkv f32 [B][T][3][H][64] on the CPU"""
    g = torch.Generator().manual_seed(1000 * CASES.index(name) + 7 * T + 3 * H + B + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    qkv = rn(B, T, 3, H, 64)
    if name == "random":
        qkv[:, :, 0] *= 0.35                               # unscaled logits: keep the softmax non-degenerate
    elif name in ("rising", "falling"):
        u = rn(B, 1, H, 64)
        u = u / u.norm(dim=-1, keepdim=True)
        sign = 1.0 - 2.0 * (torch.arange(T) % 2).double()
        a = (sign * math.sqrt(3.0) * (0.5 + torch.rand(T, generator=g, dtype=torch.float64))).view(1, T, 1, 1)
        c = math.sqrt(3.0) * (2.0 * (torch.arange(T).double() + 0.5) / T - 1.0)
        c = (c if name == "rising" else -c).view(1, T, 1, 1)
        qkv[:, :, 0] = a * u + 0.015 * qkv[:, :, 0]
        qkv[:, :, 1] = c * u + 0.015 * qkv[:, :, 1]
    elif name == "one_hot":
        k = torch.where(qkv[:, :, 1] < 0, -1.0, 1.0).double()
        qkv[:, :, 1] = k
        qkv[:, :, 0] = (ONE_HOT_LOGIT / 64) * k[:, permutation(T)]
    elif name == "uniform":
        qkv[:, :, 0] = 0.0
        order = (torch.arange(T) * 101 + 7) % T            # the ramp, visited in a scattered order: partial sums stay small
        z = (2.0 * (order.double() + 0.5) / T - 1.0).view(1, T, 1, 1)
        m = (0.02 + 0.02 * torch.rand(B, 1, H, 64, generator=g, dtype=torch.float64)) * torch.where(rn(B, 1, H, 64) < 0, -1.0, 1.0)
        qkv[:, :, 2] = m + z
    elif name == "large":
        sigma = math.sqrt(30.0 / math.sqrt(63.0))          # 63 free dimensions: logit sd = sqrt(63) sigma^2 = 30
        grid = lambda x: (torch.round(x * sigma * 4) / 4).clamp(-8, 8)
        qkv[:, :, 0], qkv[:, :, 1] = grid(qkv[:, :, 0]), grid(qkv[:, :, 1])
        qkv[:, :, 0, 1::2, 0], qkv[:, :, 1, 1::2, 0] = 16.0, -24.0
        qkv[:, :, 2] = qkv[:, :, 2].bfloat16().double()
    else:
        raise ValueError(name)
    return qkv.float()


# ------------------------------------------------------------------------------------------------ reference and models
def round_ct(x, ct):
    """float64 -> ct (round to nearest even) -> float64; ct None: unchanged"""
    return x if ct is None else x.to(ct).double()


def _heads(t):
    """[B][T][H][64] -> float64 [B * H][T][64]"""
    B, T, H, D = t.shape
    return t.double().permute(0, 2, 1, 3).reshape(B * H, T, D)


def _unheads(o, B, H):
    """[B * H][T][64] -> [B][T][H][64]"""
    return o.view(B, H, o.shape[1], o.shape[2]).permute(0, 2, 1, 3).contiguous()


def _groups(n, T):
    """head ranges whose [heads][T][T] float64 matrices stay at 8 MB"""
    step = max(1, (1 << 20) // (T * T))
    return [slice(i, min(n, i + step)) for i in range(0, n, step)]


def split_qkv(qkv):
    """qkv [B][T][3][H][64] -> q, k, v [B][T][H][64] (views)"""
    return qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]


def logits(q, k):
    """float64 [B * H][T queries][T keys]; for the CPU test's properties (small launches only)"""
    return torch.einsum("nqd,nkd->nqk", _heads(q), _heads(k))


def attention_ref(q, k, v, p_dtype=None, out_dtype=None):
    """q, k, v [B][T][H][64] in any float type (the values as the kernel reads them) -> float64 [B][T][H][64].  With
    p_dtype / out_dtype the bf16 error model (module docstring); with both None the reference."""
    B, T, H, _ = q.shape
    qh, kh, vh = _heads(q), _heads(k), _heads(v)
    out = torch.empty_like(qh)
    for g in _groups(B * H, T):
        s = torch.einsum("nqd,nkd->nqk", qh[g], kh[g])
        p = torch.exp(s - s.amax(-1, keepdim=True))
        l = p.sum(-1, keepdim=True)
        out[g] = torch.einsum("nqk,nkd->nqd", round_ct(p, p_dtype), vh[g]) / l
    return round_ct(_unheads(out, B, H), out_dtype)


def model_bf16(q, k, v):
    return attention_ref(q, k, v, p_dtype=torch.bfloat16, out_dtype=torch.bfloat16)


def planes(x):
    """f32 values (given in any type that holds them) -> their (hi, mid, lo) bf16 planes as float64"""
    x = x.float()
    hi = x.bfloat16().float()
    r1 = x - hi                                            # exact in f32
    mid = r1.bfloat16().float()
    lo = (r1 - mid).bfloat16().float()                     # r1 - mid exact in f32
    return hi.double(), mid.double(), lo.double()


def _plane_product(eq, a, b, terms):
    """sum over (i, j) in terms of einsum(eq, a[i], b[j]) in float64.  Plane sums are exact in float64 (three 8-bit terms
    inside 24 bits), so first factors that meet the same second factors are added up before the product."""
    by_i = {}
    for i, j in terms:
        by_i.setdefault(i, []).append(j)
    merged = {}
    for i, js in by_i.items():
        merged.setdefault(tuple(sorted(js)), []).append(i)
    return sum(torch.einsum(eq, sum(a[i] for i in is_), sum(b[j] for j in js)) for js, is_ in merged.items())


def plane_attention(q, k, v, drop=None):
    """the three-plane kernel's arithmetic with float64 sums: the product set SIX, or SIX without DROPS[drop]"""
    terms = [t for t in SIX if drop is None or t != DROPS[drop]]
    B, T, H, _ = q.shape
    qh, kh, vh = _heads(q), _heads(k), _heads(v)
    out = torch.empty_like(qh)
    for g in _groups(B * H, T):
        s = _plane_product("nkd,nqd->nqk", planes(kh[g]), planes(qh[g]), terms)     # K is the first factor
        p = torch.exp(s - s.amax(-1, keepdim=True)).float()
        l = p.double().sum(-1, keepdim=True)
        out[g] = _plane_product("nqk,nkd->nqd", planes(p), planes(vh[g]), terms) / l
    return _unheads(out, B, H)


# -------------------------------------------------------------------------------------------------------------- errors
def rel(got, ref):
    """whole-tensor rel-L2"""
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def row_rel(got, ref):
    """[B][T][H]: per query row of one head, the error over its 64 columns relative to that row's norm"""
    return (got.double() - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)


def worst_row(got, ref):
    return float(row_rel(got, ref).max())


def x6_bounds(qkv, ref=None):
    """qkv f32 [B][T][3][H][64] -> dict: `whole`, `row` (the bounds), `six` = (whole, worst row) of the six-product
    emulation, `five` = {name: (whole, worst row)}, `half_five` = (whole, row) before the cap at F32_TOL,
    `distinguishes` (module docstring)"""
    q, k, v = split_qkv(qkv)
    ref = attention_ref(q, k, v) if ref is None else ref
    err = lambda o: (rel(o, ref), worst_row(o, ref))
    six = err(plane_attention(q, k, v))
    five = {name: err(plane_attention(q, k, v, drop=name)) for name in DROPS}
    half = tuple(0.5 * min(e[i] for e in five.values()) for i in (0, 1))
    ok = six[0] < half[0] / 4 and six[1] < half[1] / 4
    whole, row = (min(F32_TOL, half[0]), min(F32_TOL, half[1])) if ok else (F32_TOL, F32_TOL)
    return dict(whole=whole, row=row, six=six, five=five, half_five=half, distinguishes=ok)


def bf16_row_factor(q, k, v, ref=None):
    """the factor by which the worst row of the bf16 error model exceeds the model's whole-tensor error (>= 1), and the
    two figures; q, k, v hold bf16 values.  A model whose worst row is exact to 2^-20 has no rounding to take a ratio of: 1."""
    ref = attention_ref(q, k, v) if ref is None else ref
    model = model_bf16(q, k, v)
    whole, row = rel(model, ref), worst_row(model, ref)
    if row < 2.0 ** -20:                                   # the model is exact on this case (one_hot): rows get the whole bound
        return 1.0, whole, row
    return max(1.0, row / whole), whole, row


def running_max_moves(s):
    """s float64 [n][T queries][T keys] -> bool [n][T][T / 64 - 1]: does the running maximum over 64-key chunks change at
    the boundary into chunk c + 1"""
    n, T, _ = s.shape
    cm = s.view(n, T, T // 64, 64).amax(-1)
    run = torch.cummax(cm, -1)[0]
    return run[..., 1:] > run[..., :-1]
