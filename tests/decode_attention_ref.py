"""Float64 reference of the decode-attention launch in every form the decode loop uses it (mt3_op_decode_attention_ex),
written from the rule in mt3_amd/csrc/kernels.h (DecAttnArgs) and include/mt3_hip.h, in torch on whatever device the
inputs live on.  Per slot b that is not done:

  row scale     rs = 1 / sqrt(sum(q_ss[b]) / (16 * q_ss_n) + 1e-6)        (folded form; 1 in the plain form)
  query, rows   round_ct(raw * rs): bf16 round-to-nearest-even or f32      (plain form: the rows as given)
  e4m3 caches   the rounded K / V row goes through fp8_quantize_quad's rule (_fp8_quant_ref) and is attended DEQUANTISED
  attention     softmax over keys 0 .. step[b] of cache row cache_row[b] (the new row at position step[b]; without new
                rows: over keys 0 .. n - 1 as they are), unscaled logits, then P . V

Also here: the scripted partial sums of squares the GPU tests feed the folded form with (checked on the CPU in
tests/test_decode_attention_ref.py).
"""
import torch

F8 = torch.float8_e4m3fn


def _fp8_quant_ref(x):
    """rows [..., 64] (any float dtype) -> (uint8 e4m3fn bytes, power-of-two scale, dequantised f64): the rule of
    fp8_quantize_quad: scale = 2^(exponent(amax) - 7) so that amax / scale is in [128, 256)."""
    x = x.float()
    amax = x.abs().amax(-1, keepdim=True)
    e = torch.frexp(amax)[1].float() - 1                      # amax = m * 2^e, m in [1, 2)
    scale = torch.where(amax > 0, torch.exp2(e - 7), torch.ones_like(amax))
    q = (x / scale).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale.squeeze(-1), q.float().double() * scale.double()


def round_ct(x, ct):
    """float64 -> the compute type (round to nearest even) -> float64"""
    return x.double().to(ct).double()


def row_scales(q_ss):
    """q_ss [B][n] partial sums of squares of a residual row of 16 * n columns -> 1 / rms, float64 [B]"""
    n = q_ss.shape[-1]
    return 1.0 / torch.sqrt(q_ss.double().sum(-1) / (16 * n) + 1e-6)


def dequant(cache, scale):
    """e4m3 bytes [..., 64] and their scales [...] -> float64"""
    return cache.view(F8).float().double() * scale.double().unsqueeze(-1)


def decode_attention_ref(ct, kcache, vcache, *, q=None, q_f32=None, q_ss=None, new_k=None, new_v=None, step=None,
                         n_keys=None, kv_scale=None, done=None, cache_row=None, p_dtype=None):
    """One launch.  kcache / vcache [R][H][cap][64] of the compute type `ct`, or uint8 e4m3 bytes with kv_scale
    [R][H][cap][2] = {k_scale, v_scale}.  Plain form: q (and new_k / new_v) [B][H][64] of `ct`; folded form: q_f32 (and
    new_k / new_v) [B][H][64] unnormalised f32 with q_ss [B][n].  step [B] (keys 0 .. step[b]) or n_keys for all; done /
    cache_row [B] or None.  p_dtype: round the softmax weights and the result to it (an ERROR MODEL of a low-precision
    evaluation, used to size per-row bounds; None: exact).
    Returns (out float64 [B][H][64], NaN rows for done slots; kcache, vcache, kv_scale after the call; rs float64 [B])."""
    fold = q_f32 is not None
    qsrc = q_f32 if fold else q
    B, H = qsrc.shape[0], qsrc.shape[1]
    K, V = kcache.clone(), vcache.clone()
    S = kv_scale.clone() if kv_scale is not None else None
    rs = row_scales(q_ss) if fold else torch.ones(B, dtype=torch.float64, device=qsrc.device)
    lst = lambda t: None if t is None else [int(v) for v in t.tolist()]
    step_l, done_l, row_l = lst(step), lst(done), lst(cache_row)
    out = torch.full((B, H, 64), float("nan"), dtype=torch.float64, device=qsrc.device)

    def form(x, b):
        return round_ct(x[b].double() * rs[b], ct) if fold else x[b].double()

    for b in range(B):
        if done_l is not None and done_l[b]:
            continue                                           # before anything of the slot is looked at, its step included
        r = row_l[b] if row_l is not None else b
        n = step_l[b] + 1 if step_l is not None else n_keys
        qb = form(qsrc, b)
        if new_k is not None:
            kn, vn = form(new_k, b), form(new_v, b)
            if S is not None:
                kb, ks, _ = _fp8_quant_ref(kn)
                vb, vs, _ = _fp8_quant_ref(vn)
                K[r, :, n - 1], V[r, :, n - 1] = kb, vb
                S[r, :, n - 1, 0], S[r, :, n - 1, 1] = ks, vs
            else:
                K[r, :, n - 1], V[r, :, n - 1] = kn.to(K.dtype), vn.to(V.dtype)
        if S is not None:
            Kd, Vd = dequant(K[r, :, :n], S[r, :, :n, 0]), dequant(V[r, :, :n], S[r, :, :n, 1])
        else:
            Kd, Vd = K[r, :, :n].double(), V[r, :, :n].double()
        w = torch.softmax(torch.einsum("hd,hkd->hk", qb, Kd), -1)
        if p_dtype is not None:
            w = round_ct(w, p_dtype)
        o = torch.einsum("hk,hkd->hd", w, Vd)
        out[b] = o if p_dtype is None else round_ct(o, p_dtype)
    return out, K, V, S, rs


def scripted_partial_sums(B, n, seed, shift=0, dominance=15.0):
    """q_ss [B][n] f32, independent of any q: per row n - 1 values drawn log-uniformly over four decades (1e-4 .. 1) and
    ONE dominant group at index (row * 5 + shift) % n holding `dominance` times the sum of the others.  A sum that loses
    the dominant group shrinks 16-fold (rs x 4), one that counts it twice grows 1.9-fold (rs / 1.39), one that loses
    any other float4 of a row changes by that float4's share."""
    g = torch.Generator().manual_seed(seed)
    ss = torch.pow(10.0, torch.rand(B, n, generator=g, dtype=torch.float64) * 4.0 - 4.0)
    idx = dominant_index(B, n, shift)
    rows = torch.arange(B)
    ss[rows, idx] = 0.0
    ss[rows, idx] = dominance * ss.sum(-1)
    return ss.float()


def dominant_index(B, n, shift=0):
    return (torch.arange(B) * 5 + shift) % n
