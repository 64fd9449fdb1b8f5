"""The decode-attention kernels in the forms the decode loop launches them in, through mt3_op_decode_attention_ex,
against the float64 reference of tests/decode_attention_ref.py:

  the FOLDED query  (q_f32 / q_ss / q_ss_n: unnormalised f32 q -- with append also K and V rows -- plus the partial sums of
                    squares of the residual row; the kernel forms 1/rms, scales, rounds to the compute type, persists)
  ROW RETIREMENT    (done / cache_row: a done slot's workgroup returns at once, a live slot works in row cache_row[b])

Which test launches which instantiation launch_decode_attention can select (CT = bf16 and f32 alike):

  dec_attn_kernel<CT, append, 3, folded>        test_folded_append, test_folded_append_small_cap, test_retirement[*-folded-append-*]
  dec_attn_kernel<CT, cross,  3, folded>        test_folded_cross, test_retirement[*-folded-cross-map]
  dec_attn_kernel<CT, append, 3>  (plain)       test_retirement[*-plain-append-*]; the plain launches of test_folded_append
  dec_attn_kernel<CT, cross,  3>  (plain)       test_retirement[*-plain-cross-map]; the plain launches of test_folded_cross
  dec_attn_fp8_kernel<append, 3, 3, 2>          the e4m3 cases of the append tests: a.q_f32 branch = folded, else plain
  dec_attn_fp8_kernel<cross, 4, 2, 2>           the e4m3 cases of the cross tests, likewise

The partial sums are SCRIPTED and independent of q (the kernel never relates the two): per row one dominant group at
index (row * 5 + shift) % q_ss_n, the others log-uniform over four decades (decode_attention_ref.scripted_partial_sums).
Over twelve rows and shift in {0, 8} the dominant group sits on every lane's float4 of the first DPP row, so a 1/rms that
drops a float4 is off by a factor 4 in some row.  The raw rows are scaled so that raw * rs has the 0.35 (q) / 1.0 (K, V)
standard deviation of the plain-form tests.

Bounds.  rs: the kernel's f32 1/rms may differ from the float64 one by RS = 5 * 2^-24 relative (1 ulp v_rsq_f32, 1 the
division and the add, 2 the f32 sum of <= 64 positive terms in an order the test does not fix, 1 the product); a stored
element x of the appended row therefore satisfies |x - raw rs64| <= u + RS |raw rs64| with u half an ulp of the compute
type at that value: 2^(exponent - 8) for bf16 (8 significant bits, <= 2^-8 relative; a bound of 2^-9 relative is missed by
the float64 -> bf16 rounding of the reference itself, worst 3.85e-3 on these inputs), 0 for f32.  `out`: the
tolerances of the plain-form tests of the same kernels (tests/test_gpu_kernels.py: rel-L2 5e-3 bf16 / e4m3, 2e-5 f32) on
the whole tensor, and PER ROW that tolerance times the factor by which the worst row exceeds the whole tensor in an error
model of the same inputs: the float64 reference with the softmax weights and the result rounded to the compute type
(bf16 for e4m3).  That factor is computed, not measured (1.07 - 2.16 over the cases of this file).
Measured on MI355X (every case prints its own): see MEASURED below.
"""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import decode_attention_ref as R  # noqa: E402

H, HD = 6, 6 * 64
KINDS = ("bf16", "f32", "e4m3")
TOL = {"bf16": 5e-3, "f32": 2e-5, "e4m3": 5e-3}          # rel-L2 of `out`: tests/test_gpu_kernels.py, the same kernels
RS = 5 * 2.0 ** -24
# MEASURED on MI355X over all cases of this file: worst whole-tensor rel-L2, worst single row (smallest per-row bound);
# the f32 appended rows use at most 0.51 of the RS budget, the bf16 ones reach their half ulp (ties of the rounding)
MEASURED = {"bf16": "1.66e-3, 1.77e-3 (5.4e-3)", "f32": "2.9e-7, 4.6e-7 (2.3e-5)", "e4m3": "1.72e-3, 1.89e-3 (5.7e-3)"}
STEPS_256 = [0, 1, 47, 48, 49, 95, 96, 97, 239, 240, 241, 255]   # straddle the key groups: 48 (f32), 96 (bf16, e4m3), 96 + 144
STEPS_40 = [0, 1, 38, 39] * 3                                    # cap 40: every speculative load is clamped to cap - 1
# (q_ss_n, shift) -> seed of the raw rows: chosen on the CPU so that the bf16 rounding of raw * rs is the same for every
# rs inside the RS budget in all twelve rows, with and without the e4m3 peaks (consistency with the plain form needs >= 90 %)
SS_CASES = [(4, 0), (32, 0), (48, 0), (64, 0), (48, 8), (64, 8)]
SEEDS = {c: 22 for c in SS_CASES}                      # 12 of 12 rows for every case, bf16 and e4m3 inputs alike


def ct_of(kind):
    return torch.float32 if kind == "f32" else torch.bfloat16


def bits(t):
    """the tensor's bytes as integers (NaN patterns compare like any other; e4m3 bytes: -0 is 0, compared as values)"""
    if t.dtype == torch.uint8:
        return torch.where(t == 0x80, torch.zeros_like(t), t)
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-30))


def launch(kind, **f):
    """one mt3_op_decode_attention_ex call; tensors or raw addresses for the pointers"""
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    ints = ("q_stride", "cap", "kv_stride", "n_keys", "B", "H", "q_ss_n")
    v = _lib.DecAttnView(**{k: (int(x) if k in ints else ptr(x)) for k, x in f.items()})
    rc = _lib.load().mt3_op_decode_attention_ex(_lib.MT3_F32 if kind == "f32" else _lib.MT3_BF16, C.byref(v),
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(rc)
    return rc


# ------------------------------------------------------------------------------------------------------------ inputs
def folded_rows(kind, B, n, shift, seed, exact=False):
    """-> (qkvf f32 [B][4][H][64] = raw q | k | v | cross-q, the engine's own buffer; q_ss f32 [B][n]; rs float64 [B]),
    on the CPU.  e4m3: every K and V row's largest |raw * rs| is 1.5 x a power of two (the quantisation scale of the row
    is then the same for every rs inside the budget).  exact: raw * rs sits ON bf16 values, so its rounding to bf16 is
    the same for every rs inside the budget in every element."""
    ss = R.scripted_partial_sums(B, n, seed, shift)
    rs = R.row_scales(ss)
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.randn(B, 4, H, 64, generator=g, dtype=torch.float64)
    t[:, 0] *= 0.35                                        # unscaled logits: keep the softmax non-degenerate
    t[:, 3] *= 0.35
    if kind == "e4m3":
        amax = t[:, 1:3].abs().amax(-1, keepdim=True)
        t[:, 1:3] *= 1.5 * torch.exp2(torch.floor(torch.log2(amax))) / amax
    if exact:
        t = t.to(torch.bfloat16).double()
    return (t / rs[:, None, None, None]).float(), ss, rs


def unambiguous_rows(raw, rs, ct=torch.bfloat16):
    """rows [B] of raw [B][...] whose rounding of raw * rs to `ct` does not depend on where inside the RS budget the
    kernel's rs lies (computed from the float64 rs alone)"""
    x = raw.double().flatten(1) * rs[:, None]
    return (R.round_ct(x * (1 - RS), ct) == R.round_ct(x * (1 + RS), ct)).all(-1)


def rs_f32_like_the_rule(ss):
    """rsqrt(sum / (16 n) + 1e-6) in f32 on the GPU, the sum as a pairwise tree over groups of four (each op rounded once)"""
    B, n = ss.shape
    p = torch.zeros(B, 64, device=ss.device)
    p[:, :n] = ss
    p = p.view(B, 16, 4)
    s = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    tot = s[:, 0]
    return torch.rsqrt(tot / torch.full_like(tot, 16.0 * n) + torch.full_like(tot, 1e-6))


def rs_candidates(kind, ss, rs):
    """the test's f32 row scales: bf16 / e4m3 rows are decided by the rounding, any rs inside the budget does; f32: the
    test's f32 evaluation of the rule and its neighbours one ulp down and up"""
    if kind != "f32":
        return [rs.float()]
    r = rs_f32_like_the_rule(ss)
    return [r, torch.nextafter(r, torch.zeros_like(r)), torch.nextafter(r, torch.full_like(r, 1e30))]


def make_caches(kind, rows, cap, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(rows, H, cap, 64, generator=g).cuda()
    v = torch.randn(rows, H, cap, 64, generator=g).cuda()
    if kind != "e4m3":
        return k.to(ct_of(kind)), v.to(ct_of(kind)), None
    kb, ks, _ = R._fp8_quant_ref(k * 1.3)
    vb, vs, _ = R._fp8_quant_ref(v * 0.7)
    return kb.clone(), vb.clone(), torch.stack([ks, vs], -1).contiguous()


def poison_tails(kind, kc, vc, sc, rows, steps, tail):
    """what lies at and past position steps[i] of cache row rows[i]: NaN / Inf patterns (what torch.empty may hand out)"""
    for r, n in zip(rows, steps):
        if kind == "e4m3":
            kc[r, :, n:] = 0x7F if tail == "nan" else 0xFF                          # e4m3fn NaN patterns
            vc[r, :, n:] = 0xFF if tail == "nan" else 0x7F
            sc[r, :, n:] = float(tail)
        else:
            kc[r, :, n:] = float(tail)
            vc[r, :, n:] = float("nan") if tail == "nan" else float("-inf")


def check_out(kind, what, out, ref, model):
    """whole-tensor rel-L2 under the plain-form tolerance and every row under that tolerance times the worst-row factor
    of the error model (module docstring)"""
    whole = rel(out, ref)
    rows = [rel(out[b], ref[b]) for b in range(ref.shape[0])]
    m_whole = rel(model, ref)
    m_rows = max(rel(model[b], ref[b]) for b in range(ref.shape[0]))
    factor = max(1.0, m_rows / max(m_whole, 1e-300))
    print(f"{what}: out rel-L2 {whole:.3e} (bound {TOL[kind]:.0e}), worst row {max(rows):.3e} (bound "
          f"{TOL[kind] * factor:.3e}: error model worst row / whole = {m_rows:.3e} / {m_whole:.3e} = {factor:.2f})")
    assert torch.isfinite(out.float()).all(), what
    assert whole < TOL[kind], (what, whole)
    assert max(rows) < TOL[kind] * factor, (what, rows, factor)


def half_ulp(kind, x):
    """half the spacing of the compute type's values around x: bf16 has 8 significant bits, so 2^(exponent - 8); 0 for
    f32, whose rounding is part of the RS budget"""
    if kind == "f32":
        return torch.zeros_like(x)
    return torch.exp2(torch.frexp(x.abs().clamp_min(2.0 ** -126))[1].double() - 1 - 8)


def e4m3_spacing(y):
    """spacing of the e4m3fn values around |y| (normal down to 2^-6, 3 mantissa bits; below: 2^-9)"""
    e = torch.frexp(y.abs().clamp_min(2.0 ** -6))[1].double() - 1
    return torch.exp2(e - 3)


# -------------------------------------------------------------------------------------------- the folded form, append
def run_folded_append(kind, cap, steps, n, shift):
    B = len(steps)
    ct = ct_of(kind)
    seed = SEEDS[(n, shift)]
    raw_c, ss_c, rs_c = folded_rows(kind, B, n, shift, seed)
    what = f"folded append {kind} cap {cap} q_ss_n {n} shift {shift}"
    # (5, its condition) the share of rows the reference rounding alone decides, from the CPU
    fixed = unambiguous_rows(raw_c[:, :3], rs_c) if kind != "f32" else None
    if fixed is not None:
        assert float(fixed.double().mean()) >= 0.9, (what, fixed)
    qkvf, ss, rs = raw_c.cuda().view(B, 4 * HD), ss_c.cuda(), rs_c.cuda()
    raw = qkvf.view(B, 4, H, 64)
    step = torch.tensor(steps, device="cuda", dtype=torch.int32)
    base = make_caches(kind, B, cap, seed=7)
    runs = {}
    for tail in ("clean", "nan", "inf"):
        kc, vc, sc = (t.clone() if t is not None else None for t in base)
        if tail != "clean":
            poison_tails(kind, kc, vc, sc, range(B), steps, tail)
        pre = tuple(t.clone() if t is not None else None for t in (kc, vc, sc))
        out = torch.full((B, HD), -7.5, device="cuda", dtype=ct)
        launch(kind, q_f32=qkvf, q_stride=4 * HD, q_ss=ss, q_ss_n=n, kcache=kc, vcache=vc, kv_scale=sc, cap=cap,
               new_k=qkvf.data_ptr() + HD * 4, new_v=qkvf.data_ptr() + 2 * HD * 4, kv_stride=4 * HD, step=step, out=out,
               B=B, H=H)
        runs[tail] = (out.view(B, H, 64), kc, vc, sc, pre)
    idx = torch.arange(B, device="cuda")
    pos = step.long()
    want_k, want_v = raw[:, 1].double() * rs[:, None, None], raw[:, 2].double() * rs[:, None, None]
    for tail, (out, kc, vc, sc, pre) in runs.items():
        # (1, 2) everything but the appended row (and its scale pair) keeps its bits
        for got, was in zip((kc, vc, sc), pre):
            if got is None:
                continue
            exp = was.clone()
            exp[idx, :, pos] = got[idx, :, pos]
            assert same(got, exp), (what, tail, "a cache byte outside the appended row changed")
        for name, got, want in (("K", kc, want_k), ("V", vc, want_v)):
            row = got[idx, :, pos]
            if kind != "e4m3":
                # (1) the stored row: raw * rs rounded to the compute type, rs inside its budget
                err = (row.double() - want).abs()
                lim = half_ulp(kind, want) + RS * want.abs()
                worst = float((err / lim).max())
                if tail == "clean":
                    print(f"{what}: appended {name} row, worst |x - raw rs64| = {worst:.3f} of its bound "
                          f"(half an ulp of the compute type + {RS:.2e} |raw rs64|)")
                assert bool((err <= lim).all()), (what, tail, name, worst)
            else:
                # (2) the scale pair bit for bit, the dequantised row within one e4m3 spacing of the bf16-rounded value
                refb = R.round_ct(want, torch.bfloat16)
                _, scale, _ = R._fp8_quant_ref(refb)
                col = 0 if name == "K" else 1
                assert same(sc[idx, :, pos][..., col], scale), (what, tail, name, "scale")
                deq = R.dequant(row, scale)
                lim = e4m3_spacing(refb / scale.double()[..., None]) * scale.double()[..., None]
                assert bool(((deq - refb).abs() <= lim).all()), (what, tail, name, float(((deq - refb).abs() / lim).max()))
    out, kc, vc, sc, pre = runs["clean"]
    # (3) out against the float64 reference (e4m3: over the dequantised cache as the kernel left it, checked above)
    if kind == "e4m3":
        args = dict(q=R.round_ct(raw[:, 0].double() * rs[:, None, None], ct), kv_scale=sc, step=step)
        ref = R.decode_attention_ref(ct, kc, vc, **args)[0]
        model = R.decode_attention_ref(ct, kc, vc, p_dtype=ct, **args)[0]
    else:
        args = dict(q_f32=raw[:, 0], q_ss=ss, new_k=raw[:, 1], new_v=raw[:, 2], step=step)
        ref = R.decode_attention_ref(ct, pre[0], pre[1], **args)[0]
        model = R.decode_attention_ref(ct, pre[0], pre[1], p_dtype=ct, **args)[0]
    check_out(kind, what, out, ref, model)
    # (6) NaN / Inf past each row's length change nothing
    for tail in ("nan", "inf"):
        assert same(runs[tail][0], out), (what, tail)
        for b in range(B):                                                          # nor the row the launch appended
            for i in (1, 2, 3):
                if runs[tail][i] is not None:
                    assert same(runs[tail][i][b, :, steps[b]], runs["clean"][i][b, :, steps[b]]), (what, tail, b)
    # (5) the plain form over round_ct(raw * rs), computed by the test in f32, gives the same bits
    # (f32: the row IS the f32 product, so the test's rs has to be the kernel's to the bit; the test's own f32 evaluation
    # of the rule and its two f32 neighbours are tried, a row takes part with the candidate that reproduces its stored row)
    part = torch.zeros(B, dtype=torch.bool)
    for rs32 in rs_candidates(kind, ss, rs):
        rows3 = (raw[:, :3] * rs32[:, None, None, None]).to(ct).contiguous()        # [B][3][H][64] = q | k | v
        kc2, vc2, sc2 = (t.clone() if t is not None else None for t in base)
        out2 = torch.full((B, HD), -7.5, device="cuda", dtype=ct)
        es = rows3.element_size()
        launch(kind, q=rows3, q_stride=3 * HD, kcache=kc2, vcache=vc2, kv_scale=sc2, cap=cap,
               new_k=rows3.data_ptr() + HD * es, new_v=rows3.data_ptr() + 2 * HD * es, kv_stride=3 * HD, step=step, out=out2,
               B=B, H=H)
        stored_same = torch.tensor([all(same(a[b, :, steps[b]], c[b, :, steps[b]]) for a, c in
                                        ((kc, kc2), (vc, vc2), (sc, sc2)) if a is not None) for b in range(B)])
        if kind != "f32":
            assert bool(stored_same[fixed].all()), (what, "a row the rounding decides is stored differently", stored_same)
            stored_same = fixed
        for b in range(B):
            if stored_same[b]:
                assert same(out[b], out2.view(B, H, 64)[b]), (what, "plain form differs in row", b)
        part |= stored_same
    print(f"{what}: {int(part.sum())} of {B} rows take part in the plain-form comparison")
    assert float(part.double().mean()) >= 0.9, (what, part)


@pytest.mark.parametrize("kind", KINDS)
def test_folded_append_single_key_row_is_the_stored_v_row(kind):
    """step == 0: the softmax has one key, so out[b] is the stored V row bit for bit (e4m3: the bf16 rounding of its
    dequantised value).  f32 shows every bit: the weight of the only key has to be exactly exp2(0) (the scaled logit is
    rounded once, attention.hip: log2e_logit; contracted into the subtraction of the maximum it gave 1 +- 1 ulp and 313
    of 4608 elements one ulp off)."""
    B, n, cap = 12, 32, 256
    ct = ct_of(kind)
    raw_c, ss_c, _ = folded_rows(kind, B, n, 0, SEEDS[(n, 0)])
    qkvf, ss = raw_c.cuda().view(B, 4 * HD), ss_c.cuda()
    step = torch.zeros(B, device="cuda", dtype=torch.int32)
    kc, vc, sc = make_caches(kind, B, cap, seed=7)
    out = torch.full((B, HD), -7.5, device="cuda", dtype=ct)
    launch(kind, q_f32=qkvf, q_stride=4 * HD, q_ss=ss, q_ss_n=n, kcache=kc, vcache=vc, kv_scale=sc, cap=cap,
           new_k=qkvf.data_ptr() + HD * 4, new_v=qkvf.data_ptr() + 2 * HD * 4, kv_stride=4 * HD, step=step, out=out, B=B, H=H)
    stored = vc[:, :, 0] if kind != "e4m3" else R.dequant(vc[:, :, 0], sc[:, :, 0, 1]).to(ct)
    diff = int((bits(out.view(B, H, 64)) != bits(stored)).sum())
    print(f"single-key rows {kind}: {diff} of {stored.numel()} elements of out differ from the stored V row")
    assert diff == 0, diff


@pytest.mark.parametrize("n,shift", SS_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_folded_append(kind, n, shift):
    run_folded_append(kind, 256, STEPS_256, n, shift)


@pytest.mark.parametrize("kind", KINDS)
def test_folded_append_small_cap(kind):
    run_folded_append(kind, 40, STEPS_40, 32, 0)


# --------------------------------------------------------------------------------------------- the folded form, cross
CROSS_CASES = [(k, 256, False, n, s) for k in KINDS for n, s in SS_CASES] + [(k, 256, True, 32, 0) for k in KINDS] + \
              [(k, 512, False, 48, 0) for k in ("bf16", "e4m3")]


@pytest.mark.parametrize("kind,T,dense,n,shift", CROSS_CASES)
def test_folded_cross(kind, T, dense, n, shift):
    B = 12
    ct = ct_of(kind)
    raw_c, ss_c, rs_c = folded_rows(kind, B, n, shift, SEEDS[(n, shift)])
    what = f"folded cross {kind} T {T} {'dense' if dense else 'strided'} q_ss_n {n} shift {shift}"
    fixed = unambiguous_rows(raw_c[:, 3], rs_c) if kind != "f32" else None
    if fixed is not None:
        assert float(fixed.double().mean()) >= 0.9, (what, fixed)
    qkvf, ss, rs = raw_c.cuda().view(B, 4 * HD), ss_c.cuda(), rs_c.cuda()
    raw_q = qkvf.view(B, 4, H, 64)[:, 3]
    qd = raw_q.reshape(B, HD).contiguous()
    kc, vc, sc = make_caches(kind, B, T, seed=11)
    pre = tuple(t.clone() if t is not None else None for t in (kc, vc, sc))
    out = torch.full((B, HD), -7.5, device="cuda", dtype=ct)
    launch(kind, q_f32=qd if dense else qkvf.data_ptr() + 3 * HD * 4, q_stride=HD if dense else 4 * HD, q_ss=ss, q_ss_n=n,
           kcache=kc, vcache=vc, kv_scale=sc, cap=T, n_keys=T, out=out, B=B, H=H)
    for got, was in zip((kc, vc, sc), pre):
        assert got is None or same(got, was), (what, "a cross-attention launch wrote to a cache")
    args = dict(q_f32=raw_q, q_ss=ss, n_keys=T, kv_scale=sc)
    ref = R.decode_attention_ref(ct, kc, vc, **args)[0]
    model = R.decode_attention_ref(ct, kc, vc, p_dtype=ct, **args)[0]
    check_out(kind, what, out.view(B, H, 64), ref, model)
    # the plain form over round_ct(raw * rs): the same bits
    # (f32: nothing is stored to tell the kernel's own rs from; a row takes part with the candidate rs that reproduces it)
    agree = torch.zeros(B, dtype=torch.bool)
    for rs32 in rs_candidates(kind, ss, rs):
        q = (raw_q * rs32[:, None, None]).to(ct).contiguous()
        out2 = torch.full((B, HD), -7.5, device="cuda", dtype=ct)
        launch(kind, q=q, q_stride=HD, kcache=kc, vcache=vc, kv_scale=sc, cap=T, n_keys=T, out=out2, B=B, H=H)
        agree |= torch.tensor([same(out[b], out2[b]) for b in range(B)])
    part = agree if kind == "f32" else fixed
    print(f"{what}: {int(part.sum())} of {B} rows take part in the plain-form comparison")
    assert float(part.double().mean()) >= 0.9, (what, part)
    assert bool(agree[part].all()), (what, "plain form differs", agree)


# ------------------------------------------------------------------------------------------------------- retirement
ROWS = 10
CACHE_ROW = [7, 2, 9, 0, 4, 5, 1]                        # not the identity; rows 3, 6 and 8 are nobody's
DONE = [0, 1, 0, 0, 1, 0, 1]
RET_CAP = 128
RET_STEPS = [0, 5, 47, 96, 100, 127, 3]
RET_T = 160
RET_CASES = [(k, f, "append", sc) for k in KINDS for f in ("plain", "folded")
             for sc in ("map", "identity", "all_done", "garbage_step")] + \
            [(k, f, "cross", "map") for k in KINDS for f in ("plain", "folded")]


@pytest.mark.parametrize("kind,form,mode,scenario", RET_CASES)
def test_retirement(kind, form, mode, scenario):
    """7 slots over caches of 10 rows.  Live slot b: out[b] = the reference over cache row cache_row[b], the appended row
    (e4m3: and its scale pair) at [cache_row[b], :, step[b]].  Done slot: out[b] and its cache row keep their bits.  The
    whole cache equals the reference's expected cache bit for bit (folded rows are built ON bf16 values, so their
    rounding is decided; the f32 folded row is the f32 product itself and is held to the RS budget instead).
    done without a map = the identity map; all slots done = nothing changes; a done slot's step entry may be garbage:
    the workgroup returns before it reads it."""
    B, n = 7, 32
    ct = ct_of(kind)
    append, fold = mode == "append", form == "folded"
    cap = RET_CAP if append else RET_T
    what = f"retirement {kind} {form} {mode} {scenario}"
    raw_c, ss_c, rs_c = folded_rows(kind, B, n, 0, seed=5, exact=True)
    qkvf, ss, rs = raw_c.cuda().view(B, 4 * HD), ss_c.cuda(), rs_c.cuda()
    raw = qkvf.view(B, 4, H, 64)
    rows_ct = (raw.double() * rs[:, None, None, None]).to(ct).contiguous()          # plain form: q | k | v | cross-q
    qi = 0 if append else 3
    done_l = [1] * B if scenario == "all_done" else DONE
    map_l = None if scenario == "identity" else CACHE_ROW
    steps = list(RET_STEPS)
    if scenario == "garbage_step":
        steps[1], steps[4], steps[6] = -1, cap + 5, -1                              # done slots: never read
    dev = lambda l, dt=torch.int32: None if l is None else torch.tensor(l, device="cuda", dtype=dt)
    step, done, cmap = dev(steps), dev(done_l), dev(map_l)
    kc, vc, sc = make_caches(kind, ROWS, cap, seed=13)
    pre = tuple(t.clone() if t is not None else None for t in (kc, vc, sc))
    out = torch.full((B, HD), -7.5, device="cuda", dtype=ct) + torch.arange(B, device="cuda").to(ct)[:, None]
    out0 = out.clone()
    f = dict(kcache=kc, vcache=vc, kv_scale=sc, cap=cap, out=out, B=B, H=H, done=done, cache_row=cmap)
    if fold:
        f.update(q_f32=qkvf.data_ptr() + qi * HD * 4, q_stride=4 * HD, q_ss=ss, q_ss_n=n)
        src, es, stride = qkvf, 4, 4 * HD
    else:
        f.update(q=rows_ct.data_ptr() + qi * HD * rows_ct.element_size(), q_stride=4 * HD)
        src, es, stride = rows_ct, rows_ct.element_size(), 4 * HD
    if append:
        f.update(new_k=src.data_ptr() + HD * es, new_v=src.data_ptr() + 2 * HD * es, kv_stride=stride, step=step)
    else:
        f.update(n_keys=cap)
    assert launch(kind, **f) == _lib.MT3_OK
    # the reference of the same launch
    rows = raw if fold else rows_ct.view(B, 4, H, 64)
    args = dict(kv_scale=pre[2], done=done_l, cache_row=map_l)
    args.update(dict(q_f32=rows[:, qi], q_ss=ss) if fold else dict(q=rows[:, qi]))
    args.update(dict(new_k=rows[:, 1], new_v=rows[:, 2], step=steps) if append else dict(n_keys=cap))
    args = {k: (torch.tensor(v) if isinstance(v, list) else v) for k, v in args.items()}
    ref, K, V, S, _ = R.decode_attention_ref(ct, pre[0], pre[1], **args)
    model = R.decode_attention_ref(ct, pre[0], pre[1], p_dtype=ct, **args)[0]
    live = [b for b in range(B) if not done_l[b]]
    dead = [b for b in range(B) if done_l[b]]
    row_of = lambda b: map_l[b] if map_l is not None else b
    # (2, 5) a done slot: out and the slot's cache row keep their bits
    for b in dead:
        assert same(out[b], out0[b]), (what, "out of done slot", b)
        for got, was in zip((kc, vc, sc), pre):
            assert got is None or same(got[row_of(b)], was[row_of(b)]), (what, "cache row of done slot", b)
    # (3) the whole cache: the reference's expected cache, bit for bit
    loose = fold and append and kind == "f32"
    for name, got, exp, was in (("K", kc, K, pre[0]), ("V", vc, V, pre[1]), ("scale", sc, S, pre[2])):
        if got is None:
            continue
        if loose:
            for b in live:
                r, p = row_of(b), steps[b]
                want = rows[b, 1 if name == "K" else 2].double() * rs[b]
                assert bool(((got[r, :, p].double() - want).abs() <= RS * want.abs()).all()), (what, name, b)
                exp[r, :, p] = got[r, :, p]
        assert same(got, exp), (what, name, "cache differs from the expected cache")
        touched = {row_of(b) for b in live} if append else set()
        for r in set(range(ROWS)) - touched:                                        # nobody's rows, done slots' rows, and
            assert same(got[r], was[r]), (what, name, "row", r)                     # row b of a slot mapped elsewhere
        # (1) the appended row sits at [cache_row[b], :, step[b]]
        for b in (live if append else []):
            assert not same(got[row_of(b), :, steps[b]], was[row_of(b), :, steps[b]]), (what, name, "no append", b)
    # (1) live slots against the reference over THEIR cache row
    if live:
        sel = torch.tensor(live, device="cuda")
        check_out(kind, what, out.view(B, H, 64)[sel], ref[sel], model[sel])
    else:
        assert same(out, out0)
