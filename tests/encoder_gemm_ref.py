"""Float64 reference, input scripts and checkers for one encoder-sized GEMM launch (gemm.hip: gemm_glds_kernel and the
128 x 128 gemm_kernel tile, through mt3_op_gemm_ex / mt3_op_gemm with small = 0), in torch on whatever device the operands
live on.  The launch arithmetic is decode_gemm_ref.evaluate's (STORE, F32, RESID, GEGLU, the three norms); added here:

  POS     out[r] = A[r] . Wt^T + table[r % seq_len]                                    (f32)
  HEADS   column kv * H * 64 + h * 64 + d of row b * T + t  ->  [kv][b][h][t][d]      (compute type), to_heads / from_heads

TWO INPUT SCRIPTS per form (build_case):

  exact    A integers in [-8, 8], W multiples of 0.5 in [-1, 1], RESID rows and the POS table multiples of 0.5 with
           |x| <= 1024: all exact in bf16 and f32, and every partial sum of a dot product is an integer number of units
           of 0.5 below 2^24 (exact_units: 16 K + 2048 <= 34816 at K = 2048), so the accumulator does not depend on the
           summation order: the unscaled outputs are fixed to the bit.  The norm-2 partial sums are SCRIPTED and
           independent of A (the kernel never relates the two; decode_attention_ref.scripted_partial_sums): one dominant
           16-column group per row at index (5 row) % (K / 16) -- 5 is coprime to every K / 16 in use, so over K / 16 <= 64
           consecutive rows the dominant group sits in every float4 of the row -- the others log-uniform over four decades.
           A dropped float4 shrinks the sum 16-fold in some row of every tile, a duplicated one grows it 1.9-fold.
  random   the operands of tests/test_gpu_kernels.py: unit normals, weights over sqrt(K), residual rows with a per-row
           scale (0.25 .. 4.25), their bf16 copy and partial sums from `split` (the GPU tests pass mt3_op_residual_split).

BOUNDS.  exact script, unscaled (norm 0): f32 outputs equal the float64 value, bf16 outputs its round-to-nearest-even,
bit for bit.  Scaled (norm 1 / 2): the accumulator is exact, so got must lie in [f(acc rs64 (1 - E)), f(acc rs64 (1 + E))]
with both ends rounded to the output type; E = rs_error(K, norm) bounds the f32 error of the kernel's
rs = rsqrtf(t / K + 1e-6) and of its product with the accumulator:
    norm 2   t is the sequential f32 sum of n = K / 16 positive terms: n - 1 additions, each within 2^-24 of the running
             sum <= t, halved by the square root: (n - 1) 2^-25; plus one ulp (2^-23) each for the division, the + 1e-6,
             rsqrtf and the product:  E = (K / 16 - 1) 2^-25 + 2^-21
             K   64: 5.66e-7   128: 6.85e-7   192: 8.05e-7   256: 9.24e-7   384: 1.16e-6   512: 1.40e-6   576: 1.52e-6
             K  768: 1.88e-6  1024: 2.35e-6
    norm 1   the kernel sums the squares of the integer row itself, exactly: E = 2^-21 = 4.77e-7
GEGLU: f(g, l) = gelu_tanh(g) l with both arguments scaled; the interval is the hull of f at the factors 1 - E, 1, 1 + E
(gelu_tanh is not monotone; between the three the variation is second order in E), widened by 2 G |g| |l|: the kernel's
gelu_tanh_fast is x / (1 + exp2(-1.4427 * 2u)) in f32 with two 1-ulp hardware approximations (v_exp_f32, v_rcp_f32), and
G = gelu_fast_error(args) is the worst |fast32(x) - gelu_tanh64(x)| / |x| of an f32 torch evaluation of the same formula
on the CPU over the arguments the case produces (relative to |x|, not to the value: in the negative tail the value decays
like exp(-|arg|) while the f32 rounding of the exponent grows with |arg|, so only the product sigmoid * x is well
conditioned); the factor 2 stands for the two approximations and also covers the rounding of the final product.
G = 1.09e-7 (enc_geglu), 1.17e-7 (base_geglu), 1.38e-7 / 1.44e-7 (the norm-1 forms, bf16 / f32), 1.15e-7 (f32 with
partial sums): about one f32 ulp (tests/test_encoder_gemm_ref.py prints them).
random script: the project's whole-tensor rel-L2 bound of the epilogue (BOUND: tests/test_gpu_kernels.py), and the worst
single row against the same number; tests/test_encoder_gemm_ref.py checks that the float64 result rounded to the output
type (model_worst_row) stays below half of it in its worst row for every form.  RESID by-products under both scripts:
out_ct bit-equal to the bf16 rounding of the f32 rows the launch wrote, out_ss within 1e-5 relative.

GUARDS (buffers / check_guards): every output has two rows more than the launch (HEADS: a tail of two rows behind
[2][B][H][T][64]), filled like the rest with values no result equals; everything outside rows [0, M) must come back bit
for bit.
"""
import dataclasses

import torch

from tests import decode_gemm_ref as D
from tests.decode_attention_ref import dominant_index, scripted_partial_sums  # noqa: F401  (dominant_index: the tests)

EPI_STORE, EPI_RESID, EPI_GEGLU, EPI_POS, EPI_F32, EPI_HEADS = range(6)          # MT3_EPI_* (include/mt3_hip.h)
BOUND = {(EPI_STORE, False): 6e-3, (EPI_STORE, True): 2e-5, (EPI_HEADS, False): 6e-3, (EPI_HEADS, True): 2e-5,
         (EPI_GEGLU, False): 8e-3, (EPI_GEGLU, True): 3e-5}                       # (epilogue, f32 compute type)
F32_BOUND = 2e-5                                                                  # RESID, POS, F32: f32 outputs
SS_BOUND = 1e-5
GUARD = 2                                                                         # guard rows behind every output
ROLL = 176                    # a multiple of 16 (a row keeps its MFMA lane), not of 64 (it changes fragment, wave, pass, tile)


@dataclasses.dataclass(frozen=True)
class Form:
    epi: int
    K: int
    N: int                   # weight rows (GEGLU: gate + linear)
    norm: int = 0
    f32: bool = False        # the compute type: f32 operands (else bf16)
    a_f32: bool = False      # the A operand arrives as f32 rows and is rounded to the compute type while it is staged
    by: bool = False         # RESID by-products: out_ss, and with bf16 out_ct
    seq: int = 0             # POS: rows of the table; HEADS: the segment length (0: one segment of M rows)
    rows: int = 300          # rows of operands and reference (cases use the first M)

    @property
    def ct(self):
        return torch.float32 if self.f32 else torch.bfloat16

    @property
    def out_t(self):
        return self.ct if self.epi in (EPI_STORE, EPI_GEGLU, EPI_HEADS) else torch.float32

    @property
    def width(self):
        return self.N // 2 if self.epi == EPI_GEGLU else self.N

    @property
    def bound(self):
        return BOUND.get((self.epi, self.f32), F32_BOUND)


def _forms():
    S, R_, G, P, F, H = EPI_STORE, EPI_RESID, EPI_GEGLU, EPI_POS, EPI_F32, EPI_HEADS
    f = {
        # ---- bf16, the LDS-DMA tile (launch_glds), named after the launch of encode_impl / the scoring pass
        "enc_qkv": Form(S, 512, 1152, norm=2, rows=379),           # normed_gemm(L.wqkv), 3 x 9 tiles at M = 379
        "enc_wo": Form(R_, 384, 512, by=True),                     # resid_gemm(L.wo)
        "enc_geglu": Form(G, 512, 2048, norm=2),                   # normed_gemm(L.wi)
        "enc_wo_mlp": Form(R_, 1024, 512, by=True),                # resid_gemm(L.wo_mlp)
        "enc_cross_kv": Form(H, 512, 768, rows=768),               # dense_gemm(wkv_x, MT3_EPI_HEADS)
        "score_logits": Form(F, 512, 1536, norm=2),                # normed_gemm(e->logits_w, MT3_EPI_F32), scoring pass
        "base_qkv": Form(S, 768, 2304, norm=2),                    # ismir2022/base.gin: 48 partial sums, NPV 16
        "base_geglu": Form(G, 768, 4096, norm=2),
        "base_wo_mlp": Form(R_, 2048, 768),
        "wide_qkv": Form(S, 1024, 256, norm=2),                    # all 16 partial-sum registers live
        "k576": Form(F, 576, 128, norm=2),                         # 9 of 16
        "base_logits": Form(F, 768, 1536, norm=2),                 # the scoring pass's logits at the base.gin shape
        # ---- the 128 x 128 gemm_kernel tile (launch_tile with small = 0)
        "enc_in": Form(P, 512, 512, a_f32=True, seq=100),          # dense_gemm(e->enc_in, MT3_EPI_POS)
        "enc_in_f32": Form(P, 512, 512, a_f32=True, seq=100, f32=True),
        "single_qkv": Form(S, 512, 1152, norm=1, a_f32=True),      # MT3_OPT_ENCODER_SINGLE_RESIDUAL_STREAM
        "single_geglu": Form(G, 512, 2048, norm=1, a_f32=True),
        "single_logits": Form(F, 512, 128, norm=1, a_f32=True),
        "mfma_qkv": Form(S, 512, 1152, norm=1, a_f32=True, f32=True),      # MT3_OPT_ENCODER_F32_MFMA
        "mfma_geglu": Form(G, 512, 2048, norm=1, a_f32=True, f32=True),
        "mfma_logits": Form(F, 512, 128, norm=1, a_f32=True, f32=True),
        "mfma_wo": Form(R_, 384, 512, f32=True),
        "mfma_wo_ss": Form(R_, 384, 128, f32=True, by=True),
        "mfma_cross_kv": Form(H, 512, 768, f32=True, rows=768),
        "store_k96": Form(S, 96, 128),                             # K % 64 != 0: off the LDS-DMA tile
        "resid_k96": Form(R_, 96, 128, by=True),
        "heads_k96": Form(H, 96, 128),
        "f32out_k96": Form(F, 96, 128),
        "plain_store_f32": Form(S, 384, 128, f32=True),
        "plain_f32out_f32": Form(F, 512, 128, f32=True),           # the weight folds of mt3_engine_finalize
        "af32_store": Form(S, 128, 128, a_f32=True),
        "af32_f32out": Form(F, 128, 128, a_f32=True),
        "af32_store_f32": Form(S, 128, 128, a_f32=True, f32=True),
        "af32_f32out_f32": Form(F, 128, 128, a_f32=True, f32=True),
        # f32 operands with partial sums: reachable through mt3_op_gemm_ex, launched by no engine (an f32 engine keeps
        # the single f32 stream)
        "split_store_f32": Form(S, 512, 128, norm=2, f32=True),
        "split_geglu_f32": Form(G, 512, 128, norm=2, f32=True),
        "split_f32out_f32": Form(F, 512, 128, norm=2, f32=True),
        "split_store_f32_k768": Form(S, 768, 128, norm=2, f32=True),
        "split_geglu_f32_k768": Form(G, 768, 128, norm=2, f32=True),
        "split_f32out_f32_k768": Form(F, 768, 128, norm=2, f32=True),
    }
    for K in RING_K:       # the K ladder of the ring; 128 n - 5 rows for n = 1 .. 9 workgroups
        f[f"ring_store_k{K}"] = Form(S, K, 128, rows=1147)
        f[f"ring_f32out_k{K}"] = Form(F, K, 128, norm=2, rows=1147)
    # the 256-row tile: the smallest M with ceil(M / 256) * N / 128 >= 1024 and a ragged last tile
    f["enc_qkv_tall"] = dataclasses.replace(f["enc_qkv"], rows=113 * 256 + 37)
    f["enc_geglu_tall"] = dataclasses.replace(f["enc_geglu"], rows=63 * 256 + 37)
    f["enc_cross_kv_tall"] = dataclasses.replace(f["enc_cross_kv"], seq=100, rows=43800)
    f["base_qkv_tall"] = dataclasses.replace(f["base_qkv"], rows=56 * 256 + 37)
    f["base_geglu_tall"] = dataclasses.replace(f["base_geglu"], rows=31 * 256 + 37)
    f["score_logits_tall"] = dataclasses.replace(f["score_logits"], rows=85 * 256 + 37)
    f["base_logits_tall"] = dataclasses.replace(f["base_logits"], rows=85 * 256 + 37)
    return f


# MT3_GLDS_NS = 3 ring stages (two K slices in flight), MT3_GLDS_BK = 32: these K are 2, 4, 6, 8 and 12 slices -- fewer
# slices than the ring has stages (K = 64), and both live branches of the wait ladder in every launch (`ahead == 1` up
# to the last slice but one, the vmcnt(0) tail; with three stages the `ahead >= 2` branch is compiled out)
RING_K = (64, 128, 192, 256, 384)
FORMS = _forms()
TALL = tuple(n for n in FORMS if n.endswith("_tall"))


def rs_error(K, norm):
    """E of the module docstring: the relative f32 error of the kernel's 1/rms times accumulator"""
    if norm == 0:
        return 0.0
    return (K // 16 - 1) * 2.0 ** -25 + 2.0 ** -21 if norm == 2 else 2.0 ** -21


def exact_units(K):
    """the largest |partial sum| of the exact script, in units of 0.5: K products of at most 8 * 1, plus a residual /
    table element of at most 1024"""
    return 16 * K + 2048


def gelu_fast32(x):
    """gelu_tanh_fast (device.h) evaluated by torch in f32"""
    x = x.float()
    u2 = 1.5957691216057308 * (x + 0.044715 * x * x * x)
    return x * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * u2)))


def gelu_fast_error(args):
    """G of the module docstring over the arguments `args` (any shape), evaluated on the CPU"""
    x = args.detach().reshape(-1).cpu().float()
    x = x[x != 0]
    if x.numel() == 0:
        return 0.0
    return float(((gelu_fast32(x).double() - D.gelu_tanh(x.double())).abs() / x.double().abs()).max())


def to_heads(x, seq):
    """logical [M][2 H 64] -> [2][B][H][T][64]"""
    M, N = x.shape
    return x.view(M // seq, seq, 2, N // 128, 64).permute(2, 0, 3, 1, 4).contiguous()


def from_heads(flat, M, N, seq):
    """the first M * N elements of a HEADS buffer -> logical [M][N]"""
    return flat[:M * N].view(2, M // seq, N // 128, seq, 64).permute(1, 3, 0, 2, 4).reshape(M, N)


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ---------------------------------------------------------------------------------------------------- the two scripts
def _halves(shape, limit, g):
    """multiples of 0.5 in [-limit, limit]"""
    return torch.randint(-2 * limit, 2 * limit + 1, shape, generator=g).float() * 0.5


def _cpu_split(x):
    return x.to(torch.bfloat16), (x.double() ** 2).view(x.shape[0], x.shape[1] // 16, 16).sum(-1).float()


def build_case(form, script, seed, device="cpu", split=None):
    """operands of `form` under `script` ('exact' / 'random') for form.rows rows on `device`, the float64 accumulator
    `acc` [rows][N] (unscaled A . Wt^T), the float64 row scales `rs` [rows][1] and the float64 result `ref`
    [rows][width] in the logical row layout.  split: f32 rows on `device` -> (bf16 copy, partial sums)."""
    f, g = form, torch.Generator().manual_seed(seed)
    R_, K, ct = f.rows, f.K, f.ct
    c = dict(form=f, script=script, a_ss=None, out0=None, pos=None, G=0.0)
    if script == "exact":
        assert exact_units(K) < 2 ** 24
        A = torch.randint(-8, 9, (R_, K), generator=g).float()
        c["A"] = A if f.a_f32 else A.to(ct)
        if f.norm == 2:
            c["a_ss"] = scripted_partial_sums(R_, K // 16, seed)
        w = _halves((f.N, K), 1, g).to(ct)
        c["Wt"] = D.interleave16(w[:f.N // 2], w[f.N // 2:]) if f.epi == EPI_GEGLU else w
        if f.epi == EPI_RESID:
            c["out0"] = _halves((R_, f.N), 1024, g)
        if f.epi == EPI_POS:
            c["pos"] = _halves((f.seq, f.N), 1024, g)
    else:
        x = torch.randn(R_, K, generator=g)
        if f.norm:
            x = x * (0.25 + 4 * torch.rand(R_, 1, generator=g))
        if f.norm == 2 and f.f32:                               # f32 rows are their own compute-type copy
            c["A"], c["a_ss"] = x, _cpu_split(x)[1]
        elif f.norm == 2:
            c["A"], c["a_ss"] = (split or _cpu_split)(x.to(device))
        else:
            c["A"] = x if f.a_f32 else x.to(ct)
        c["Wt"] = D.geglu_weight(f.N // 2, K, seed + 1, ct)[0] if f.epi == EPI_GEGLU else D.weight(f.N, K, seed + 1, ct)
        if f.epi == EPI_RESID:
            c["out0"] = torch.randn(R_, f.N, generator=g) * (0.25 + 4 * torch.rand(R_, 1, generator=g))
        if f.epi == EPI_POS:
            c["pos"] = torch.randn(f.seq, f.N, generator=g)
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            c[k] = v.to(device)
    a = (c["A"].to(ct) if f.a_f32 else c["A"]).double()
    c["acc"] = a @ c["Wt"].double().T
    c["rs"] = D.row_scales(f.norm, c["A"], c["a_ss"], K)
    if script == "exact":
        top = float(c["acc"].abs().max()) + (1024 if f.epi in (EPI_RESID, EPI_POS) else 0)
        assert 2 * top <= exact_units(K) < 2 ** 24, "the exact script left its magnitude bound"
    # the float64 result: decode_gemm_ref.evaluate for the arithmetic it knows; POS and HEADS are an unscaled product
    # with a table row added / stored elsewhere
    epi = {EPI_POS: EPI_F32, EPI_HEADS: EPI_STORE}.get(f.epi, f.epi)
    c["ref"] = D.evaluate(A=c["A"], Wt=c["Wt"], M=R_, N=f.N, K=K, epilogue=epi, ct=ct, norm=f.norm, a_is_f32=f.a_f32,
                          a_ss=c["a_ss"], out=c["out0"])[0]
    if f.epi == EPI_POS:
        c["ref"] = c["ref"] + c["pos"].double()[torch.arange(R_, device=device) % f.seq]
    if f.epi == EPI_GEGLU and script == "exact":
        gate = (c["acc"] * c["rs"]).view(R_, f.N // 32, 2, 16)[:min(R_, 300), :, 0]
        c["G"] = gelu_fast_error(gate)
    return c


def rolled(c, M, shift=ROLL):
    """the case with its first M rows rolled by `shift`: row r of every per-row operand and of the reference moves to
    row (r + shift) % M"""
    out = dict(c)
    for k in ("A", "a_ss", "out0", "acc", "rs", "ref"):
        if c[k] is not None:
            out[k] = torch.roll(c[k][:M], shift, 0)
    if c["form"].epi == EPI_POS:                                  # the table row belongs to the position, not to the row
        dev = c["ref"].device
        r = torch.arange(M, device=dev)
        out["ref"] = out["ref"] - c["pos"].double()[torch.roll(r, shift) % c["form"].seq] + c["pos"].double()[r % c["form"].seq]
    return out


# ------------------------------------------------------------------------------------------------------------ buffers
def garbage(shape, dt, seed, device):
    """values no result equals (and no two alike enough for a misplaced store to go unnoticed)"""
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(*shape, device=device, generator=g) * 300 + 7777).to(dt)


def buffers(c, M):
    """the output buffers of a launch on the first M rows, each with GUARD rows more: `out` ([M + 2][width]; HEADS: flat
    [(M + 2) N]; RESID: rows [0, M) hold the residual rows), and for the RESID by-products `out_ss` / `out_ct`"""
    f, dev = c["form"], c["Wt"].device
    if f.epi == EPI_HEADS:
        b = {"out": garbage(((M + GUARD) * f.N,), f.out_t, 1, dev)}
    else:
        b = {"out": garbage((M + GUARD, f.width), f.out_t, 1, dev)}
    if f.epi == EPI_RESID:
        b["out"][:M] = c["out0"][:M]
        if f.by:
            b["out_ss"] = garbage((M + GUARD, f.N // 16), torch.float32, 2, dev)
            if not f.f32:
                b["out_ct"] = garbage((M + GUARD, f.N), torch.bfloat16, 3, dev)
    return b


def primary(c, M, b, seq=None):
    """what the launch wrote, in the logical row layout [M][width]"""
    f = c["form"]
    if f.epi == EPI_HEADS:
        return from_heads(b["out"], M, f.N, seq or f.seq or M)
    return b["out"][:M]


def check_guards(c, M, b, before):
    """everything outside what the launch owns came back bit for bit"""
    f = c["form"]
    for k, t in b.items():
        if f.epi == EPI_HEADS:
            assert torch.equal(bits(t[M * f.N:]), bits(before[k][M * f.N:])), "HEADS wrote behind [2][B][H][T][64]"
        else:
            assert D.untouched(t, before[k], M, 0, t.shape[1]), f"{k}: a store outside rows [0, {M})"


# ----------------------------------------------------------------------------------------------------------- checkers
def where(bad):
    r, col = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
    return f"{int(bad.sum())} elements differ, rows {sorted(set(torch.nonzero(bad)[:, 0].tolist()))[:8]}, first at ({r}, {col})"


def check_by_products(c, M, b, figs):
    f = c["form"]
    if not f.by:
        return
    rows = b["out"][:M]
    ct_ref, ss_ref = D.by_products(rows, torch.bfloat16)
    figs["ss"] = float(((b["out_ss"][:M].double() - ss_ref).abs() / ss_ref.clamp_min(1e-30)).max())
    assert figs["ss"] < SS_BOUND, f"out_ss worst relative error {figs['ss']:.3e}"
    if "out_ct" in b:
        bad = bits(b["out_ct"][:M]) != bits(ct_ref)
        assert not bool(bad.any()), "out_ct is not the rounding of the f32 rows: " + where(bad)


def check_exact(c, M, b, seq=None):
    """the exact script: bit equality of the unscaled outputs, the E interval of the scaled ones -> figures"""
    f = c["form"]
    got = primary(c, M, b, seq)
    ref = c["ref"][:M]
    figs = dict(rel=D.rel(got, ref), row=D.worst_row(got, ref), share=None, ss=None)
    if f.norm == 0:
        want = (ref + 0.0).to(f.out_t)
        bad = bits(got.contiguous()) != bits(want)
        assert not bool(bad.any()), "the unscaled exact result is fixed to the bit: " + where(bad)
    else:
        E = rs_error(f.K, f.norm)
        v = c["acc"][:M] * c["rs"][:M]
        if f.epi == EPI_GEGLU:
            p = v.view(M, f.N // 32, 2, 16)
            g, l = p[:, :, 0].reshape(M, -1), p[:, :, 1].reshape(M, -1)
            cand = torch.stack([D.gelu_tanh(g * s) * (l * s) for s in (1 - E, 1.0, 1 + E)])
            widen = 2 * c["G"] * g.abs() * l.abs()
            lo, hi = cand.amin(0) - widen, cand.amax(0) + widen
        else:
            lo, hi = torch.minimum(v * (1 - E), v * (1 + E)), torch.maximum(v * (1 - E), v * (1 + E))
            if f.out_t == torch.float32:
                nz = v != 0
                figs["share"] = float(((got.double() - v)[nz].abs() / (E * v[nz].abs())).max()) if bool(nz.any()) else 0.0
        lo, hi = lo.float().to(f.out_t).double(), hi.float().to(f.out_t).double()
        bad = (got.double() < lo) | (got.double() > hi) | ~torch.isfinite(got.double())
        assert not bool(bad.any()), f"outside the interval of E = {E:.3e}: " + where(bad)
    check_by_products(c, M, b, figs)
    return figs


def check_random(c, M, b, seq=None):
    """the random script: whole tensor and worst single row against the project's bound of the epilogue -> figures"""
    f = c["form"]
    got, ref = primary(c, M, b, seq), c["ref"][:M]
    figs = dict(rel=D.rel(got, ref), row=D.worst_row(got, ref), share=None, ss=None)
    assert figs["rel"] < f.bound, f"whole-tensor rel-L2 {figs['rel']:.3e} (bound {f.bound:.0e})"
    assert figs["row"] < f.bound, f"worst row rel-L2 {figs['row']:.3e} (bound {f.bound:.0e})"
    check_by_products(c, M, b, figs)
    return figs


def check(c, M, b, before, seq=None):
    check_guards(c, M, b, before)
    return (check_exact if c["script"] == "exact" else check_random)(c, M, b, seq)


def model_worst_row(c, M):
    """worst-row rel-L2 of the error model: the float64 result rounded to the output type"""
    ref = c["ref"][:M]
    return D.worst_row(ref.float().to(c["form"].out_t), ref)


# ------------------------------------------------------------------ a correct launch in plain f32 torch (the CPU tests)
def model_launch(c, M, b, acc=None, a_ss=None, out0=None, seq=None):
    """What a correct kernel leaves in the buffers `b`, computed with plain torch in f32 from the exact accumulator.
    The overrides are how tests/test_encoder_gemm_ref.py builds WRONG launches: another accumulator [M][N], other
    partial sums [M][K / 16], other residual rows [M][N]."""
    f = c["form"]
    acc = (c["acc"][:M] if acc is None else acc).float()
    if f.norm == 2:
        t = (c["a_ss"][:M] if a_ss is None else a_ss).float().sum(-1, keepdim=True)
    elif f.norm == 1:
        t = (c["A"][:M].float() ** 2).sum(-1, keepdim=True)
    rs = torch.rsqrt(t / float(f.K) + 1e-6) if f.norm else torch.ones(M, 1)
    v = acc * rs.to(acc.device)
    if f.epi == EPI_GEGLU:
        p = v.view(M, f.N // 32, 2, 16)
        v = (gelu_fast32(p[:, :, 0]) * p[:, :, 1]).reshape(M, f.N // 2)
    elif f.epi == EPI_RESID:
        v = (c["out0"][:M] if out0 is None else out0) + v
    elif f.epi == EPI_POS:
        v = v + c["pos"][torch.arange(M) % f.seq]
    if f.epi == EPI_HEADS:
        b["out"][:M * f.N] = to_heads(v.to(f.out_t), seq or f.seq or M).reshape(-1)
    else:
        b["out"][:M] = v.to(f.out_t)
    if f.by:
        ct, ss = D.by_products(b["out"][:M], torch.bfloat16)
        b["out_ss"][:M] = ss.float()
        if "out_ct" in b:
            b["out_ct"][:M] = ct
    return b
