"""Forms, operand scripts, float64 references and checkers for one launch of the MXFP8 dense path (gemm_mx8.hip:
gemm_mx8_kernel through mt3_op_gemm_mx8, mx8_quantize_kernel through mt3_op_mx8_quantize), in torch on whatever device
the operands live on.  The format is tests/mx8_ref.py's: e4m3fn bytes `q`, one E8M0 byte `sc` per 32 consecutive k.

THREE OPERAND SCRIPTS (build_case).  The operands are built as bytes: the GEMM is tested apart from the quantisers.

  onehot   row m of A holds the single e4m3 value 1.0 at k_m = (37 m + 11) % K (onehot_k) and zeros elsewhere, under the
           scale bytes 120 + (3 m + 5 b) % 13 of its blocks b; W[n][k] is the finite e4m3 code number (5 k + 3 n) % 254
           (all 254 of them: subnormals, +-448, +0, -0) under the scale bytes 121 + (n + 3 b) % 11.  Every output is ONE
           product, at least 2^-9 2^-7 2^-6 and at most 448 2^5 2^4: a normal f32 that is exact in bf16 too, so the output
           is fixed to the bit whatever the MFMA does when it aligns its 128 products.  Neighbouring blocks of a row never
           share a scale byte (5 and 3 are no multiples of 13 and 11), and the codes at k and k +- 16, k +- 64 differ in
           value (80 and 66 are neither 0 nor 127 modulo 254).  37 is coprime to every K in use, so rows 0 .. K - 1 hit
           every k of every 128-step exactly once; the case has max(300, K) rows and test_onehot_every_k launches K of them.
           The row-count cases use the first M <= 300 rows: the k they hit are onehot_k(arange(M), K).
  exact    elements are integers in -EXACT_LIMIT .. EXACT_LIMIT; A's scale byte is 127 + r[m] + d[b], W's 127 + c[n] - d[b]
           with r, c in -3 .. 3 and d[b] = (step + 2 g) % 9 - 4 for block g of K step `step` (exact_offsets: distinct
           over the four blocks of a step, different in neighbouring steps).  The offsets cancel in every product, which
           is an integer of magnitude <= 16 in units of 2^(r + c); every partial sum stays below 16 K <= 2^15 units, so the
           f32 sum is exact in any order.  A kernel that pairs block g's elements with block g''s scale is off by
           2^(d[g'] - d[g]) in that block's share.  RESID adds integer rows |x0| <= 64: at most (16 K + 64) 64 < 2^24
           units of min(1, 2^(r + c)) (exact_units).
  random   tests/test_gpu_mx8.py's rows (unit normals, a log-normal factor per row, outlier columns x 30) and weights
           (normals x 0.05), quantised by mx8_ref.quantize; the fused norm's partial sums are those of the rows.

With the fused norm the partial sums of onehot / exact are SCRIPTED and independent of A (the kernel never relates the
two): decode_attention_ref.scripted_partial_sums, one dominant 16-column group per row at (5 row) % (K / 16), so a dropped
float4 of partial sums shrinks the sum 16-fold in some row of any 64 consecutive ones.

BOUNDS (check).  None is looser than tests/test_gpu_mx8.py's for the same quantity.
  onehot / exact, no norm   STORE / HEADS: the bf16 rounding of the float64 value, bit for bit; RESID: the f32 rounding of
                            x0 + value, bit for bit, out_q / out_sc equal to mx8_ref.quantize of those rows (e4m3 zeros
                            compared as values, as everywhere in this project), out_ss within 1e-6 relative; on `exact`
                            the ties of the e4m3 grid among the stored values are counted and some must occur
  onehot / exact, norm      |got - value rs| <= |value rs| / 256 with rs from float64: no MFMA slack
  random                    STORE / HEADS: |value rs| / 256 + MFMA_TOL sum|a w| rs;  RESID: 2e-7 |want| + MFMA_TOL sum|a w|
                            + 1e-7, by-products against the rows the kernel itself stored
  GEGLU                     test_gemm_mx8_every_epilogue's first-order propagation through gelu(g) l plus one e4m3
                            rounding; on onehot / exact with the MFMA terms set to zero; the share of block scales that
                            differ from those of the float64 result stays below 0.02
GUARDS (buffers / check_guards): every output carries 130 rows (HEADS: at least one batch entry per plane) of the byte
0xA5 behind row M; every byte outside what the launch owns must come back unchanged.

THE QUANTISER SCRIPTS (tie_rows, position_rows, range_rows; check_quantiser): bit equality with mx8_ref.quantize.
"""
import dataclasses

import torch

from tests import mx8_ref
from tests.decode_attention_ref import scripted_partial_sums
from tests.decode_gemm_ref import gelu_tanh, rel, worst_row
from tests.encoder_gemm_ref import from_heads, gelu_fast32, to_heads, where

EPI_STORE, EPI_RESID, EPI_GEGLU, EPI_HEADS = 0, 1, 2, 5                          # MT3_EPI_* (include/mt3_hip.h)
MFMA_TOL = 2.5e-4             # tests/test_gpu_mx8.py: |error| <= MFMA_TOL * sum_k |a_k w_k|
SS_BOUND = 1e-6
SCALE_SHARE = 0.02
GUARD = 130                   # guard rows behind every output: more than one 128-row tile
SENTINEL = 0xA5
ROWS = 300
ROW_LIST = (1, 63, 64, 65, 127, 128, 129, 300)
SEGMENTS = ((1, 5), (50, 3), (64, 2), (100, 3), (129, 1), (140, 2))             # HEADS: (seq, B)
A_ROLL = 75
EXACT_LIMIT = 4               # |element| of the exact script
SCRIPTS = ("onehot", "exact", "random")
CODES = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)     # every finite e4m3fn code
ONE = 0x38                    # e4m3fn 1.0


@dataclasses.dataclass(frozen=True)
class Form:
    epi: int
    N: int                    # weight rows (GEGLU: gate + linear, interleaved in 16s)
    K: int
    norm: bool = False        # the fused RMSNorm: a_ss

    @property
    def npv(self):            # the instantiation launch_mx8 selects
        return 16 if self.norm and self.K > 512 else 8


def _forms():
    S, R_, G, H = EPI_STORE, EPI_RESID, EPI_GEGLU, EPI_HEADS
    f = {
        "enc_qkv": Form(S, 1152, 512, True), "enc_wo": Form(R_, 512, 384), "enc_geglu": Form(G, 2048, 512, True),
        "enc_wo_mlp": Form(R_, 512, 1024), "enc_cross_kv": Form(H, 768, 512),
        "base_qkv": Form(S, 2304, 768, True), "base_wo": Form(R_, 768, 768), "base_geglu": Form(G, 4096, 768, True),
        "base_wo_mlp": Form(R_, 768, 2048), "base_cross_kv": Form(H, 1536, 768),
        # the ABI reaches these, the engine does not (its cross K/V projection reads un-normed rows)
        "heads_normed": Form(H, 256, 512, True), "heads_normed_k768": Form(H, 256, 768, True),
    }
    for K in LADDER_K:        # npv = K / 64 = 2 .. 16 of the NPV registers, the clamp u < npv ? u : npv - 1
        f[f"ladder_store_k{K}"] = Form(S, 256, K, True)
        f[f"ladder_geglu_k{K}"] = Form(G, 256, K, True)
    for K in PLAIN_K:         # one and two K steps (the ring is never refilled) and sixteen, without the norm
        f[f"plain_store_k{K}"] = Form(S, 256, K)
    return f


LADDER_K = (128, 256, 384, 512, 640, 896, 1024)
PLAIN_K = (128, 256, 2048)
LADDER_M = 65
FORMS = _forms()
ENGINE = ("enc_qkv", "enc_wo", "enc_geglu", "enc_wo_mlp", "enc_cross_kv", "base_qkv", "base_wo", "base_geglu",
          "base_wo_mlp", "base_cross_kv")
ROW_FORMS = tuple(n for n in ENGINE if FORMS[n].epi != EPI_HEADS)
HEAD_FORMS = tuple(n for n in ENGINE if FORMS[n].epi == EPI_HEADS)


def onehot_k(m, K):
    return (37 * m + 11) % K


def exact_offsets(K):
    """d [K / 32]: block g of K step `step` -> (step + 2 g) % 9 - 4"""
    b = torch.arange(K // 32)
    return (b // 4 + 2 * (b % 4)) % 9 - 4


def exact_units(K):
    """the largest |x0 + partial sum| of the exact script in units of min(1, 2^(r + c)) (module docstring)"""
    return (16 * K + 64) * 64


def e4m3(x):
    return x.float().to(torch.float8_e4m3fn).view(torch.uint8)


def pow2(e):
    """2^e in float64 from its bits (integer tensor, -1022 <= e <= 1023): torch.ldexp on a GPU goes through a power
    function and returns 2^-4 (1 - 2^-53) and the like, which turns exact sums into near misses of a rounding tie"""
    return ((e.long() + 1023) << 52).view(torch.float64)


def dequantize(q, sc):
    """mx8_ref.dequantize with exact scales on every device -> float64 [rows, K]"""
    rows, K = q.shape
    v = q.view(torch.float8_e4m3fn).double().view(rows, K // 32, 32)
    return (v * pow2(sc.int() - 127)[..., None]).reshape(rows, K)


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def w_roll(form):
    """W rows to roll by: 16 * 7 (a row keeps its MFMA lane, changes fragment and tile); GEGLU 64 * 3, which keeps the
    gate / linear pairs of 16 together AND the 32-blocks of the MXFP8 output (64 W rows each)"""
    return 192 if form.epi == EPI_GEGLU else 112


# -------------------------------------------------------------------------------------------------------- the scripts
def build_case(form, script, seed, rows=None, limit=EXACT_LIMIT, device="cpu"):
    """operands of `form` under `script` for `rows` rows on `device` (aq, asc, wq, wsc, a_ss, x0), the float64
    accumulator `acc` [rows][N] of the dequantised operands, `mag` = sum_k |a w| (random only) and the float64 row
    scales `rs` [rows][1].  `limit`: |element| of the exact script; 4 held bit for bit on the MI355X (MEASURED in
    tests/test_gpu_mx8_forms.py), the parameter stays for the one-time narrowing to 2 should another part need it."""
    f, g = form, torch.Generator().manual_seed(seed)
    K, N = f.K, f.N
    R_ = rows or (max(ROWS, K) if script == "onehot" else ROWS)
    m, n, kb = torch.arange(R_), torch.arange(N), torch.arange(K // 32)
    c = dict(form=f, script=script, a_ss=None, x0=None, mag=None)
    if script == "onehot":
        aq = torch.zeros(R_, K, dtype=torch.uint8)
        aq[m, onehot_k(m, K)] = ONE
        asc = 120 + (3 * m[:, None] + 5 * kb[None]) % 13
        wq = CODES[(5 * torch.arange(K)[None] + 3 * n[:, None]) % 254]
        wsc = 121 + (n[:, None] + 3 * kb[None]) % 11
    elif script == "exact":
        aq = e4m3(torch.randint(-limit, limit + 1, (R_, K), generator=g))
        wq = e4m3(torch.randint(-limit, limit + 1, (N, K), generator=g))
        c["r"], c["c"] = torch.randint(-3, 4, (R_,), generator=g), torch.randint(-3, 4, (N,), generator=g)
        d = exact_offsets(K)
        asc, wsc = 127 + c["r"][:, None] + d[None], 127 + c["c"][:, None] - d[None]
    else:
        x = torch.randn(R_, K, generator=g)
        x *= torch.exp(torch.randn(R_, 1, generator=g))
        x[:, 3::97] *= 30.0
        (aq, asc), (wq, wsc) = mx8_ref.quantize(x), mx8_ref.quantize(torch.randn(N, K, generator=g) * 0.05)
        if f.norm:
            c["a_ss"] = (x.double() ** 2).view(R_, K // 16, 16).sum(-1).float()
    if f.norm and script != "random":
        c["a_ss"] = scripted_partial_sums(R_, K // 16, seed)
    if f.epi == EPI_RESID:
        c["x0"] = torch.randn(R_, N, generator=g) if script == "random" else torch.randint(-64, 65, (R_, N), generator=g).float()
    c.update(aq=aq, asc=asc.to(torch.uint8), wq=wq, wsc=wsc.to(torch.uint8))
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            c[k] = v.to(device)
    ad, wd = dequantize(c["aq"], c["asc"]), dequantize(c["wq"], c["wsc"])
    # the accumulator of the two bit-exact scripts is built from exact pieces alone (one product; integers rounded to
    # integers, times an exact power of two): an error of 1e-16 is enough to break a tie of the output's rounding
    if script == "onehot":
        km = onehot_k(torch.arange(R_, device=device), K)
        c["acc"] = ad[torch.arange(R_, device=device), km][:, None] * wd[:, km].T + 0.0    # the one product, exact (+ the zeros)
    elif script == "exact":
        ints = lambda q: q.view(torch.float8_e4m3fn).double()
        units = (ints(c["aq"]) @ ints(c["wq"]).T).round()                                   # integers below 2^15
        c["acc"] = units * pow2(c["r"][:, None] + c["c"][None])
    else:
        c["acc"] = ad @ wd.T
    if script == "random":
        c["mag"] = ad.abs() @ wd.abs().T
    if f.norm:
        c["rs"] = torch.rsqrt(c["a_ss"].double().sum(-1, keepdim=True) / K + 1e-6)
    else:
        c["rs"] = torch.ones(R_, 1, dtype=torch.float64, device=device)
    return c


def rolled_rows(c, M, shift=A_ROLL):
    """the case with its first M rows rolled: row r of every per-row operand and reference moves to (r + shift) % M"""
    out = dict(c)
    for k in ("aq", "asc", "a_ss", "x0", "acc", "mag", "rs", "r"):
        if c.get(k) is not None:
            out[k] = torch.roll(c[k][:M], shift, 0)
    return out


def rolled_w(c, shift):
    """the case with its W rows (= output columns; the residual's columns with them) rolled by `shift`"""
    out = dict(c)
    for k in ("wq", "wsc", "c"):
        if c.get(k) is not None:
            out[k] = torch.roll(c[k], shift, 0)
    for k in ("x0", "acc", "mag"):
        if c.get(k) is not None:
            out[k] = torch.roll(c[k], shift, 1)
    return out


# ------------------------------------------------------------------------------------------------------------ buffers
def sentinel(shape, dt, device):
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty(0, dtype=dt).element_size(),), SENTINEL, dtype=torch.uint8, device=device).view(dt).view(*shape)


def buffers(c, M, seq=None):
    """the outputs of a launch on the first M rows, filled with the sentinel byte and GUARD rows longer; RESID's `out`
    holds the residual rows in [0, M).  HEADS: flat, with max(GUARD, seq) rows -- at least the two batch entries of one
    per plane -- in ONE tail behind [2][B][H][seq][64].  A guard entry behind each plane cannot be laid out: the kernel
    derives B from M / seq and packs the planes, so the K plane's entry B IS the V plane's entry 0; a store there is
    caught by the value check of that entry (every element of both planes is compared), not by the guard."""
    f, dev = c["form"], c["wq"].device
    R_ = M + GUARD
    if f.epi == EPI_HEADS:
        return {"out": sentinel(((M + max(GUARD, seq or M)) * f.N,), torch.bfloat16, dev)}
    if f.epi == EPI_STORE:
        return {"out": sentinel((R_, f.N), torch.bfloat16, dev)}
    if f.epi == EPI_GEGLU:
        return {"out_q": sentinel((R_, f.N // 2), torch.uint8, dev), "out_sc": sentinel((R_, f.N // 64), torch.uint8, dev)}
    b = {"out": sentinel((R_, f.N), torch.float32, dev), "out_q": sentinel((R_, f.N), torch.uint8, dev),
         "out_sc": sentinel((R_, f.N // 32), torch.uint8, dev), "out_ss": sentinel((R_, f.N // 16), torch.float32, dev)}
    b["out"][:M] = c["x0"][:M]
    return b


def check_guards(c, M, b, before):
    """every byte outside what the launch owns came back unchanged"""
    f = c["form"]
    for k, t in b.items():
        own = M * f.N if f.epi == EPI_HEADS else M
        bad = bits(t[own:]) != bits(before[k][own:])
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} elements stored behind row {M}"


def unchanged(b, before):
    return all(torch.equal(bits(t), bits(before[k])) for k, t in b.items())


# ----------------------------------------------------------------------------------------------------------- checkers
def count_ties(rows, sc):
    """how many elements of the f32 rows sit exactly half way between two e4m3 values once divided by their block scale"""
    return int(tie_mask(scaled(rows, sc)).sum())


def scaled(rows, sc):
    """rows / block scale in float64 (the reciprocal clamps at 2^127 as the rule's does)"""
    M, W = rows.shape
    inv = pow2((127 - sc.int()).clamp(max=127))
    return (rows.double().view(M, W // 32, 32) * inv[..., None]).reshape(M, W)


def tie_mask(y):
    """y float64, already divided by the block scale (|y| < 256)"""
    q = y.float().to(torch.float8_e4m3fn).double()
    other = q + 2 * (y - q)                   # q mirrored at y: an e4m3 value exactly when y is a midpoint
    return (y != q) & (other.float().to(torch.float8_e4m3fn).double() == other)


def _within(got, want, bound, what):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{what}: " + where(bad)
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def _same_bits(got, want, what):
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"{what}: " + where(bad)


def check_mx8_copy(rows, q, sc, ss, figs):
    """out_q / out_sc / out_ss against the f32 rows [M][N] they were made from"""
    M, N = rows.shape
    rq, rsc = mx8_ref.quantize(rows)
    assert torch.equal(sc, rsc), "out_sc: " + where(sc != rsc)
    bad = q.view(torch.float8_e4m3fn).float() != rq.view(torch.float8_e4m3fn).float()
    assert not bool(bad.any()), "out_q: " + where(bad)
    figs["zero_signs"] = int((q != rq).sum())
    ref = (rows.double() ** 2).view(M, N // 16, 16).sum(-1)
    figs["ss"] = float(((ss.double() - ref).abs() / ref.clamp_min(1e-30)).max())
    assert figs["ss"] < SS_BOUND, f"out_ss worst relative error {figs['ss']:.3e}"


def check(c, M, b, before, seq=None):
    """guards, then the bounds of the module docstring -> figures (rel, row: rel-L2 against float64; share: the largest
    share of an elementwise bound used; ss, ties)"""
    check_guards(c, M, b, before)
    f, script = c["form"], c["script"]
    acc, rs = c["acc"][:M], c["rs"][:M]
    mag = c["mag"][:M] if script == "random" else None
    figs = dict(rel=None, row=None, share=None, ss=None, ties=None)
    if f.epi in (EPI_STORE, EPI_HEADS):
        got = from_heads(b["out"], M, f.N, seq or M) if f.epi == EPI_HEADS else b["out"][:M]
        want = acc * rs
        if script == "random":
            figs["share"] = _within(got, want, want.abs() / 256 + MFMA_TOL * mag * rs, "outside the MFMA bound")
        elif f.norm:
            figs["share"] = _within(got, want, want.abs() / 256, "outside |want| / 256 (no MFMA slack)")
        else:
            _same_bits(got, (want + 0.0).float().to(torch.bfloat16), f"the {script} result is fixed to the bit")
    elif f.epi == EPI_RESID:
        got, want = b["out"][:M], c["x0"][:M].double() + acc
        if script == "random":
            figs["share"] = _within(got, want, want.abs() * 2e-7 + MFMA_TOL * mag + 1e-7, "outside the MFMA bound")
        else:
            _same_bits(got, (want + 0.0).float(), f"the {script} result is fixed to the bit")
        check_mx8_copy(got, b["out_q"][:M], b["out_sc"][:M], b["out_ss"][:M], figs)
        if script == "exact":
            figs["ties"] = count_ties(got, b["out_sc"][:M])
            assert figs["ties"] > 0, "no stored value is a tie of the e4m3 grid: the script lost its point"
    else:
        hq, hsc = b["out_q"][:M], b["out_sc"][:M]
        p4 = (acc * rs).view(M, f.N // 32, 2, 16)
        gate, lin = p4[:, :, 0], p4[:, :, 1]
        want = (gelu_tanh(gate) * lin).reshape(M, f.N // 2)
        slack = torch.zeros_like(want)
        if script == "random":      # first-order propagation of the MFMA bound through gelu(g) * l (|gelu'| <= 1.13)
            m4 = (mag * rs).view(M, f.N // 32, 2, 16)
            eg, el = MFMA_TOL * m4[:, :, 0], MFMA_TOL * m4[:, :, 1]
            slack = (1.13 * eg * lin.abs() + (gelu_tanh(gate).abs() + 1.13 * eg) * el).reshape(M, f.N // 2)
        got = dequantize(hq, hsc)
        step = pow2(hsc.int() - 127).repeat_interleave(32, 1) / 512
        figs["share"] = _within(got, want, (want.abs() + slack) / 16 + slack + step + 1e-6 * want.abs(), "GEGLU bound")
        figs["scales"] = float((hsc != mx8_ref.quantize(want.float())[1]).float().mean())
        assert figs["scales"] < SCALE_SHARE, f"share of differing GEGLU block scales {figs['scales']:.4f}"
    figs["rel"], figs["row"] = rel(got, want), worst_row(got, want)
    return figs


def check_quantiser(x, q, sc, ss=None):
    """the device rule is mx8_ref's, bit for bit (e4m3 zeros as values); ss: the sums of squares of the 16-column groups
    within SS_BOUND of float64 wherever that sum is below 1e38 (a group whose squares overflow f32 has no value to meet)"""
    rq, rsc = mx8_ref.quantize(x)
    assert torch.equal(sc, rsc), "scale bytes: " + where(sc != rsc)
    bad = q.view(torch.float8_e4m3fn).float() != rq.view(torch.float8_e4m3fn).float()
    assert not bool(bad.any()), "elements: " + where(bad)
    if ss is not None:
        ref = (x.double() ** 2).view(x.shape[0], x.shape[1] // 16, 16).sum(-1)
        bad = ~((ss.double() - ref).abs() <= SS_BOUND * ref.clamp_min(1e-30)) & (ref < 1e38)
        assert not bool(bad.any()), "sums of squares: " + where(bad)


# ---------------------------------------------------------------- a correct launch in plain torch (the CPU tests)
def model_launch(c, M, b, seq=None, aq=None, asc=None, a_ss=None, heads_stride64=False):
    """What a kernel that keeps its contract leaves in `b`: float64 products of the dequantised operands, rounded where
    the kernel rounds.  The overrides are how tests/test_mx8_gemm_ref.py builds WRONG launches: other operand bytes /
    scale bytes [M][..], other partial sums, the HEADS batch index taken once per 64-row pass."""
    f = c["form"]
    if aq is None and asc is None:
        acc = c["acc"][:M]
    else:
        acc = dequantize(c["aq"][:M] if aq is None else aq, c["asc"][:M] if asc is None else asc) @ \
            dequantize(c["wq"], c["wsc"]).T
    v = acc.float()
    if f.norm:
        t = (c["a_ss"][:M] if a_ss is None else a_ss).float().sum(-1, keepdim=True)
        v = v * torch.rsqrt(t / float(f.K) + 1e-6)
    if f.epi == EPI_STORE:
        b["out"][:M] = v.to(torch.bfloat16)
    elif f.epi == EPI_HEADS:
        seq = seq or M
        if not heads_stride64:
            b["out"][:M * f.N] = to_heads(v.to(torch.bfloat16), seq).reshape(-1)
        else:
            row, col = torch.arange(M)[:, None], torch.arange(f.N)[None]
            hd, H, B = f.N // 2, f.N // 128, M // seq
            bb, tt = (row // 64 * 64) // seq, row % seq
            dst = ((((col // hd) * B + bb) * H + (col % hd) // 64) * seq + tt) * 64 + col % 64
            b["out"][dst.reshape(-1)] = v.to(torch.bfloat16).reshape(-1)
    elif f.epi == EPI_RESID:
        x = c["x0"][:M] + v
        b["out"][:M] = x
        b["out_q"][:M], b["out_sc"][:M] = mx8_ref.quantize(x)
        b["out_ss"][:M] = (x.double() ** 2).view(M, f.N // 16, 16).sum(-1).float()
    else:
        p = v.view(M, f.N // 32, 2, 16)
        b["out_q"][:M], b["out_sc"][:M] = mx8_ref.quantize((gelu_fast32(p[:, :, 0]) * p[:, :, 1]).reshape(M, f.N // 2))
    return b


# ------------------------------------------------------------------------------------------- the quantiser's scripts
ANCHORS = tuple((mant, e) for e in (-100, -30, -7, 0, 1, 7, 30, 100) for mant in (1.0, 1.875))


def midpoints():
    """the 112 midpoints of the non-negative e4m3 grid below 128: eight between subnormal results (the last one between
    7 2^-9 and the smallest normal), and (8 + j + 0.5) / 8 2^p for p = -6 .. 6.  At most 5 significant bits: exact in bf16"""
    sub = [(j + 0.5) * 2.0 ** -9 for j in range(8)]
    return torch.tensor(sub + [(8 + j + 0.5) / 8 * 2.0 ** p for p in range(-6, 7) for j in range(8)], dtype=torch.float64)


def _neighbour(x, dtype, step):
    """the positive values x (exact in dtype) moved by `step` ulps of dtype, as f32"""
    if dtype == torch.bfloat16:
        return (x.to(dtype).view(torch.int16) + step).view(dtype).float()
    return (x.float().view(torch.int32) + step).view(torch.float32)


def tie_rows(dtype):
    """[len(ANCHORS)][384] in `dtype`: per anchor amax = mant 2^e twelve blocks, each the amax and 31 values from the list
    (midpoint, one ulp of dtype below, one above) of every midpoint times the block scale 2^(e - 7), signs alternating"""
    rows = []
    for mant, e in ANCHORS:
        mid = (midpoints() * 2.0 ** (e - 7)).float()
        vals = torch.stack([mid, _neighbour(mid, dtype, -1), _neighbour(mid, dtype, 1)], 1).reshape(-1)        # 336
        vals = vals * torch.tensor([1.0, -1.0]).repeat(168)
        vals = torch.cat([vals, vals])[:12 * 31].view(12, 31)
        amax = torch.full((12, 1), mant * 2.0 ** e) * torch.tensor([1.0, -1.0]).repeat(6)[:, None]
        rows.append(torch.cat([amax, vals], 1).reshape(-1))
    return torch.stack(rows).to(dtype)


def position_rows(dtype):
    """[128][64]: the amax (+-3072) at each of the 32 positions of the first, then of the second block of a 64-element
    row; the blocks' other elements live in the binades of 2^-3 and 2^5, so the row's two scale bytes always differ"""
    i = torch.arange(32)
    sign = torch.tensor([1.0, -1.0]).repeat(16)
    base = torch.cat([(1 + (i % 7) / 8) * 2.0 ** -3 * sign, (1 + (i % 5) / 8) * 2.0 ** 5 * -sign])
    x = base.repeat(128, 1)
    r = torch.arange(128)
    x[r, (r // 64) * 32 + r % 32] = torch.where((r // 32) % 2 == 0, 3072.0, -3072.0)
    return x.to(dtype)


def range_rows(dtype):
    """[6][64]: 448 2^k on top of a ramp for k = 0, 20, -20; blocks of ~1e30 and ~1e-30; amax in [2^-121, 2^-120) (the
    scale byte clamps at 0) and exactly 2^-120; f32 subnormals; zeros with -0.0 among them; the largest finite bf16"""
    g = torch.Generator().manual_seed(5)
    ramp = torch.cat([torch.tensor([448.0]), torch.linspace(0.0, 447.9, 31)])
    i = torch.arange(32, dtype=torch.float32)
    tiny = (1 + i / 64) * 2.0 ** -121
    edge = torch.cat([torch.tensor([2.0 ** -120]), tiny[1:] / 4])
    sub = (i + 1) * 1000 * 2.0 ** -149
    zero = torch.zeros(32)
    zero[1::3] = -0.0
    top = torch.cat([torch.tensor([-3.3895313892515355e38]), torch.randn(31, generator=g) * 1e37])
    return torch.stack([torch.cat([ramp, ramp * 2.0 ** 20]), torch.cat([ramp * 2.0 ** -20, torch.randn(32, generator=g) * 1e30]),
                        torch.cat([torch.randn(32, generator=g) * 1e-30, tiny]), torch.cat([edge, sub]),
                        torch.cat([zero, -sub]), torch.cat([top, zero])]).to(dtype)


QUANT_SCRIPTS = {"ties": tie_rows, "position": position_rows, "range": range_rows}
QUANT_SIZES = ((1, 64), (3, 64), (5, 384), (300, 768))


def quant_random_rows(M, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    x[:, 3::97] *= 30.0
    return x.to(dtype)
