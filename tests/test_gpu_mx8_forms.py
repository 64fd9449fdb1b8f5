"""The MXFP8 dense path (gemm_mx8.hip) in the forms the encoder launches it in, through mt3_op_gemm_mx8 and
mt3_op_mx8_quantize only, against the float64 references, the three operand scripts and the checkers of
tests/mx8_gemm_ref.py (forms, scripts, bounds and their derivation: its docstring; its checkers are themselves tested on
the CPU in tests/test_mx8_gemm_ref.py).  tests/test_gpu_mx8.py keeps the engine-level distances.

Which test launches which instantiation.  launch_mx8 takes NPV 16 with partial sums (a_ss) and K > 512, else NPV 8.

  gemm_mx8_kernel<STORE, 8>    test_rows[enc_qkv], test_norm_ladder[store, K <= 512], test_plain_ladder
  gemm_mx8_kernel<STORE, 16>   test_rows[base_qkv] (npv 12), test_norm_ladder[store, K = 640 (10), 896 (14), 1024 (16)]
  gemm_mx8_kernel<RESID, 8>    test_rows[enc_wo, enc_wo_mlp, base_wo, base_wo_mlp]
  gemm_mx8_kernel<RESID, 16>   unreachable: RESID with a_ss is rejected (test_rejected_calls_leave_the_outputs_alone)
  gemm_mx8_kernel<GEGLU, 8>    test_rows[enc_geglu], test_norm_ladder[geglu, K <= 512]
  gemm_mx8_kernel<GEGLU, 16>   test_rows[base_geglu] (npv 12), test_norm_ladder[geglu, K >= 640]
  gemm_mx8_kernel<HEADS, 8>    test_heads_segments[enc_cross_kv, base_cross_kv], test_heads_normed[heads_normed] (K = 512)
  gemm_mx8_kernel<HEADS, 16>   test_heads_normed[heads_normed_k768]: the ABI reaches it, no engine launches it (the cross
                               K/V projection reads un-normed rows)
  mx8_quantize_kernel<float, true>   test_quantiser_scripts[f32_ss-*], test_quantiser_sizes[f32_ss-*]
  mx8_quantize_kernel<float, false>  test_quantiser_scripts[f32-*], test_quantiser_sizes[f32-*]
  mx8_quantize_kernel<bf16, false>   test_quantiser_scripts[bf16-*], test_quantiser_sizes[bf16-*]
  every instantiation again: test_onehot_every_k (K rows: every k of every K step), test_rolled_rows, test_rolled_w_rows,
  test_rows_against_300

The 3 x 9 tile grid (27 workgroups, 27 % 8 = 3, through xcd_remap) is test_rows[enc_qkv-300-*], rolled in
test_rolled_rows[enc_qkv] and test_rolled_w_rows[enc_qkv].  a_ss with K > 1024 is rejected, so NPV 16 never sees
npv > 16.  The ring has MT3_MX8_NS = 2 stages: K = 128 and 256 are launches that never refill it.

Every case prints its figures (FIG lines): whole-tensor and worst-row rel-L2 against float64, the largest share of the
elementwise bound used, the worst out_ss error, the ties among the stored values, the share of GEGLU block scales that
differ from those of the float64 result.  What the MI355X gave, and what the `exact` script did there: MEASURED below.
"""
import functools
import zlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import mx8_gemm_ref as X  # noqa: E402

VARIANTS = {"f32": (torch.float32, False), "f32_ss": (torch.float32, True), "bf16": (torch.bfloat16, False)}
# MEASURED on MI355X, worst over all cases of a form (row counts, segments, test_onehot_every_k): whole-tensor | worst-row
# rel-L2 against float64, the largest share of the elementwise bound used, the worst out_ss error (bound 1e-6).
#
# The `exact` script at EXACT_LIMIT = 4 (integers -4 .. 4) held BIT FOR BIT in every un-normed STORE / HEADS / RESID case,
# K = 128 .. 2048: the scaled MFMA's alignment of its 128 products and the accumulator loses nothing of sums of up to
# 2^15 units whose products share one unit.  The narrowing to -2 .. 2 was not needed and not made.  `onehot` held bit for
# bit in every case as well.  The first run did show 98 failures, all of the REFERENCE: torch.ldexp on the GPU returns
# 2^-4 (1 - 2^-53) and the like, so x0 + (-x0 (1 - 2^-53)) was 3.6e-15 where the kernel rightly stored 0.0, and ties of the
# bf16 rounding fell the other way; mx8_gemm_ref.pow2 builds the scales from their bits and the accumulators of onehot /
# exact from exact pieces.  The kernel was not changed.  Every rolled-row, rolled-W, M-against-300, guard, rejected-call
# and quantiser comparison (ties, amax positions, range rows with f32 subnormals: the device does not flush them) held bit
# for bit on the first run; sign-of-zero differences between out_q and mx8_ref.quantize: none.
MEASURED = """
  random script                rel-L2 whole | worst row     share of the bound    out_ss
  enc_qkv                      1.66e-3 | 1.80e-3            0.86
  base_qkv                     1.66e-3 | 1.75e-3            0.87
  enc_cross_kv                 1.67e-3 | 1.81e-3            0.87
  base_cross_kv                1.66e-3 | 1.76e-3            0.84
  heads_normed / _k768         1.66e-3 | 1.97e-3  /  1.67e-3 | 1.93e-3     0.84 / 0.82
  enc_wo                       5.04e-5 | 9.78e-5            0.55                  1.4e-7
  enc_wo_mlp                   5.54e-5 | 8.94e-5            0.27                  1.5e-7
  base_wo                      5.52e-5 | 8.28e-5            0.33                  1.8e-7
  base_wo_mlp                  5.24e-5 | 7.98e-5            0.20                  1.5e-7
  enc_geglu                    2.72e-2 | 3.21e-2            0.91    differing block scales 0
  base_geglu                   2.67e-2 | 3.13e-2            0.91    differing block scales 5.2e-5 (cap 0.02)
  ladder_store K 128 .. 1024   1.68e-3 | 2.02e-3            0.89
  ladder_geglu K 128 .. 1024   2.74e-2 | 4.08e-2            0.91    differing block scales 0
  plain_store K 128, 256, 2048 1.68e-3 | 1.91e-3            0.89
  (STORE / HEADS: the rel-L2 is the bf16 rounding of the output, the share is mostly that rounding's |want| / 256;
   RESID: f32 outputs, the share is the MFMA's alignment against MFMA_TOL = 2.5e-4 of sum|a w|: at most 0.55;
   GEGLU: the rel-L2 is the e4m3 rounding of the output.)
  onehot / exact scripts
  un-normed STORE / HEADS / RESID      bit for bit; RESID out_ss <= 2.5e-7; ties of the e4m3 grid among the stored values
                                       of `exact`: 38 .. 57 at M = 1, 1.0e4 .. 1.6e4 at M = 300
  normed STORE / HEADS (|want| / 256)  share 0.994 (enc_qkv, base_qkv), 0.996 (heads_normed), 0.993 (ladder): the bf16
                                       rounding alone reaches 1 - 2^-8, the f32 1 / rms adds 1e-6
  GEGLU (MFMA terms zero)              share 0.941 everywhere (the e4m3 rounding against |want| / 16), differing scales 0
"""


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def case(name, script):
    """operands of a form on the GPU and the float64 reference of all its rows, computed once"""
    return X.build_case(X.FORMS[name], script, zlib.crc32(name.encode()) % 10000 + X.SCRIPTS.index(script), device="cuda")


def launch(c, M, b, seq=None):
    """one launch on the first M rows of the case -> the return code.  A, its scales and a_ss are allocated with
    exactly M rows: nothing behind them"""
    f = c["form"]
    aq, asc = c["aq"][:M].clone(), c["asc"][:M].clone()
    a_ss = None if c["a_ss"] is None else c["a_ss"][:M].clone()
    p = lambda t: None if t is None else t.data_ptr()
    rc = _lib.load().mt3_op_gemm_mx8(aq.data_ptr(), asc.data_ptr(), c["wq"].data_ptr(), c["wsc"].data_ptr(), p(b.get("out")),
                                     M, f.N, f.K, f.epi, (seq or M) if f.epi == X.EPI_HEADS else 0, p(a_ss),
                                     p(b.get("out_q")), p(b.get("out_sc")), p(b.get("out_ss")), stream())
    torch.cuda.synchronize()
    return rc


def outputs(c, M, seq=None):
    """the launch without the value checks (guards only) -> the buffers, HEADS in the logical row layout"""
    b = X.buffers(c, M, seq)
    before = {k: t.clone() for k, t in b.items()}
    _lib.check(launch(c, M, b, seq))
    X.check_guards(c, M, b, before)
    if c["form"].epi == X.EPI_HEADS:
        return {"out": X.from_heads(b["out"], M, c["form"].N, seq or M)}
    return {k: t[:M] for k, t in b.items()}


def run(name, script, M, seq=None):
    """the form on its first M rows with every check of mx8_gemm_ref.check"""
    c = case(name, script)
    assert M <= c["aq"].shape[0]
    b = X.buffers(c, M, seq)
    before = {k: t.clone() for k, t in b.items()}
    _lib.check(launch(c, M, b, seq))
    figs = X.check(c, M, b, before, seq)
    print(f"FIG {name} {script} M {M} seq {seq}: " + " ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}"
                                                               for k, v in figs.items() if v is not None))


def same(a, b, what):
    bad = X.bits(a) != X.bits(b)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, rows {sorted(set(torch.nonzero(bad)[:, 0].tolist()))[:8]}"


# ---------------------------------------------------------------------------------------------------------- the GEMM
@pytest.mark.parametrize("script", X.SCRIPTS)
@pytest.mark.parametrize("M", X.ROW_LIST)
@pytest.mark.parametrize("name", X.ROW_FORMS)
def test_rows(name, M, script):
    """every STORE / RESID / GEGLU launch of the MT3 and the base encoder at every row count around one 128-row tile and
    its two 64-row epilogue passes"""
    run(name, script, M)


@pytest.mark.parametrize("script", X.SCRIPTS)
@pytest.mark.parametrize("seq,B", X.SEGMENTS)
@pytest.mark.parametrize("name", X.HEAD_FORMS)
def test_heads_segments(name, seq, B, script):
    """HEADS with batch seams inside a 64-row pass and inside a 128-row tile, and M = 5, 150, 128, 300, 129, 280"""
    run(name, script, seq * B, seq=seq)


@pytest.mark.parametrize("script", X.SCRIPTS)
@pytest.mark.parametrize("name", ["heads_normed", "heads_normed_k768"])
def test_heads_normed(name, script):
    run(name, script, 150, seq=50)


@pytest.mark.parametrize("script", X.SCRIPTS)
@pytest.mark.parametrize("K", X.LADDER_K)
@pytest.mark.parametrize("kind", ["store", "geglu"])
def test_norm_ladder(kind, K, script):
    """npv = K / 64 = 2 .. 16 partial-sum float4s and the NPV 8 -> 16 switch between K = 512 and 640; 1 .. 8 K steps"""
    assert X.FORMS[f"ladder_{kind}_k{K}"].npv == (8 if K <= 512 else 16)
    run(f"ladder_{kind}_k{K}", script, X.LADDER_M)


@pytest.mark.parametrize("script", X.SCRIPTS)
@pytest.mark.parametrize("K", X.PLAIN_K)
def test_plain_ladder(K, script):
    run(f"plain_store_k{K}", script, X.LADDER_M)


@pytest.mark.parametrize("name", X.ENGINE + ("ladder_store_k128", "ladder_geglu_k640", "heads_normed_k768"))
def test_onehot_every_k(name):
    """K rows of the onehot script: every k of every K step alone in some row, so every k is pinned to its lane, fragment
    half, XOR slot and scale byte"""
    K = X.FORMS[name].K
    assert sorted(X.onehot_k(torch.arange(K), K).tolist()) == list(range(K))
    run(name, "onehot", K)


# ------------------------------------------------------------------------------------------ positions, GPU against GPU
@functools.lru_cache(maxsize=None)
def full(name):
    return outputs(case(name, "random"), X.ROWS)


@pytest.mark.parametrize("name", X.ROW_FORMS)
def test_rolled_rows(name):
    """the A rows (with a_ss, x0) rolled by 75: every output row keeps its bits at its new place"""
    got = outputs(X.rolled_rows(case(name, "random"), X.ROWS), X.ROWS)
    for k, t in full(name).items():
        same(got[k], torch.roll(t, X.A_ROLL, 0), f"{k} of rows rolled by {X.A_ROLL}")


@pytest.mark.parametrize("name", X.ROW_FORMS)
def test_rolled_w_rows(name):
    """the W rows rolled (by 112; GEGLU by 192 = 96 hidden units = three output blocks): every column keeps its bits.
    RESID: x only, the 32-blocks of out_q move with the roll"""
    f = X.FORMS[name]
    shift = X.w_roll(f)
    got = outputs(X.rolled_w(case(name, "random"), shift), X.ROWS)
    base = full(name)
    if f.epi == X.EPI_GEGLU:
        same(got["out_q"], torch.roll(base["out_q"], shift // 2, 1), "out_q")
        same(got["out_sc"], torch.roll(base["out_sc"], shift // 64, 1), "out_sc")
    else:
        same(got["out"], torch.roll(base["out"], shift, 1), "out")


@pytest.mark.parametrize("M", X.ROW_LIST)
@pytest.mark.parametrize("name", X.ENGINE)
def test_rows_against_300(name, M):
    """the first M rows of the M-row launch are those of the 300-row launch, bit for bit (HEADS: one segment of M)"""
    got = outputs(case(name, "random"), M)
    for k, t in full(name).items():
        same(got[k], t[:M], f"{k} at M = {M} against M = 300")


def test_rejected_calls_leave_the_outputs_alone():
    dev, u8 = "cuda", torch.uint8
    M, N, K = 128, 256, 2048                        # every operand is allocated for the largest shape named below
    aq, asc = torch.zeros(M, K, device=dev, dtype=u8), torch.full((M, K // 32), 127, device=dev, dtype=u8)
    wq, wsc = torch.zeros(N, K, device=dev, dtype=u8), torch.full((N, K // 32), 127, device=dev, dtype=u8)
    a_ss = torch.ones(M, K // 16, device=dev)
    b = {"out": X.sentinel((M + X.GUARD, N), torch.float32, dev), "out_q": X.sentinel((M + X.GUARD, N), u8, dev),
         "out_sc": X.sentinel((M + X.GUARD, N // 32), u8, dev), "out_ss": X.sentinel((M + X.GUARD, N // 16), torch.float32, dev)}
    before = {k: t.clone() for k, t in b.items()}
    S, R_, G, H = X.EPI_STORE, X.EPI_RESID, X.EPI_GEGLU, X.EPI_HEADS
    calls = {"K % 128": (S, M, N, 96, 0, False), "N % 128": (S, M, 64, 128, 0, False), "GEGLU with N % 256": (G, M, 128, 128, 0, False),
             "a_ss with K > 1024": (S, M, N, 2048, 0, True), "RESID with a_ss": (R_, M, N, 512, 0, True),
             "HEADS with M % seq": (H, M, N, 512, 50, False)}
    for what, (epi, m, n, k, seq, ss) in calls.items():
        rc = _lib.load().mt3_op_gemm_mx8(aq.data_ptr(), asc.data_ptr(), wq.data_ptr(), wsc.data_ptr(), b["out"].data_ptr(), m, n, k,
                                         epi, seq, a_ss.data_ptr() if ss else None, b["out_q"].data_ptr(), b["out_sc"].data_ptr(),
                                         b["out_ss"].data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc != 0, f"{what} was accepted"
        assert b"gemm_mx8" in _lib.load().mt3_last_error()
        assert X.unchanged(b, before), f"{what}: a rejected call stored something"


# ------------------------------------------------------------------------------------------------------ the quantiser
def dev_quantize(x, with_ss):
    """x [M][K] on the CPU -> (q, sc, ss) of mt3_op_mx8_quantize on the CPU; the input has exactly M rows, every output
    a tail of sentinel bytes that must come back unchanged"""
    M, K = x.shape
    xd = x.cuda().contiguous()
    n = M * K
    q, sc = X.sentinel((n + 4096,), torch.uint8, "cuda"), X.sentinel((n // 32 + 512,), torch.uint8, "cuda")
    ss = X.sentinel((n // 16 + 512,), torch.float32, "cuda")
    _lib.check(_lib.load().mt3_op_mx8_quantize(xd.data_ptr(), 1 if x.dtype == torch.float32 else 0, M, K, q.data_ptr(),
                                               sc.data_ptr(), ss.data_ptr() if with_ss else None, stream()))
    torch.cuda.synchronize()
    for t, own, what in ((q, n, "q"), (sc, n // 32, "sc"), (ss, n // 16 if with_ss else 0, "ss")):
        assert bool((X.bits(t[own:]) == X.bits(X.sentinel((1,), t.dtype, "cuda"))).all()), f"{what}: a store behind the last row"
    return q[:n].view(M, K).cpu(), sc[:n // 32].view(M, K // 32).cpu(), ss[:n // 16].view(M, K // 16).cpu()


@pytest.mark.parametrize("script", list(X.QUANT_SCRIPTS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_quantiser_scripts(variant, script):
    """ties of the e4m3 grid (normal and subnormal results) with their one-ulp neighbours under sixteen amax anchors; the
    amax at every position of both blocks of a row; 448 2^k, huge, tiny, sub-2^-120 and f32-subnormal blocks, -0.0"""
    dtype, with_ss = VARIANTS[variant]
    x = X.QUANT_SCRIPTS[script](dtype)
    q, sc, ss = dev_quantize(x, with_ss)
    X.check_quantiser(x, q, sc, ss if with_ss else None)


@pytest.mark.parametrize("M,K", X.QUANT_SIZES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_quantiser_sizes(variant, M, K):
    """one partial 256-lane block (16, 48, 480 lanes) and 225 whole ones; the partial sums of squares with them"""
    dtype, with_ss = VARIANTS[variant]
    x = X.quant_random_rows(M, K, dtype, 7)
    x[M // 2, 32:64] = 0
    q, sc, ss = dev_quantize(x, with_ss)
    X.check_quantiser(x, q, sc, ss if with_ss else None)
