"""The encoder-sized GEMM tiles (gemm.hip: gemm_glds_kernel with its 128- and 256-row tiles, and the 128 x 128 gemm_kernel
tile) in the forms encode_impl, normed_gemm and resid_gemm (engine.hip) launch them in, through mt3_op_gemm_ex /
mt3_op_gemm with small = 0, against the float64 reference, the two input scripts and the checkers of
tests/encoder_gemm_ref.py (forms, scripts, bounds and their derivation: its docstring; its checkers are themselves tested
on the CPU in tests/test_encoder_gemm_ref.py).

Which test launches which instantiation launch_gemm can select with small = 0.  NPV 16 is taken with partial sums and
K > 512, BM 256 when ceil(M / 256) * N / 128 >= 1024 (never for RESID).

  gemm_glds_kernel<STORE, 8>        test_glds_rows[enc_qkv], test_ring[store-*] (norm 0), test_three_by_nine_tiles
  gemm_glds_kernel<STORE, 16>       test_glds_rows[base_qkv, wide_qkv]
  gemm_glds_kernel<STORE, 8, 256>   test_tall_tile[enc_qkv_tall]
  gemm_glds_kernel<STORE, 16, 256>  test_tall_tile[base_qkv_tall]
  gemm_glds_kernel<RESID, 8>        test_glds_rows[enc_wo, enc_wo_mlp, base_wo_mlp] (RESID carries no partial sums: never 16)
  gemm_glds_kernel<GEGLU, 8>        test_glds_rows[enc_geglu]
  gemm_glds_kernel<GEGLU, 16>       test_glds_rows[base_geglu]
  gemm_glds_kernel<GEGLU, 8, 256>   test_tall_tile[enc_geglu_tall]
  gemm_glds_kernel<GEGLU, 16, 256>  test_tall_tile[base_geglu_tall]
  gemm_glds_kernel<HEADS, 8>        test_glds_rows[enc_cross_kv], test_cross_kv_segments
  gemm_glds_kernel<HEADS, 8, 256>   test_tall_tile[enc_cross_kv_tall]
  gemm_glds_kernel<HEADS, 16[, 256]> unreachable: HEADS launches carry no partial sums
  gemm_glds_kernel<F32, 8>          test_glds_rows[score_logits], test_ring[f32out-*] (norm 2)
  gemm_glds_kernel<F32, 16>         test_glds_rows[k576, base_logits]
  gemm_glds_kernel<F32, 8, 256>     test_tall_tile[score_logits_tall]
  gemm_glds_kernel<F32, 16, 256>    test_tall_tile[base_logits_tall]
  gemm_kernel<bf16, 128, 128, 32, 2, 2, A_F32, NORM, EPI, NPV> (bf16 launches that are not LDS-DMA eligible):
    <true, false, POS>              test_big_tile_rows[enc_in]
    <true, true, STORE | GEGLU>     test_big_tile_rows[single_qkv, single_geglu]  (MT3_OPT_ENCODER_SINGLE_RESIDUAL_STREAM)
    <true, true, F32>               test_other_big_tile_instantiations[single_logits]
    <true, false, STORE | F32>      test_other_big_tile_instantiations[af32_store, af32_f32out]
    <false, false, STORE>           test_big_tile_rows[store_k96]  (K % 64 != 0)
    <false, false, RESID | HEADS | F32>  test_other_big_tile_instantiations[resid_k96, heads_k96, f32out_k96]
    norm 2 (a_ss; NPV 8 and 16)     unreachable: every bf16 norm-2 shape launch_typed accepts is LDS-DMA eligible
  gemm_kernel<float, 128, 128, 16, 2, 2, A_F32, NORM, EPI, NPV> (MT3_OPT_ENCODER_F32_MFMA):
    <true, false, POS>              test_big_tile_rows[enc_in_f32]
    <true, true, STORE | GEGLU>     test_big_tile_rows[mfma_qkv, mfma_geglu]
    <true, true, F32>               test_other_big_tile_instantiations[mfma_logits]
    <false, false, RESID | HEADS>   test_big_tile_rows[mfma_wo, mfma_cross_kv]; with out_ss: [mfma_wo_ss]
    <false, false, STORE | F32>     test_other_big_tile_instantiations[plain_store_f32, plain_f32out_f32]
    <true, false, STORE | F32>      test_other_big_tile_instantiations[af32_store_f32, af32_f32out_f32]
    norm 2 <.., STORE | GEGLU | F32, 8 | 16>  test_other_big_tile_instantiations[split_*_f32, split_*_f32_k768]; no engine
                                    launches them (an f32 engine keeps the single f32 stream), the ABI reaches them

The ring: MT3_GLDS_NS = 3 stages and MT3_GLDS_BK = 32 in this build (the issue that asked for these tests assumed 4):
K = 64 .. 384 is 2 .. 12 slices -- fewer slices than stages at K = 64, and both live branches of the wait ladder
(`ahead == 1`, the vmcnt(0) tail) at every K; the `ahead >= 2` branch does not exist with three stages.  PPW = 4 waits
run in every 128-row launch, PPW = 6 in the tall ones.

Every case prints its figures: whole-tensor and worst-row rel-L2 against float64, the share of the E interval used (f32
outputs of the exact script), the worst out_ss error.  Rolled rows (test_rolled_rows): the same rows rolled by 176 must
give every row the same bits at its new position.  MEASURED on MI355X, worst over all cases: see MEASURED below.
"""
import functools
import zlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import encoder_gemm_ref as E  # noqa: E402

BF16, F32 = _lib.MT3_BF16, _lib.MT3_F32
ROWS = [1, 63, 64, 65, 127, 128, 129, 300]          # one 128-row tile and its two 64-row passes from both sides; three tiles
GLDS = ["enc_qkv", "enc_wo", "enc_geglu", "enc_wo_mlp", "enc_cross_kv", "score_logits", "base_qkv", "base_geglu",
        "base_wo_mlp", "wide_qkv", "k576", "base_logits"]
BIG = ["enc_in", "enc_in_f32", "single_qkv", "single_geglu", "mfma_qkv", "mfma_geglu", "mfma_wo", "mfma_cross_kv",
       "store_k96"]
OTHER = ["single_logits", "mfma_logits", "mfma_wo_ss", "resid_k96", "heads_k96", "f32out_k96", "plain_store_f32",
         "plain_f32out_f32", "af32_store", "af32_f32out", "af32_store_f32", "af32_f32out_f32", "split_store_f32",
         "split_geglu_f32", "split_f32out_f32", "split_store_f32_k768", "split_geglu_f32_k768", "split_f32out_f32_k768"]
SCRIPTS = ["exact", "random"]
# MEASURED on MI355X, worst over all cases of a form (tall cases included): whole-tensor | worst-row rel-L2 against float64
# on the random script (bound), share of the E interval used on the exact script (f32 outputs), worst out_ss error.
# Every bit comparison of this file held on the first run: the unscaled exact outputs of every form, out_ct, the tall
# against the 128-row tile, the rolled rows of every STORE / F32 / RESID / HEADS form on both kernels, and every guard.
MEASURED = """
  enc_qkv 1.69e-3 | 1.83e-3 (6e-3)      base_qkv 1.66e-3 | 1.78e-3 (6e-3)     wide_qkv 1.67e-3 | 1.99e-3 (6e-3)
  enc_geglu 1.75e-3 | 2.32e-3 (8e-3)    base_geglu 1.70e-3 | 2.02e-3 (8e-3)   enc_cross_kv 1.74e-3 | 1.88e-3 (6e-3)
  enc_wo 4.8e-8 | 1.2e-7 (2e-5), out_ss 1.5e-7      enc_wo_mlp 7.4e-8 | 1.9e-7 (2e-5), out_ss 1.6e-7 (bound 1e-5)
  base_wo_mlp 2.5e-7 | 2.9e-7 (2e-5)    score_logits 1.7e-7 | 2.4e-7 (2e-5), E share 0.25     k576 1.6e-7 | 2.4e-7, 0.15
  base_logits 1.8e-7 | 3.2e-7 (2e-5), E share 0.19
  ring_store_k64 .. k384 1.68e-3 | 2.16e-3 (6e-3)   ring_f32out_k64 .. k384 1.2e-7 | 2.1e-7 (2e-5), E share 0.30 .. 0.21
  enc_in 1.0e-7 | 1.1e-7, f32 2.9e-7 | 3.3e-7 (2e-5)          single_qkv 1.67e-3 | 1.80e-3 (6e-3)
  single_geglu 1.90e-3 | 1.99e-3 (8e-3)                       single_logits 1.4e-7 | 2.0e-7 (2e-5), E share 0.25
  mfma_qkv 4.1e-7 | 4.7e-7 (2e-5), E share 0.27               mfma_geglu 6.3e-7 | 8.5e-7 (3e-5)
  mfma_wo 1.6e-7 | 3.6e-7 (2e-5), out_ss 1.3e-7               mfma_cross_kv 4.2e-7 | 4.6e-7 (2e-5)
  store_k96 / heads_k96 / af32_store 1.70e-3 | 2.05e-3 (6e-3); resid_k96 / f32out_k96 / af32_f32out below 1e-7 (2e-5)
  f32 operands, the other instantiations: at most 5.0e-7 | 6.6e-7 (2e-5), GEGLU 7.5e-7 | 1.3e-6 (3e-5), E share <= 0.25
"""


def stream():
    return torch.cuda.current_stream().cuda_stream


def split(x):
    """f32 rows -> (bf16 copy, per-16-column sums of squares) through mt3_op_residual_split"""
    M, K = x.shape
    ct = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
    ss = torch.empty(M, K // 16, device="cuda")
    _lib.check(_lib.load().mt3_op_residual_split(BF16, x.data_ptr(), ct.data_ptr(), ss.data_ptr(), M, K, stream()))
    torch.cuda.synchronize()
    return ct, ss


@functools.lru_cache(maxsize=None)
def case(name, script):
    """operands of a form on the GPU and the float64 reference of all its rows, computed once"""
    f = E.FORMS[name]
    seed = zlib.crc32(name.replace("_tall", "").encode()) % 10000 + (1 if script == "random" else 0)
    return E.build_case(f, script, seed, device="cuda", split=split if not f.f32 else None)


def launch(c, M, out, seq=None, r0=0, out_ct=None, out_ss=None):
    """one launch on rows [r0, r0 + M) of the case.  A and a_ss are allocated with exactly M rows: nothing behind them"""
    f = c["form"]
    A = c["A"][r0:r0 + M].clone()
    a_ss = None if c["a_ss"] is None else c["a_ss"][r0:r0 + M].clone()
    p = lambda t: None if t is None else t.data_ptr()
    seq_len = f.seq if f.epi == E.EPI_POS else (seq or f.seq or M) if f.epi == E.EPI_HEADS else 0
    dt = F32 if f.f32 else BF16
    if f.norm == 2 or out_ss is not None:
        rc = _lib.load().mt3_op_gemm_ex(dt, A.data_ptr(), int(f.a_f32), f.norm, c["Wt"].data_ptr(), out.data_ptr(), M, f.N,
                                        f.K, f.epi, p(c["pos"]), seq_len, 0, p(a_ss), p(out_ct), p(out_ss), stream())
    else:
        rc = _lib.load().mt3_op_gemm(dt, A.data_ptr(), int(f.a_f32), f.norm, c["Wt"].data_ptr(), out.data_ptr(), M, f.N,
                                     f.K, f.epi, p(c["pos"]), seq_len, 0, stream())
    torch.cuda.synchronize()
    _lib.check(rc)


def run(name, script, M, seq=None, roll=False):
    """The form on its first M rows with every check of encoder_gemm_ref.check -> the buffers the launch left"""
    c = case(name, script)
    assert M <= c["form"].rows
    if roll:
        c = E.rolled(c, M)
    b = E.buffers(c, M)
    before = {k: t.clone() for k, t in b.items()}
    launch(c, M, b["out"], seq, out_ct=b.get("out_ct"), out_ss=b.get("out_ss"))
    figs = E.check(c, M, b, before, seq=seq)
    fmt = lambda v: "-" if v is None else f"{v:.3e}"
    print(f"FIG {name} {script} M {M} seq {seq} roll {int(roll)}: rel {fmt(figs['rel'])} row {fmt(figs['row'])} "
          f"bound {c['form'].bound:.0e} share {fmt(figs['share'])} ss {fmt(figs['ss'])}")
    b["out"] = E.primary(c, M, b, seq)
    return b


def tall_tiles(M, N):
    """what launch_glds counts: 256-row tiles of the launch; the tall tile is taken from 1024"""
    return (M + 255) // 256 * (N // 128)


def tile_is_tall(name, M):
    f = E.FORMS[name]
    return not f.f32 and not f.a_f32 and f.norm != 1 and f.K % 64 == 0 and f.epi != E.EPI_RESID and tall_tiles(M, f.N) >= 1024


# ------------------------------------------------------------------------------------------------- the LDS-DMA tile
@pytest.mark.parametrize("script", SCRIPTS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("name", GLDS)
def test_glds_rows(name, M, script):
    """every form of the bf16 encoder and of the scoring pass's logits on the 128 x 128 LDS-DMA tile, at every row count
    around one tile and its 64-row passes (enc_cross_kv: one segment of M positions)"""
    assert not tile_is_tall(name, M)
    run(name, script, M)


@pytest.mark.parametrize("script", SCRIPTS)
@pytest.mark.parametrize("seq,B", [(256, 3), (100, 3), (100, 5)])
def test_cross_kv_segments(seq, B, script):
    """HEADS with tiles that straddle segment boundaries: seq_len 100 puts a boundary inside every tile"""
    run("enc_cross_kv", script, seq * B, seq=seq)


@pytest.mark.parametrize("script", SCRIPTS)
@pytest.mark.parametrize("n", range(1, 10))
@pytest.mark.parametrize("K", E.RING_K)
@pytest.mark.parametrize("kind", ["store", "f32out"])
def test_ring(kind, K, n, script):
    """The K ladder of the ring (2, 4, 6, 8, 12 slices: encoder_gemm_ref.RING_K) at N = 128, STORE with norm 0 and F32 with
    norm 2, on grids of n = 1 .. 9 workgroups (xcd_remap with fewer than 8, exactly 8, and 8 + 1), last tile 5 rows short"""
    run(f"ring_{kind}_k{K}", script, 128 * n - 5)


@pytest.mark.parametrize("script", SCRIPTS)
def test_three_by_nine_tiles(script):
    """27 workgroups (27 % 8 = 3) on a grid with both dimensions above one"""
    assert (379 + 127) // 128 == 3 and E.FORMS["enc_qkv"].N // 128 == 9
    run("enc_qkv", script, 379)


@pytest.mark.parametrize("script", SCRIPTS)
@pytest.mark.parametrize("name,piece", [("enc_qkv_tall", 113 * 128), ("enc_geglu_tall", 63 * 128), ("base_qkv_tall", 56 * 128),
                                        ("base_geglu_tall", 31 * 128), ("score_logits_tall", 85 * 128),
                                        ("base_logits_tall", 85 * 128),
                                        ("enc_cross_kv_tall", 100 * 128)])
def test_tall_tile(name, piece, script):
    """The 256 x 128 tile at the smallest M that takes it (>= 1024 tall tiles; enc_cross_kv: 438 segments of 100), the
    last tile ragged (37 rows; 24 for enc_cross_kv, where the last tile and most tile seams fall inside a segment), against
    float64 -- and bit for bit against the same rows launched in slices that stay on the 128-row tile"""
    f = E.FORMS[name]
    M = f.rows
    assert tall_tiles(M, f.N) >= 1024 and M % 256 in (37, 24)
    assert name == "enc_cross_kv_tall" or tall_tiles(M - 256, f.N) < 1024
    assert tall_tiles(piece, f.N) < 1024 and tall_tiles(M - piece, f.N) < 1024 and piece % (f.seq or 1) == 0
    tall = run(name, script, M, seq=f.seq or None)["out"]
    c = case(name, script)
    parts = []
    for r0 in range(0, M, piece):
        m = min(piece, M - r0)
        out = E.garbage(((m + E.GUARD) * f.N,) if f.epi == E.EPI_HEADS else (m + E.GUARD, f.width), f.out_t, 5, "cuda")
        launch(c, m, out, f.seq or None, r0=r0)
        parts.append(E.from_heads(out, m, f.N, f.seq) if f.epi == E.EPI_HEADS else out[:m])
    bad = E.bits(torch.cat(parts).contiguous()) != E.bits(tall.contiguous())
    assert not bool(bad.any()), "the 256-row and the 128-row tile must produce identical outputs: " + E.where(bad)


# ------------------------------------------------------------------------------------- the 128 x 128 gemm_kernel tile
@pytest.mark.parametrize("script", SCRIPTS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("name", BIG)
def test_big_tile_rows(name, M, script):
    """launch_tile's big tile on the launches that are not LDS-DMA eligible: the f32 input projection with the position
    table (seq_len 100: the table wraps inside a tile), the norm-1 forms of the single residual stream, the f32-operand
    forms of MT3_OPT_ENCODER_F32_MFMA, and bf16 K = 96"""
    run(name, script, M)


@pytest.mark.parametrize("script", SCRIPTS)
@pytest.mark.parametrize("name", OTHER)
def test_other_big_tile_instantiations(name, script):
    """the remaining gemm_kernel instantiations launch_gemm can select with small = 0, two tiles, the second with one row"""
    run(name, script, 129)


# ------------------------------------------------------------------------------------------------------- rolled rows
@pytest.mark.parametrize("name,M,seq", [(n, 300, None) for n in GLDS + BIG + ["mfma_wo_ss", "resid_k96"]
                                         if E.FORMS[n].epi != E.EPI_GEGLU and E.FORMS[n].epi != E.EPI_POS] +
                         [("enc_cross_kv", 300, 100), ("mfma_cross_kv", 300, 100), ("ring_f32out_k64", 1147, None),
                          ("enc_qkv_tall", 113 * 256 + 37, None), ("enc_cross_kv_tall", 43800, 100)])
def test_rolled_rows(name, M, seq):
    """Random script.  The same rows rolled by 176 positions -- a multiple of 16, so a row keeps its MFMA lane, and no
    multiple of 64, so it changes fragment, wave, 64-row pass and tile, and moves into or out of the ragged last tile --
    must give every row the same bits at its new position: STORE, F32, RESID (with its by-products) and HEADS."""
    a, b = run(name, "random", M, seq=seq), run(name, "random", M, seq=seq, roll=True)
    for k in a:
        bad = E.bits(torch.roll(a[k][:M], E.ROLL, 0).contiguous()) != E.bits(b[k][:M].contiguous())
        assert not bool(bad.any()), f"{k}: a row's bits depend on its position: (rolled positions) " + E.where(bad)
