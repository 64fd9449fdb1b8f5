"""The decode-sized GEMM tiles (gemm.hip: gemm_kernel through launch_tile) in the forms enqueue_chain_op (engine.hip)
launches them in, through mt3_op_gemm_decode, against the float64 reference of tests/decode_gemm_ref.py on the same
(already rounded) operands.

Forms (FORMS below), named after the op of a decoder layer that launches them:

  mt3_op0     StoreQ  N = 4 HD, n_split = 3 HD, norm 2, ld2 = 0        the q-fold without the qkv-fold (kEpiStoreQ)
  mt3_op2     ResidQ  K = HD, N = emb + HD; out2 dense (ld2 = 0: the plain q-fold) or at column 3 HD of a [M][4 HD]
                      buffer with ld2 = 4 HD (the qkv-fold: the cross query's columns of the next op 4)
  mt3_op5     RESID   K = HD, N = emb, with out_ct / out_ss            every step's cross-attention out-projection
  mt3_op6     GEGLU   norm 2, K = emb, N = 2 mlp                       the GEGLU launch without the qkv-fold
  mt3_op6p    GegluP  the same with 1568 side columns (a width that ends mid-tile) behind it
  base_*      the ismir2022/base.gin shape (bf16, emb = HD = 768, mlp 2048): op 0 StoreQ, op 6 GEGLU, op 5 RESID and op 2
              ResidQ at K = 768, op 7 RESID at K = 2048

Bounds: the ones the project states for each epilogue (tests/test_gpu_kernels.py, tests/test_gpu_fold_side_product.py):
STORE 6e-3 bf16 / 2e-5 f32 rel-L2, RESID / f32 outputs / side products 2e-5, GEGLU 8e-3 bf16 / 3e-5 f32, out_ss 1e-5
relative, out_ct bit-equal to the rounding of the f32 rows, worst side-product row 1e-4.  K = 768 and K = 2048 had no
decode-sized bound of their own; the same ones are asserted, next to the error of a plain f32-accumulated torch.matmul
of the same operands pushed through the same epilogue (printed by every base.gin case; see BASELINE below).

Guards around every launch: each output has one more row than the launch has, filled like the rest of the buffer with
values no result equals, and everything outside rows [0, M) x the region's columns must come back bit for bit
(decode_gemm_ref.untouched): the guard row, the q | k | v columns of a strided side region, the next row's head.
Every case prints its measured errors.
"""
import ctypes as C
import dataclasses
import functools
import zlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import decode_gemm_ref as R  # noqa: E402

BF16, F32 = _lib.MT3_BF16, _lib.MT3_F32
EMB, HD, MLP = 512, 384, 1024                  # the MT3 shape
BEMB, BHD, BMLP = 768, 768, 2048               # ismir2022/base.gin
STORE, RESID, GEGLU = _lib.EPI_STORE, _lib.EPI_RESID, _lib.EPI_GEGLU
BOUND = {(STORE, BF16): 6e-3, (STORE, F32): 2e-5, (RESID, BF16): 2e-5, (RESID, F32): 2e-5, (GEGLU, BF16): 8e-3,
         (GEGLU, F32): 3e-5}
SIDE_BOUND, SIDE_ROW_BOUND, SS_BOUND = 2e-5, 1e-4, 1e-5
# BASELINE, measured on MI355X for the K = 768 / K = 2048 forms (bf16), worst M of each form: rel-L2 against float64 of
# the kernel | of an f32-accumulated torch.matmul of the same operands through the same epilogue.  The kernel stays inside
# the project's bound for the epilogue in every form, so that bound is the one asserted (no 4 x baseline margin needed):
#   base_op0 StoreQ  K 768   primary 1.658e-3 | 1.658e-3 (bound 6e-3: the bf16 rounding of the output), side 1.56e-7 | 1.00e-7
#   base_op6 GEGLU   K 768   primary 1.668e-3 | 1.668e-3 (bound 8e-3)
#   base_op5 RESID   K 768   primary 1.14e-7  | 1.50e-7  (bound 2e-5), out_ss 1.4e-7
#   base_op2 ResidQ  K 768   primary 1.14e-7  | 1.51e-7  (bound 2e-5), side 2.7e-8 | 2.7e-8, out_ss 1.5e-7
#   base_op7 RESID   K 2048  primary 1.92e-7  | 1.21e-7  (bound 2e-5), out_ss 1.3e-7
# The MT3 shape, worst over all cases: bf16 STORE 1.69e-3, GEGLU 1.63e-3, RESID 9.3e-8, side products 1.3e-7 (row 1.4e-7);
# f32 STORE 4.2e-7, GEGLU 6.3e-7, RESID 2.7e-7, side products 4.1e-7 (row 4.6e-7); out_ss 1.6e-7.
# Every bit comparison of this file (64-row against 32-row tile, one against two K slices, slices that start mid-tile)
# held on the first run.
KG = {BF16: 32, F32: 16}                       # elements of one MFMA K-group (CTraits<CT>::KGROUP)


@dataclasses.dataclass(frozen=True)
class Form:
    epi: int
    K: int
    n1: int                  # weight rows of the primary region (GEGLU: gate + linear)
    ns: int = 0              # columns of the second product (0: none)
    norm: int = 0
    col0: int = 0            # where the side region starts in a row of the out2 buffer
    ld2: int = 0             # row stride of the out2 buffer as passed (0: the side width)
    by: bool = False         # RESID by-products: out_ss, and with bf16 out_ct
    rows: int = 321          # rows of operands and reference (cases use the first M)


FORMS = {
    "mt3_op0": Form(STORE, EMB, 3 * HD, HD, norm=2, rows=65),
    "mt3_op2_dense": Form(RESID, HD, EMB, HD, by=True),
    "mt3_op2_strided": Form(RESID, HD, EMB, HD, col0=3 * HD, ld2=4 * HD, by=True),
    "mt3_op5": Form(RESID, HD, EMB, by=True, rows=513),
    "mt3_op6": Form(GEGLU, EMB, 2 * MLP, norm=2),
    "mt3_op6p": Form(GEGLU, EMB, 2 * MLP, 1568, norm=2, rows=33),
    "base_op0": Form(STORE, BEMB, 3 * BHD, BHD, norm=2, rows=96),
    "base_op6": Form(GEGLU, BEMB, 2 * BMLP, norm=2, rows=129),
    "base_op5": Form(RESID, BHD, BEMB, by=True),
    "base_op2": Form(RESID, BHD, BEMB, BHD, by=True, rows=161),
    "base_op7": Form(RESID, BMLP, BEMB, by=True, rows=65),
}


def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """operands of a form on the GPU and the float64 reference of all its rows, computed once"""
    f, ct = FORMS[name], tdt(dtype)
    seed = zlib.crc32(name.encode()) % 10000 + 17 * dtype
    c = dict(form=f, a_ss=None, out0=None, side0=None)
    if f.norm == 2:
        c["A"] = R.residual_rows(f.rows, f.K, seed).to(ct)
        c["a_ss"] = R.partial_sums(c["A"])
    else:
        c["A"] = R.activations(f.rows, f.K, seed, ct)
    if f.epi == GEGLU:
        c["Wt"] = R.geglu_weight(f.n1 // 2, f.K, seed + 1, ct, n_side=f.ns)[0]
    else:
        c["Wt"] = R.weight(f.n1 + f.ns, f.K, seed + 1, ct)
    c["N"] = c["Wt"].shape[0]
    g = torch.Generator().manual_seed(seed + 5)
    if f.epi == RESID:
        c["out0"] = torch.randn(f.rows, f.n1, generator=g)
        if f.ns:
            c["side0"] = torch.randn(f.rows, f.ns, generator=g) * 20
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            c[k] = v.cuda()
    c["primary"], c["side"] = R.evaluate(A=c["A"], Wt=c["Wt"], M=f.rows, N=c["N"], K=f.K, epilogue=f.epi, ct=ct,
                                         norm=f.norm, a_ss=c["a_ss"], out=c["out0"], n_split=f.n1 if f.ns else 0,
                                         ld2=f.ns if f.epi == GEGLU else 0, side=c["side0"])
    return c


def launch(dtype, **f):
    """one mt3_op_gemm_decode call; tensors (views: their first element) for the pointers"""
    ptrs = ("A", "Wt", "out", "a_ss", "out_ct", "out_ss", "out2")
    v = _lib.GemmView(**{k: ((None if x is None else x.data_ptr()) if k in ptrs else int(x)) for k, x in f.items()})
    _lib.check(_lib.load().mt3_op_gemm_decode(dtype, C.byref(v), torch.cuda.current_stream().cuda_stream))


def garbage(rows, cols, dt, seed):
    """values no result equals (and no two alike enough for a misplaced store to go unnoticed)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(rows, cols, device="cuda", generator=g) * 300 + 7777).to(dt)


def run(name, dtype, M, concurrent=0, piece=None):
    """The form on its first M rows -- in one launch, or in row slices of `piece` rows -- with every check of this file.
    Returns the outputs (for bit comparisons between launches of the same product)."""
    c = case(name, dtype)
    f, ct = c["form"], tdt(dtype)
    assert M <= f.rows
    geglu, resid = f.epi == GEGLU, f.epi == RESID
    wout = f.n1 // 2 if geglu else f.n1
    out = garbage(M + 1, wout, torch.float32 if resid else ct, 1)
    if resid:
        out[:M] = c["out0"][:M]
    out_ss = garbage(M + 1, wout // 16, torch.float32, 2) if f.by else None
    out_ct = garbage(M + 1, wout, torch.bfloat16, 3) if f.by and dtype == BF16 else None
    side = None
    if f.ns:
        side = garbage(M + 1, f.ld2 if f.ld2 else f.ns, torch.float32, 4)
        if resid:
            side[:M, f.col0:f.col0 + f.ns] = c["side0"][:M]
    before = [None if t is None else t.clone() for t in (out, out_ss, out_ct, side)]
    for r0 in range(0, M, piece or M):
        m = min(piece or M, M - r0)
        launch(dtype, A=c["A"][r0:], Wt=c["Wt"], out=out[r0:], M=m, N=c["N"], K=f.K, lda=0, ldo=wout, a_is_f32=0,
               norm=f.norm, epilogue=f.epi, a_ss=None if c["a_ss"] is None else c["a_ss"][r0:],
               out_ct=None if out_ct is None else out_ct[r0:], out_ss=None if out_ss is None else out_ss[r0:],
               out2=None if side is None else side[r0:, f.col0:], n_split=f.n1 if f.ns else 0,
               ld2=(f.ns if geglu else f.ld2) if f.ns else 0, concurrent=concurrent)
    torch.cuda.synchronize()
    tag = f"{name} dtype {dtype} M {M} concurrent {concurrent} piece {piece}:"
    e = R.rel(out[:M], c["primary"][:M])
    print(tag, f"primary rel-L2 {e:.3e} (bound {BOUND[(f.epi, dtype)]:.0e})")
    assert e < BOUND[(f.epi, dtype)], e
    assert R.untouched(out, before[0], M, 0, wout), "the primary region wrote outside its rows"
    if f.by:
        ct_ref, ss_ref = R.by_products(out[:M], torch.bfloat16)
        e_ss = float(((out_ss[:M].double() - ss_ref).abs() / ss_ref).max())
        print(tag, f"out_ss worst relative error {e_ss:.3e}")
        assert e_ss < SS_BOUND, e_ss
        assert R.untouched(out_ss, before[1], M, 0, wout // 16)
        if out_ct is not None:
            assert torch.equal(out_ct[:M], ct_ref), "out_ct is not the rounding of the f32 rows"
            assert R.untouched(out_ct, before[2], M, 0, wout)
    if f.ns:
        got = side[:M, f.col0:f.col0 + f.ns]
        e_s, e_r = R.rel(got, c["side"][:M]), R.worst_row(got, c["side"][:M])
        print(tag, f"second product rel-L2 {e_s:.3e}, worst row {e_r:.3e}")
        assert e_s < SIDE_BOUND and e_r < SIDE_ROW_BOUND, (e_s, e_r)
        assert R.untouched(side, before[3], M, f.col0, f.ns), "the second product wrote outside its region"
    return [t for t in (out, out_ss, out_ct, side) if t is not None]


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def wgs(M, N, bm=32, bn=32):
    """workgroups of a launch on bm x bn tiles: what launch_tile's thresholds count"""
    return ((M + bm - 1) // bm) * (N // bn)


def f32_model(name, dtype, M):
    """rel-L2 against float64 of the same launch evaluated by an f32-accumulated torch.matmul and f32 epilogue math:
    what a different summation order costs at this K (primary region; second product or None)"""
    c = case(name, dtype)
    f, ct = c["form"], tdt(dtype)
    a, w = c["A"][:M].float(), c["Wt"].float()
    rs = R.row_scales(f.norm, c["A"][:M], None if c["a_ss"] is None else c["a_ss"][:M], f.K).float()
    P = (a @ w[:f.n1].T) * rs
    if f.epi == GEGLU:
        g = P.view(M, f.n1 // 32, 2, 16)
        P = (R.gelu_tanh(g[:, :, 0]) * g[:, :, 1]).reshape(M, f.n1 // 2).to(ct)
    elif f.epi == RESID:
        P = c["out0"][:M] + P
    else:
        P = P.to(ct)
    s = None
    if f.ns and f.epi != GEGLU:
        S = a @ w[f.n1:].T
        s = R.rel(c["side0"][:M] + S if f.epi == RESID else S, c["side"][:M])
    return R.rel(P, c["primary"][:M]), s


# ------------------------------------------------------------------------------------------------------- the MT3 shape
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("M", [1, 31, 65])
def test_mt3_op0_store_with_the_cross_query_columns(dtype, M):
    """enqueue_chain_op case 0 with e->q_fold and without the qkv-fold: normed_gemm(L.wqkv_ext, kEpiStoreQ), N = 4 HD,
    n_split = 3 HD, norm 2, ld2 = 0 -> q | k | v in the compute type with 1/rms, the cross query unscaled in f32.
    launch_tile: K = 512 is `deep` -- bf16 32 x 32 x 512 in one slice, f32 32 x 32 x 256 in two."""
    assert FORMS["mt3_op0"].K % (16 * KG[dtype]) == 0
    run("mt3_op0", dtype, M)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("layout", ["strided", "dense"])
@pytest.mark.parametrize("M", [1, 31, 33, 64, 65, 288, 289])
def test_mt3_op2_resid_with_the_cross_query_product(dtype, layout, M):
    """enqueue_chain_op case 2 with e->q_fold: resid_gemm(L.wo_ext, kEpiResidQ), K = HD = 384, N = emb + HD, with out_ct /
    out_ss.  strided: the qkv-fold's out2 = qkvf + 3 HD, ld2 = 4 HD (the epilogue's accumulate AND the xpre preload
    index through ld2; q | k | v in front must come back bit for bit); dense: the plain q-fold's ld2 = 0.
    launch_tile: bf16 K = 12 KG -> 32 x 32 x 384 in one slice; f32 K = 24 KG -> one slice while the launch has <= 256
    workgroups, two slices of 12 KG above: M = 288 / 289 straddle the switch."""
    N = EMB + HD
    assert wgs(288, N) == 252 <= 256 < wgs(289, N) == 280
    run("mt3_op2_" + layout, dtype, M)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("M", [1, 31, 33, 65])
def test_mt3_op5_resid_with_by_products(dtype, M):
    """enqueue_chain_op case 5: resid_gemm(L.wo_x, MT3_EPI_RESID), K = HD = 384, N = emb, with out_ct / out_ss (bf16) or
    out_ss alone (f32).  launch_tile: bf16 32 x 32 x 384 (K = 12 KG), f32 32 x 32 x 384 (K = 24 KG, <= 256 workgroups)."""
    assert wgs(65, EMB) <= 256
    run("mt3_op5", dtype, M)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_mt3_op6_geglu_side_columns_end_mid_tile(dtype):
    """enqueue_chain_op case 6 under the qkv-fold: normed_gemm(L.wi, kEpiGegluP) with a side width of 1568 (not a multiple
    of the 64-column tile): the weight's padding rows hold 1e30 and their columns are never stored -- they would land in
    the next row's head or, for the last row, in the guard row.  launch_tile: kGeglu, `deep` -> 32 x 64 x 16 KG."""
    run("mt3_op6p", dtype, 33)


@pytest.mark.parametrize("name", ["mt3_op5", "mt3_op6", "mt3_op2_strided"])
@pytest.mark.parametrize("M", [256, 257, 300, 321])
def test_f32_64_row_tile_against_float64_and_the_32_row_tile(name, M):
    """GemmArgs::concurrent with f32 operands and M >= 256: launch_tile's 64 x 32 x 128 tile (four waves stacked along
    M), as the row groups of a 1024+ slot engine launch it -- plain RESID (case 5; K = 384 in three slices), plain GEGLU
    (case 6 without the qkv-fold, norm 2; K = 512 in four) and ResidQ with the strided out2 (case 2).  Each against
    float64, and bit for bit against the same launch with concurrent = 0 (the 32-row tiles: for M >= 289 case 2 takes
    two 12 KG slices there)."""
    assert M >= 256 and FORMS[name].K % (8 * KG[F32]) == 0
    tall = run(name, F32, M, concurrent=1)
    short = run(name, F32, M, concurrent=0)
    assert same_bits(tall, short), "the 64-row and the 32-row tile must produce identical outputs"


@pytest.mark.parametrize("name", ["mt3_op5", "mt3_op6", "mt3_op2_strided"])
def test_f32_255_concurrent_rows_stay_on_the_32_row_tile(name):
    """one row below launch_tile's `g.M >= 256`: concurrent = 1 changes nothing"""
    assert same_bits(run(name, F32, 255, concurrent=1), run(name, F32, 255, concurrent=0))


# ------------------------------------------------------------------------------------------ ismir2022/base.gin, bf16
def _base(name, M):
    out = run(name, BF16, M)
    e, s = f32_model(name, BF16, M)
    print(f"{name} M {M}: an f32-accumulated torch.matmul through the same epilogue: rel-L2 {e:.3e}"
          + ("" if s is None else f", second product {s:.3e}"))
    return out


@pytest.mark.parametrize("M", [64, 96])
def test_base_op0_store_with_the_cross_query_columns(M):
    """enqueue_chain_op case 0 at the base.gin shape (q-fold, no qkv-fold): kEpiStoreQ, K = 768, N = 3072, n_split = 2304,
    norm 2 from 48 partial sums (NPV = 16).  launch_tile: K = 24 KG -> 32 x 32 x 768 in ONE slice while the launch has
    <= 256 workgroups (M = 64: 192), two slices of 12 KG above (M = 96: 288).  The weight is over 3 MB: n_major dealing."""
    assert wgs(64, 4 * BHD) == 192 <= 256 < wgs(96, 4 * BHD) == 288
    _base("base_op0", M)


@pytest.mark.parametrize("M", [128, 129])
def test_base_op6_geglu(M):
    """enqueue_chain_op case 6 without the qkv-fold at the base.gin shape: MT3_EPI_GEGLU, norm 2, K = 768, N = 4096.
    launch_tile: 32 x 64 x 768 in one slice at <= 256 workgroups (M = 128: 256), 32 x 64 x 384 twice above (M = 129:
    320)."""
    assert wgs(128, 2 * BMLP, bn=64) == 256 and wgs(129, 2 * BMLP, bn=64) == 320 > 256
    _base("base_op6", M)


@pytest.mark.parametrize("M", [160, 161, 320, 321])
def test_base_op5_resid_k768(M):
    """enqueue_chain_op cases 2 (no q-fold) / 5 at the base.gin shape: MT3_EPI_RESID, K = 768, N = 768, out_ct / out_ss.
    launch_tile: 24 workgroups per row block, so M = 160 / 161 (120 / 144) both take the one-slice 32 x 32 x 768 tile;
    the two-slice tile starts at M = 321 (264 workgroups; M = 320: 240)."""
    assert wgs(161, BEMB) == 144 <= 256 and wgs(320, BEMB) == 240 <= 256 < wgs(321, BEMB) == 264
    _base("base_op5", M)


@pytest.mark.parametrize("M", [160, 161])
def test_base_op2_resid_with_the_cross_query_product_k768(M):
    """enqueue_chain_op case 2 with the q-fold at the base.gin shape: kEpiResidQ, K = 768, N = 768 + 768, ld2 = 0, out_ct
    / out_ss.  launch_tile: one slice of 24 KG at M = 160 (240 workgroups), two of 12 KG at M = 161 (288)."""
    assert wgs(160, 2 * BEMB) == 240 <= 256 < wgs(161, 2 * BEMB) == 288
    _base("base_op2", M)


def test_base_op7_resid_k2048():
    """enqueue_chain_op default case (op 7) at the base.gin shape: MT3_EPI_RESID, K = mlp = 2048, N = 768, out_ct /
    out_ss.  launch_tile: K is neither 24 KG nor 12 KG and `deep` -> 32 x 32 x 512, four slices."""
    assert BMLP % (16 * KG[BF16]) == 0 and BMLP not in (24 * KG[BF16], 12 * KG[BF16])
    _base("base_op7", 65)


# ------------------------------------------------------------------------------------------------ threshold invariance
@pytest.mark.parametrize("name,dtype,M,piece,bn", [
    ("mt3_op2_strided", F32, 289, 161, 32), ("mt3_op2_dense", F32, 289, 161, 32), ("mt3_op5", F32, 513, 290, 32),
    ("base_op0", BF16, 96, 49, 32), ("base_op6", BF16, 129, 97, 64), ("base_op2", BF16, 161, 97, 32),
    ("base_op5", BF16, 321, 193, 32)])
def test_one_and_two_k_slices_give_the_same_bits(name, dtype, M, piece, bn):
    """Every form above whose tile depends on the launch's workgroup count (one K slice at <= 256 workgroups, two above),
    at an M above the threshold and again in row slices that stay below it (the slices start mid-tile: a row's result
    does not depend on where in a tile it lands).  Both meet the float64 bound; and since the accumulator chain of an
    output element runs over the K-groups in order whatever BK is, and the norm-2 row scale depends on the row's partial
    sums alone, they are bit-identical."""
    N = case(name, dtype)["N"]
    assert wgs(M, N, bn=bn) > 256 >= wgs(piece, N, bn=bn) and M - piece <= piece
    assert same_bits(run(name, dtype, M), run(name, dtype, M, piece=piece)), "one and two K slices differ"
