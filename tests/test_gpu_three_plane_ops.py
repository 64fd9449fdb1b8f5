"""The f32 engine's three-plane kernels alone: planes_kernel (mt3_op_planes), gemm_x6_kernel (mt3_op_gemm_x6) and
enc_attn_x6_kernel (mt3_op_encoder_attention_x6); include/mt3_hip.h states their rules.

What each check would catch:
  planes, bit-equal to the host rule    a plane rounded another way than to nearest even, a remainder taken from the
                                        rounded instead of the exact difference, a carry into the exponent mishandled
                                        (all-ones mantissas), signs of zero, an index past n (n = 255 / 256 / 257 around
                                        the 256-thread block; the sentinels behind n)
  gemm_x6 against float64               a wrong product set or plane pairing, a K slice dropped or doubled (K = 64: the
                                        steady-state loop never runs; 512 and 1024: it does), wrong row statistics
                                        (rows carry scales 1 .. 4), the epilogue's addressing (GEGLU interleave, POS row
                                        modulo, HEADS permutation)
  ragged M (1, 64, 130, 192)            a store at or past row M (sentinels up to the next multiple of 128 rows), RESID
                                        reading or rewriting rows past M, a clamped load that leaks into a stored row
  placement                             rows [0, M) of the ragged launch against the same rows in a launch of 256 rows
                                        with other rows behind them, and (STORE / GEGLU / RESID) with five other rows in
                                        FRONT of them, bit for bit: a row's result and its RMSNorm statistics must not
                                        depend on its place in the tile or on its neighbours
  encoder_attention_x6                  test_encoder_attention's inputs and reference (tests/test_gpu_kernels.py); every
                                        form and scripted case: tests/test_gpu_encoder_attention_forms.py

Bounds: rel-L2 against float64 on the same f32 operands (row rms in double).  Each case takes the SMALLER of the f32 figure
of tests/test_gpu_kernels.py for the same shape of product (2e-5; 3e-5 for GEGLU and the attention) and HALF the smallest
error among the three five-product emulations on its own operands (score_prefill_ref.x6_bound, encoder_attention_ref
.x6_bounds: the kernel's six plane products summed in float64, and with mid.mid, hi.lo or lo.hi left out) -- 1.1e-6 to
1.3e-6 for the GEMM cases, 1.5e-6 to 1.8e-6 for GEGLU, 2.5e-6 for the attention, where a five-product kernel would show
2.3e-6 or more (5e-6 in the attention) and passed the old figures with a factor of five to spare.  The six-product
emulation has to stay under a quarter of the bound (6e-9 to 2e-8: every case does, GEGLU M = 1 included;
CANNOT_TELL_FIVE_FROM_SIX would name a case that did not and keeps the old figure).  Every case prints its value next to
what mt3_op_gemm(MT3_F32, ...) -- the f32 matrix instruction -- gives on the same operands; no ratio of the two is
asserted.
MEASURED on MI355X (worst over the cases of each kind; x6 / f32 instruction): see MEASURED below.  Case by case the
three-plane tile is below the f32 instruction in 51 of 52 GEMM cases and both attention cases; the exception is the
single row of GEGLU M = 1 (7.7e-7 against 4.6e-7).  planes: bit-equal at every n.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import encoder_attention_ref as ER  # noqa: E402
from tests import score_prefill_ref as R  # noqa: E402

E = _lib
MEASURED = {"STORE": "5.3e-7 / 6.5e-7", "GEGLU": "7.7e-7 / 6.4e-7", "RESID": "5.1e-7 / 6.2e-7", "POS": "5.1e-7 / 6.2e-7",
            "HEADS": "5.2e-7 / 6.3e-7", "attention": "5.2e-7 / 8.2e-7"}
# smallest bound of each kind under the five-product rule (before: 2e-5; 3e-5 for GEGLU and the attention)
BOUNDS = {"STORE": 1.2e-6, "GEGLU": 1.47e-6, "RESID": 1.06e-6, "POS": 1.06e-6, "HEADS": 1.2e-6, "attention": 2.57e-6}
SENTINEL = -7.5


def stream():
    return torch.cuda.current_stream().cuda_stream


def rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ planes
def plane_inputs():
    """100003 f32 values: the edge cases first (so that n = 1 and n = 255 meet them), then normals over 60 binades"""
    rng = np.random.default_rng(0)
    ones = np.array([(e << 23) | 0x7FFFFF for e in (64, 100, 127, 128, 160, 253)], np.uint32)    # all-ones mantissas
    ones = np.concatenate([ones, ones | 0x80000000]).view(np.float32)
    top = np.array([0x7F7F0000, 0xFF7F0000, 0x7F7E0000, 0xFF7E0000], np.uint32).view(np.float32)  # largest finite bf16
    half = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0x3F807FFF, 0x3F808001], np.uint32).view(np.float32)  # ties
    edge = np.concatenate([ones[:1], np.float32([0.0, -0.0]), ones[1:], top, half])
    n = 100003 - len(edge)
    body = rng.standard_normal(n).astype(np.float32) * np.exp2(rng.integers(-30, 31, n)).astype(np.float32)
    return np.concatenate([edge, body]).astype(np.float32)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_planes_are_the_host_split(n):
    w = plane_inputs()[:n]
    guard = 64
    out = [torch.full((n + guard,), 0x7BCD, device="cuda", dtype=torch.int16) for _ in range(3)]
    d = torch.from_numpy(w).cuda()
    _lib.check(_lib.load().mt3_op_planes(d.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n, stream()))
    torch.cuda.synchronize()
    for name, got, want in zip(("hi", "mid", "lo"), out, R.planes_ref(w)):
        got = got.cpu().numpy().view(np.uint16)
        bad = np.nonzero(got[:n] != want)[0]
        assert len(bad) == 0, (name, len(bad), [(hex(w[i:i + 1].view(np.uint32)[0]), hex(got[i]), hex(want[i])) for i in bad[:5]])
        assert (got[n:] == 0x7BCD).all(), (name, "a store at or past n")
    # the three terms are the value: hi + mid + lo within 2^-26 |w| (tests/test_three_plane_arithmetic.py)
    terms = [t[:n].view(torch.bfloat16).double().cpu().numpy() for t in out]
    rem = np.abs(w.astype(np.float64) - terms[0] - terms[1] - terms[2])
    assert (rem <= np.abs(w.astype(np.float64)) * 2.0 ** -26).all()


# ----------------------------------------------------------------------------------------------------------- gemm_x6
def make_planes(W):
    """W f32 [N][K] on the GPU -> its three bf16 planes through mt3_op_planes (checked above)"""
    p = [torch.empty(W.shape, device="cuda", dtype=torch.bfloat16) for _ in range(3)]
    _lib.check(_lib.load().mt3_op_planes(W.data_ptr(), p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), W.numel(), stream()))
    return p


def gemm_x6(A, planes, norm, epi, out, M, N, K, aux=None, seq_len=0):
    _lib.check(_lib.load().mt3_op_gemm_x6(A.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
                                          int(norm), epi, out.data_ptr(), M, N, K, aux.data_ptr() if aux is not None else None,
                                          seq_len, stream()))
    torch.cuda.synchronize()


def gemm_f32(A, W, norm, epi, out, M, N, K, aux=None, seq_len=0):
    """the f32 matrix instruction on the same operands (large tile); -> False if that op has no such launch"""
    a_f32 = int(norm or epi == E.EPI_POS)                  # the forms tests/test_gpu_kernels.py launches
    rc = _lib.load().mt3_op_gemm(E.MT3_F32, A.data_ptr(), a_f32, int(norm), W.data_ptr(), out.data_ptr(), M, N, K, epi,
                                 aux.data_ptr() if aux is not None else None, seq_len, 0, stream())
    torch.cuda.synchronize()
    return rc == E.MT3_OK


TODAY = {"STORE": 2e-5, "RESID": 2e-5, "POS": 2e-5, "HEADS": 2e-5, "GEGLU": 3e-5}     # the bounds before the five-product rule
CANNOT_TELL_FIVE_FROM_SIX = ()                          # (epi, M, N, K) whose six-product emulation is not under a quarter


CASES = [(epi, M, N, K) for epi in ("STORE", "RESID", "POS", "HEADS") for M in (1, 64, 130, 192)
         for N, K in ((128, 64), (1152, 512), (512, 1024))] + [("GEGLU", M, 256, 512) for M in (1, 64, 130, 192)]


@pytest.mark.parametrize("epi,M,N,K", CASES)
def test_gemm_x6(epi, M, N, K):
    what = f"gemm_x6 {epi} M {M} N {N} K {K}"
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
    MP, Mr = 256, (M + 127) // 128 * 128                  # rows of the padded launch; rows the ragged launch's tiles cover
    norm = epi in ("STORE", "GEGLU")
    code = {"STORE": E.EPI_STORE, "RESID": E.EPI_RESID, "POS": E.EPI_POS, "HEADS": E.EPI_HEADS, "GEGLU": E.EPI_GEGLU}[epi]
    seq = {1: 1, 64: 64, 130: 65, 192: 64}[M] if epi == "HEADS" else 64 if epi == "POS" else 0
    # MP rows of A: the first M are the case's, the others stand behind them in the padded launch
    A_all = torch.randn(MP + 5, K, device="cuda", generator=g) * (1 + 3 * torch.rand(MP + 5, 1, device="cuda", generator=g))
    A = A_all[:M].contiguous()
    W = torch.randn(N, K, device="cuda", generator=g) / math.sqrt(K)
    aux = torch.randn(seq, N, device="cuda", generator=g) if epi == "POS" else None
    res_all = torch.randn(MP + 5, N, device="cuda", generator=g)
    NO = N // 2 if epi == "GEGLU" else N                  # output columns
    planes = make_planes(W)
    # ---- float64 reference on the same f32 operands, and the bound from the five-product emulations on them
    finish = lambda prod: R.x6_epilogue(epi, prod, A, res_all[:M], aux, seq)
    ref = finish(A.double() @ W.double().T)
    tol, tells, six, five = R.x6_bound(TODAY[epi], lambda drop: rel(finish(R.plane_product(A, W, drop)), ref))
    assert tells or (epi, M, N, K) in CANNOT_TELL_FIVE_FROM_SIX, (what, six, five)

    def out_buffer(rows):
        """the launch's output with sentinels behind it up to `rows` rows (HEADS: as many elements)"""
        buf = torch.full((rows * NO,), SENTINEL, device="cuda")
        if epi == "RESID":
            buf[:] = res_all[:rows].reshape(-1)
        return buf

    # ---- the ragged launch
    buf = out_buffer(Mr)
    gemm_x6(A, planes, norm, code, buf, M, N, K, aux, seq)
    out = buf[:M * NO].view(ref.shape)
    tail = buf[M * NO:]
    if epi == "RESID":
        assert same(tail, res_all[M:Mr].reshape(-1)), (what, "RESID touched rows past M")
    else:
        assert bool((tail == SENTINEL).all()), (what, "a store past row M")
    err = rel(out, ref)
    o32 = out_buffer(Mr)
    f32 = f"{rel(o32[:M * NO].view(ref.shape), ref):.3e}" if gemm_f32(A, W, norm, code, o32, M, N, K, aux, seq) \
        else "no F32 counterpart through mt3_op_gemm"
    print(f"{what}: rel-L2 {err:.3e} (bound {tol:.2e}: today's {TODAY[epi]:.0e}, six products {six:.2e}, without "
          + ", ".join(f"{n} {e:.2e}" for n, e in five.items()) + f"); mt3_op_gemm(F32) on the same operands: {f32}")
    assert torch.isfinite(out).all() and err < tol, (what, err)
    # ---- placement: 256 rows, the case's rows first
    if epi != "HEADS" or MP % seq == 0:
        big = out_buffer(MP)
        gemm_x6(A_all[:MP].contiguous(), planes, norm, code, big, MP, N, K, aux, seq)
        if epi == "HEADS":
            got = big.view(2, MP // seq, N // 128, seq, 64)[:, :M // seq]
        else:
            got = big.view(MP, NO)[:M].view(ref.shape)
        assert same(got.contiguous(), out.contiguous()), (what, "rows differ from the launch padded to 256 rows")
    # ---- and five other rows in front of them: every row sits at another place of its tile
    if epi in ("STORE", "GEGLU", "RESID"):
        rows = M + 5
        A5 = torch.cat([A_all[MP:MP + 5], A]).contiguous()
        b5 = torch.full((rows * NO,), SENTINEL, device="cuda")
        if epi == "RESID":
            b5[:] = torch.cat([res_all[MP:MP + 5], res_all[:M]]).reshape(-1)
        gemm_x6(A5, planes, norm, code, b5, rows, N, K, aux, seq)
        assert same(b5.view(rows, NO)[5:].contiguous(), out.contiguous()), (what, "rows differ when shifted by five rows")


# ------------------------------------------------------------------------------------------------ encoder attention
@pytest.mark.parametrize("T", [256, 512])
def test_encoder_attention_x6(T):
    B, H = 2, 6
    g = torch.Generator(device="cuda").manual_seed(T)
    qkv = torch.randn(B, T, 3, H, 64, device="cuda", generator=g)
    qkv[:, :, 0] *= 0.35                                   # unscaled logits: keep softmax non-degenerate
    guard = 4
    full = torch.full((B * T + 2 * guard, H * 64), SENTINEL, device="cuda")
    out = full[guard:guard + B * T]
    _lib.check(_lib.load().mt3_op_encoder_attention_x6(qkv.data_ptr(), out.data_ptr(), B, T, H, stream()))
    torch.cuda.synchronize()
    q, k, v = (qkv[:, :, i].double() for i in range(3))
    w = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k), -1)
    ref = torch.einsum("bhqk,bkhd->bqhd", w, v).reshape(B * T, H * 64)
    err = rel(out, ref)
    b = ER.x6_bounds(qkv, ref.view(B, T, H, 64))
    assert b["distinguishes"] and b["whole"] < 3e-5, b
    o32 = torch.zeros(B, T, H * 64, device="cuda")
    _lib.check(_lib.load().mt3_op_encoder_attention(E.MT3_F32, qkv.data_ptr(), o32.data_ptr(), B, T, H, stream()))
    torch.cuda.synchronize()
    print(f"encoder_attention_x6 T {T}: rel-L2 {err:.3e} (bound {b['whole']:.2e}: half the smallest five-product error, six "
          f"products {b['six'][0]:.2e}); mt3_op_encoder_attention(F32) on the same inputs: {rel(o32.view(B * T, H * 64), ref):.3e}")
    assert err < b["whole"], (err, b)
    assert bool((full[:guard] == SENTINEL).all()) and bool((full[guard + B * T:] == SENTINEL).all())
