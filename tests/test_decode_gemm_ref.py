"""tests/decode_gemm_ref.py on the CPU: the reference against plain torch float64 formulas on tiny shapes (every epilogue,
every norm, the second product stored / accumulated / placed at a stride), and the conditions the case generators of the
GPU tests promise -- every row rms >= 10, weights that make a transposed tile fail, padding weight rows of 1e30."""
import pytest

torch = pytest.importorskip("torch")
from tests import decode_gemm_ref as R  # noqa: E402

CTS = [torch.bfloat16, torch.float32]


def close(a, b):
    """float64 results of the same formula (BLAS may order a sum differently for another shape)"""
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    return True


def _tiny(ct, M=5, N=96, K=64, seed=3):
    x = R.residual_rows(M, K, seed)
    return x, x.to(ct), R.weight(N, K, seed + 1, ct)


@pytest.mark.parametrize("ct", CTS)
def test_store_and_f32_with_every_norm(ct):
    M, N, K = 5, 96, 64
    x, xc, w = _tiny(ct)
    plain = xc.double() @ w.double().T
    for epi in (R.EPI_STORE, R.EPI_F32):
        got, side = R.evaluate(A=xc, Wt=w, M=M, N=N, K=K, epilogue=epi, ct=ct)
        assert side is None and close(got, plain)
        # norm 1: statistics of the f32 rows, operand rounded to the compute type
        got, _ = R.evaluate(A=x, Wt=w, M=M, N=N, K=K, epilogue=epi, ct=ct, norm=1, a_is_f32=True)
        rs = 1 / torch.sqrt((x.double() ** 2).mean(-1, keepdim=True) + 1e-6)
        torch.testing.assert_close(got, plain * rs, rtol=1e-13, atol=0)
        # norm 2: statistics from the partial sums alone -- scripted ones, unrelated to the rows
        ss = torch.rand(M, K // 16) * 1000 + 1
        got, _ = R.evaluate(A=xc, Wt=w, M=M, N=N, K=K, epilogue=epi, ct=ct, norm=2, a_ss=ss)
        rs2 = 1 / torch.sqrt(ss.double().sum(-1, keepdim=True) / K + 1e-6)
        torch.testing.assert_close(got, plain * rs2, rtol=1e-13, atol=0)
    # fewer rows than the operands hold: the first M
    got, _ = R.evaluate(A=xc, Wt=w, M=2, N=N, K=K, epilogue=R.EPI_STORE, ct=ct)
    assert close(got, plain[:2])


@pytest.mark.parametrize("ct", CTS)
def test_geglu_interleave_against_torch_gelu(ct):
    M, F, K = 4, 48, 64
    x = R.residual_rows(M, K, 9)
    xc, ss = x.to(ct), R.partial_sums(x.to(ct))
    w, gate_t, lin_t, _ = R.geglu_weight(F, K, 11, ct)
    assert w.shape == (2 * F, K)
    # rows [32q, 32q + 16) are gate columns 16q .., rows [32q + 16, 32q + 32) the linear columns
    assert torch.equal(w[32:48], gate_t[16:32]) and torch.equal(w[48:64], lin_t[16:32])
    got, _ = R.evaluate(A=xc, Wt=w, M=M, N=2 * F, K=K, epilogue=R.EPI_GEGLU, ct=ct, norm=2, a_ss=ss)
    rs = torch.rsqrt(ss.double().sum(-1, keepdim=True) / K + 1e-6)
    ref = torch.nn.functional.gelu((xc.double() @ gate_t.double().T) * rs, approximate="tanh") * ((xc.double() @ lin_t.double().T) * rs)
    assert got.shape == (M, F)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("ct", CTS)
def test_resid_and_its_by_products(ct):
    M, N, K = 5, 96, 64
    a = R.activations(M, K, 5, ct)
    w = R.weight(N, K, 6, ct)
    y0 = torch.randn(M, N, generator=torch.Generator().manual_seed(7))
    got, _ = R.evaluate(A=a, Wt=w, M=M, N=N, K=K, epilogue=R.EPI_RESID, ct=ct, out=y0)
    assert close(got, y0.double() + a.double() @ w.double().T)
    rows = got.float()
    copy, ss = R.by_products(rows, ct)
    assert copy.dtype == ct and torch.equal(copy.float(), rows.to(ct).float())
    for r, c in ((0, 0), (4, 5)):
        assert float(ss[r, c]) == pytest.approx(float((rows[r, 16 * c:16 * c + 16].double() ** 2).sum()), rel=1e-14)


@pytest.mark.parametrize("ct", CTS)
def test_second_product_is_plain_unscaled_and_placed_at_a_stride(ct):
    M, n1, ns, K = 5, 64, 32, 64
    x = R.residual_rows(M, K, 21)
    xc, ss = x.to(ct), R.partial_sums(x.to(ct))
    w = R.weight(n1 + ns, K, 22, ct)
    rs = torch.rsqrt(ss.double().sum(-1, keepdim=True) / K + 1e-6)
    plain = xc.double() @ w.double().T
    # STORE: the primary columns carry 1/rms, the side columns do not
    p, s = R.evaluate(A=xc, Wt=w, M=M, N=n1 + ns, K=K, epilogue=R.EPI_STORE, ct=ct, norm=2, a_ss=ss, n_split=n1)
    torch.testing.assert_close(p, plain[:, :n1] * rs, rtol=1e-13, atol=0)
    assert close(s, plain[:, n1:])
    # RESID: both regions accumulate
    y0, s0 = torch.randn(M, n1), torch.randn(M, ns)
    p, s = R.evaluate(A=xc, Wt=w, M=M, N=n1 + ns, K=K, epilogue=R.EPI_RESID, ct=ct, out=y0, n_split=n1, side=s0)
    assert close(p, y0.double() + plain[:, :n1]) and close(s, s0.double() + plain[:, n1:])
    # at a stride inside a wider buffer: the other columns and the guard row stay bit for bit
    before = torch.randn(M + 1, 4 * ns)
    after = R.placed(before, s, col0=3 * ns)
    assert torch.equal(after[:M, 3 * ns:], s.float()) and torch.equal(after[:, :3 * ns], before[:, :3 * ns])
    assert torch.equal(after[M], before[M])
    assert R.untouched(after, before, M, 3 * ns, ns)
    for (r, c) in ((0, 3 * ns - 1), (M, 3 * ns), (M - 1, 0)):                       # left neighbour, guard row, next row's head
        spoiled = after.clone()
        spoiled[r, c] += 1
        assert not R.untouched(spoiled, before, M, 3 * ns, ns)
    # GEGLU: the weight rows are padded to whole tiles with 1e30, the side width is ld2 and nothing else is produced
    F, nside = 32, 40
    wg, gate_t, lin_t, side_t = R.geglu_weight(F, K, 23, ct, n_side=nside)
    assert wg.shape == (2 * F + 64, K)
    assert bool((wg[2 * F + nside:].float() == torch.tensor(R.PAD_WEIGHT).to(ct).float()).all())
    assert float(wg[2 * F + nside:].float().min()) > 9e29
    p, s = R.evaluate(A=xc, Wt=wg, M=M, N=2 * F + 64, K=K, epilogue=R.EPI_GEGLU, ct=ct, norm=2, a_ss=ss, n_split=2 * F, ld2=nside)
    assert p.shape == (M, F) and s.shape == (M, nside)
    assert close(s, xc.double() @ side_t.double().T) and float(s.abs().max()) < 1e6
    with pytest.raises(ValueError):
        R.evaluate(A=xc, Wt=w, M=M, N=n1 + ns, K=K, epilogue=R.EPI_F32, ct=ct, n_split=n1)


@pytest.mark.parametrize("ct", CTS)
@pytest.mark.parametrize("K", [384, 512, 768])
def test_generated_rows_make_a_misplaced_row_scale_an_order_one_error(ct, K):
    M = 321
    x = R.residual_rows(M, K, 1000 + K)
    xc = x.to(ct)
    ss = R.partial_sums(xc)
    rms = torch.sqrt(ss.double().sum(-1) / K)
    assert float(rms.min()) >= 10 and float(rms.max()) < 50
    assert float((torch.sqrt((x.double() ** 2).mean(-1))).min()) >= 10                    # norm 1 sees the f32 rows
    w = R.weight(128, K, 5, ct)
    p, s = R.evaluate(A=xc, Wt=w, M=M, N=128, K=K, epilogue=R.EPI_STORE, ct=ct, norm=2, a_ss=ss, n_split=64)
    unscaled = xc.double() @ w.double().T
    # the scale left out of the primary columns, or applied to the side columns: every ROW is off by a factor >= 10
    assert float(((unscaled[:, :64] - p).norm(dim=1) / p.norm(dim=1)).min()) > 9
    rs = torch.rsqrt(ss.double().sum(-1, keepdim=True) / K + 1e-6)
    assert float(((unscaled[:, 64:] * rs - s).norm(dim=1) / s.norm(dim=1)).min()) > 0.9


@pytest.mark.parametrize("ct", CTS)
def test_generated_weights_make_a_transposed_tile_fail(ct):
    M, N, K = 64, 64, 384
    a = R.activations(M, K, 31, ct)
    w = R.weight(N, K, 32, ct)
    p, _ = R.evaluate(A=a, Wt=w, M=M, N=N, K=K, epilogue=R.EPI_STORE, ct=ct)
    for t in (16, 32, 64):                                   # a C fragment, a wave's tile, a workgroup tile written transposed
        q = p.view(M // t, t, N // t, t).transpose(1, 3).reshape(M, N)
        assert R.rel(q, p) > 1.0
    # rows 4g + r of a fragment swapped for 4r + g (frag_g / r exchanged in a row index)
    q = p.view(M // 16, 4, 4, N).transpose(1, 2).reshape(M, N)
    assert R.rel(q, p) > 1.0 and R.worst_row(q, p) > 1.0
    # the weight itself: no symmetry a transposed operand tile could hide behind
    assert R.rel(w[:, :N].float().T, w[:, :N].float()) > 1.0
