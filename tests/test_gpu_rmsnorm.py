"""rmsnorm_kernel alone, through mt3_op_rmsnorm (include/mt3_hip.h states the rule): the standalone T5 LayerNorm that
writes enc_out, which every cross-attention K/V projection reads.  Against float64:
y = x * rsqrt(mean(x^2) + 1e-6) * scale.

What each check would catch:
  dim 64 / 512 / 768             a lane that reads past a short row (64: only 16 lanes have a float4), the second and the
                                 THIRD trip of the 256-column loop (768 = MT3_BASE) dropped from the sum or from the store
  rows 1 / 3 / 4 / 5 / 130       the block of four rows: a partial last block (1, 3, 5, 130 = 32 * 4 + 2), a store at or
                                 past row `rows` (sentinel rows behind the last row and one in front of the first)
  ct only / f32 only / both      an output written through a NULL pointer's sibling, a result that depends on which
                                 outputs are given (the three launches agree bit for bit)
  bf16 and f32                   the two instantiations; at f32 out_ct IS out_f32, bit for bit
  rows over four decades         1e-6 added outside the root or scaled wrongly, a sum that loses small rows
  a row of zeros                 rsqrt(0 + 1e-6) is finite: the row is exactly 0, not NaN
  scale with both signs          |scale| or a scale index off by a float4

Bounds.  out_f32 may differ from the float64 value by RN = 15 * 2^-24 relative, in units of u = 2^-24 (one rounding to
nearest): the sum of squares is a sum of positive terms, so its relative error is at most one u per rounding on the
longest path to the total -- the square (1), the lane's chain of dim / 256 float4s of four terms (12 at dim 768) and the
six shuffle steps: 19 u, halved by the root: 9.5; the division by dim and the addition of 1e-6: 1 u each, halved: 1;
rsqrtf, one ulp: 2; the two products x * rs * scale: 2.  14.5, rounded up.  out_ct in bf16 is that f32 value rounded to
nearest: half a bf16 ulp at the float64 value (2^(exponent - 8)) plus RN.
MEASURED on MI355X: see MEASURED below.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402

RN = 15 * 2.0 ** -24
SENTINEL = -7.5
GUARD = 4                                                # sentinel rows behind row rows - 1 (and one in front of row 0)
# MEASURED on MI355X, worst over all cases: |out_f32 - y64| / |y64| as a share of RN; bf16 out_ct as a share of its bound
MEASURED = {"out_f32": "0.21 of RN", "out_ct bf16": "1.00 (ties of the rounding reach the half ulp)"}


def rmsnorm(dtype, x, scale, out_ct, out_f32, rows, dim):
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = _lib.load().mt3_op_rmsnorm(dtype, x.data_ptr(), scale.data_ptr(), ptr(out_ct), ptr(out_f32), rows, dim,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(rc)


def same(a, b):
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def half_ulp_bf16(x):
    return torch.exp2(torch.frexp(x.abs().clamp_min(2.0 ** -126))[1].double() - 1 - 8)


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 130])
@pytest.mark.parametrize("dim", [64, 512, 768])
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_rmsnorm(kind, dim, rows):
    what = f"rmsnorm {kind} rows {rows} dim {dim}"
    dtype, ct = (_lib.MT3_BF16, torch.bfloat16) if kind == "bf16" else (_lib.MT3_F32, torch.float32)
    g = torch.Generator().manual_seed(1000 * dim + rows)
    x = torch.randn(rows, dim, generator=g) * torch.pow(10.0, 4 * torch.rand(rows, 1, generator=g) - 2)
    zero_row = (rows - 1) // 2 if rows >= 3 else None
    if zero_row is not None:
        x[zero_row] = 0.0
    scale = torch.randn(dim, generator=g)
    assert bool((scale > 0).any()) and bool((scale < 0).any())
    x, scale = x.cuda(), scale.cuda()
    x0, scale0 = x.clone(), scale.clone()
    y = x.double() * torch.rsqrt((x.double() ** 2).mean(-1, keepdim=True) + 1e-6) * scale.double()

    def buffers(want_ct, want_f32):
        mk = lambda t: torch.full((1 + rows + GUARD, dim), SENTINEL, device="cuda", dtype=t)
        return (mk(ct) if want_ct else None), (mk(torch.float32) if want_f32 else None)

    got = {}
    for outs in ("ct", "f32", "both"):
        b_ct, b_f32 = buffers(outs != "f32", outs != "ct")
        rmsnorm(dtype, x, scale, None if b_ct is None else b_ct[1:], None if b_f32 is None else b_f32[1:], rows, dim)
        for name, buf in (("ct", b_ct), ("f32", b_f32)):
            if buf is None:
                continue
            assert bool((buf[0] == SENTINEL).all()), (what, outs, name, "a store in front of row 0")
            assert bool((buf[1 + rows:] == SENTINEL).all()), (what, outs, name, "a store at or past row `rows`")
            got[(outs, name)] = buf[1:1 + rows]
    assert same(x, x0) and same(scale, scale0), (what, "an input changed")
    # which outputs are given changes no bit
    assert same(got[("ct", "ct")], got[("both", "ct")]), (what, "out_ct depends on out_f32 being given")
    assert same(got[("f32", "f32")], got[("both", "f32")]), (what, "out_f32 depends on out_ct being given")
    o_ct, o_f32 = got[("both", "ct")], got[("both", "f32")]
    assert bool(torch.isfinite(o_f32).all()) and bool(torch.isfinite(o_ct.float()).all()), what
    if zero_row is not None:
        assert bool((o_f32[zero_row] == 0).all()) and bool((o_ct[zero_row] == 0).all()), (what, "the row of zeros")
    err = (o_f32.double() - y).abs()
    share = float((err / (RN * y.abs()).clamp_min(1e-300)).max())
    if kind == "f32":
        assert same(o_ct, o_f32), (what, "at f32 out_ct is out_f32")
        share_ct = share
    else:
        lim = half_ulp_bf16(y) + RN * y.abs()
        e_ct = (o_ct.double() - y).abs()
        share_ct = float((e_ct / lim.clamp_min(1e-300)).max())
        assert bool((e_ct <= lim).all()), (what, "out_ct", share_ct)
    print(f"{what}: out_f32 worst |y - y64| = {share:.3f} of RN |y64| (RN = {RN:.2e}); out_ct {share_ct:.3f} of its bound")
    assert bool((err <= RN * y.abs()).all()), (what, "out_f32", share)
