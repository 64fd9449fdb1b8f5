"""The encoder self-attention kernels in every form launch_encoder_attention and launch_encoder_attention_x6 select,
through mt3_op_encoder_attention and mt3_op_encoder_attention_x6, on the scripted cases of tests/encoder_attention_ref.py
(its docstring says what each case catches) against that module's float64 reference.

Which test launches which instantiation (B x T x H as in the test id; `random` runs B in {1, 3} x H in {1, 6, 12}, every
other case (B, H) = (3, 6) and (1, 12): the smallest launches in which b, h, the query quarter and the key part all take
more than one value):

  enc_attn_kernel<bf16, 256, 8>            test_case[bf16-*-256-*],  test_placement[bf16-256-*]
  enc_attn_kernel<bf16, 512>               test_case[bf16-*-512-*],  test_placement[bf16-512-*]
  enc_attn_kernel<float, 256>              test_case[f32-*-256-*],   test_placement[f32-256-*]
  enc_attn_split_kernel<float, 512, 2, 4>  test_case[f32-*-512-*],   test_placement[f32-512-*]
  enc_attn_x6_kernel<256, 2, 8>            test_case[x6-*-256-*],    test_placement[x6-256-*]
  enc_attn_x6_kernel<512, 4, 8>            test_case[x6-*-512-*],    test_placement[x6-512-*]

What every test_case checks:
  against float64, whole and per row   the whole tensor's rel-L2 and every query row of every head (64 columns, relative
                                       to that row's norm): one wrong row in 2 x 512 x 6 is 1.3e-2 of a whole-tensor norm
                                       even as pure noise, a wrongly rescaled one far less
  sentinels                            four rows of -7.5 in the output's type in front of `out` and behind it keep their
                                       bits (the bf16 store writes dwords at column fr - odd: an off-by-one lands on a
                                       neighbour, in the first and last row on a sentinel)
  inputs untouched                     qkv is bit-equal to a copy taken before the launch
  one_hot                              out[i] is V[pi(i)] to ONE unit in the last place of the output type: the weight of
                                       every other key is below 2^-40 and l rounds to 1 in f32, so 1 / l adds nothing
test_placement: head (b, h) = (2, 5) of the B = 3, H = 6 launch, resp. (0, 11) of (1, 12), against the same head's Q, K and
V in a contiguous B = 1, H = 1 launch, bit for bit: neither H nor B enters a head's arithmetic, only its addressing.

Bounds.  bf16: whole tensor 1e-2 (test_encoder_attention); per row 1e-2 times the factor by which the worst row of the
bf16 error model exceeds that model's whole-tensor error on the same inputs -- computed, not measured, printed by every
test (1.0 - 2.6).  f32 instruction and three planes alike (encoder_attention_ref.x6_bounds): the smaller of 3e-5 and half
the smallest error among the three five-product emulations on the case's inputs, whole tensor and worst row each; about
2.5e-6 / 9e-6 on random, 1.2e-6 / 1.6e-6 to 1.8e-6 on rising and falling (whose logits stay inside +-4.5: at twice
that amplitude the f32 instruction's own accumulation of a logit, ulp(8) = 9.5e-7 per probability, measured 1.96e-6 in its
worst row against 1.77e-6).  one_hot, uniform and large cannot tell five products
from six (the reference module says why) and keep 3e-5.  Every test asserts, from the inputs alone, that the six-product
emulation is under a quarter of its bounds.
MEASURED on MI355X: see MEASURED below (worst over the cases of each kind: whole tensor, worst row as a share of its
bound).
"""
import functools

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import encoder_attention_ref as R  # noqa: E402

KINDS = ("bf16", "f32", "x6")
SENTINEL = -7.5
GUARD = 4                                                # sentinel rows in front of `out` and behind it
# MEASURED on MI355X, worst over all cases of this file: whole-tensor rel-L2 (the case), largest row error / row bound
MEASURED = {"bf16": "2.25e-3 (rising 3 x 512 x 6, bound 1e-2), 0.23 (falling 1 x 256 x 12: 3.27e-3 of 1.45e-2)",
            "f32": "3.6e-6 (uniform 1 x 512 x 12, bound 3e-5; 8.3e-7 on random and rising), 0.64 (rising 1 x 512 x 12: 1.00e-6 of 1.56e-6)",
            "x6": "5.2e-7 (random 1 x 512 x 1, bound 2.5e-6), 0.53 (rising 1 x 512 x 12: 8.3e-7 of 1.56e-6)"}
# one_hot: bf16 and f32 give V[pi(i)] bit for bit; x6 within one unit in the last place (reached: hi + mid + lo is summed in
# f32, smallest first).  placement: 0 elements differ in every launch.
CASE_IDS = [("random", *g) for g in R.GEOMETRIES] + [(n, *g) for n in R.CASES[1:] for g in R.SCRIPTED_GEOMETRIES]


def ct_of(kind):
    return torch.bfloat16 if kind == "bf16" else torch.float32


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b):
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def launch(kind, qkv, out, B, T, H):
    s = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    if kind == "x6":
        rc = lib.mt3_op_encoder_attention_x6(qkv.data_ptr(), out.data_ptr(), B, T, H, s)
    else:
        rc = lib.mt3_op_encoder_attention(_lib.MT3_BF16 if kind == "bf16" else _lib.MT3_F32, qkv.data_ptr(), out.data_ptr(),
                                          B, T, H, s)
    torch.cuda.synchronize()
    _lib.check(rc)


def run(kind, qkv):
    """qkv [B][T][3][H][64] in the kind's type -> out [B][T][H][64]; sentinels and input bits checked"""
    B, T, _, H, _ = qkv.shape
    qkv = qkv.contiguous()
    before = qkv.clone()
    full = torch.full((B * T + 2 * GUARD, H * 64), SENTINEL, device="cuda", dtype=qkv.dtype)
    out = full[GUARD:GUARD + B * T]
    launch(kind, qkv, out, B, T, H)
    assert same(qkv, before), "the launch wrote to qkv"
    assert bool((full[:GUARD] == SENTINEL).all()), "a store in front of out"
    assert bool((full[GUARD + B * T:] == SENTINEL).all()), "a store behind out"
    return out.view(B, T, H, 64)


@functools.lru_cache(maxsize=2)
def prepared(name, B, T, H, bf16):
    """the case on the GPU in the kernel's input type, its float64 reference, and the bounds: (qkv, ref, whole, row, note)"""
    qkv = R.make_case(name, B, T, H).cuda()
    if bf16:
        qkv = qkv.bfloat16()
        q, k, v = R.split_qkv(qkv)
        ref = R.attention_ref(q, k, v)
        factor, m_whole, m_row = R.bf16_row_factor(q, k, v, ref)
        note = f"error model worst row / whole = {m_row:.3e} / {m_whole:.3e} -> factor {factor:.2f}"
        return qkv, ref, R.BF16_TOL, R.BF16_TOL * factor, note
    ref = R.attention_ref(*R.split_qkv(qkv))
    b = R.x6_bounds(qkv, ref)
    # from the inputs alone: the case is what the reference module says it is, and six products fit with room
    assert b["distinguishes"] == (name not in R.CANNOT_TELL_FIVE_FROM_SIX), (name, b)
    assert b["six"][0] < b["whole"] / 4 and b["six"][1] < b["row"] / 4, (name, b)
    note = (f"six products {b['six'][0]:.2e} / {b['six'][1]:.2e}, half the smallest five-product error "
            f"{b['half_five'][0]:.2e} / {b['half_five'][1]:.2e}")
    return qkv, ref, b["whole"], b["row"], note


def ulp(kind, x):
    """the spacing of the output type's values at |x|: 24 significant bits for f32, 8 for bf16"""
    e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))[1].double() - 1
    return torch.exp2(e - (7 if kind == "bf16" else 23))


@pytest.mark.parametrize("kind,name,B,T,H", [(kind, *c) for c in CASE_IDS for kind in KINDS])   # a case's kinds in a row
def test_case(kind, name, B, T, H):
    qkv, ref, tol_whole, tol_row, note = prepared(name, B, T, H, kind == "bf16")
    what = f"encoder attention {kind} {name} B {B} T {T} H {H}"
    out = run(kind, qkv)
    assert bool(torch.isfinite(out.float()).all()), what
    whole, rows = R.rel(out, ref), R.row_rel(out, ref)
    worst = float(rows.max())
    print(f"{what}: rel-L2 {whole:.3e} (bound {tol_whole:.2e}), worst row {worst:.3e} (bound {tol_row:.2e}) = "
          f"{worst / tol_row:.2f} of it; {note}")
    assert whole < tol_whole, (what, whole, tol_whole)
    assert worst < tol_row, (what, worst, tol_row, [int(i) for i in torch.nonzero(rows >= tol_row)[0]])
    if name == "one_hot":
        want = R.split_qkv(qkv)[2][:, R.permutation(T).cuda()].double()
        off = ((out.double() - want).abs() / ulp(kind, want)).max()
        print(f"{what}: out[i] against V[pi(i)]: at most {float(off):.2f} units in the last place")
        assert float(off) <= 1.0, (what, float(off))


@pytest.mark.parametrize("B,H,b,h", [(3, 6, 2, 5), (1, 12, 0, 11)])
@pytest.mark.parametrize("T", [256, 512])
@pytest.mark.parametrize("kind", KINDS)
def test_placement(kind, T, B, H, b, h):
    for name in ("random", "rising"):
        qkv = R.make_case(name, B, T, H).cuda().to(ct_of(kind))
        big = run(kind, qkv)[b, :, h]
        alone = run(kind, qkv[b:b + 1, :, :, h:h + 1].contiguous())[0, :, 0]
        diff = int((bits(big.contiguous()) != bits(alone.contiguous())).sum())
        print(f"placement {kind} {name} T {T}: head ({b}, {h}) of B {B} H {H} against the head alone: {diff} elements differ")
        assert diff == 0, (kind, name, T, diff)
