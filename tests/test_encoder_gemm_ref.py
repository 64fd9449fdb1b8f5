"""tests/encoder_gemm_ref.py on the CPU: the conditions of its two input scripts, and that its checkers NOTICE.  A correct
launch is computed by plain f32 torch from the exact script (encoder_gemm_ref.model_launch); each test below breaks it the
way a kernel bug would and requires the checker to fail; the unbroken launch must pass for every form."""
import zlib

import pytest

torch = pytest.importorskip("torch")
from tests import encoder_gemm_ref as E  # noqa: E402

SMALL = [n for n in E.FORMS if n not in E.TALL]          # the tall forms are the same operands with more rows
M = 300                                                  # three 128-row tiles, the last one ragged
T0, T1 = 128, 256                                        # the corrupted 128 x 128 tile: rows and columns [128, 256)
_cases = {}


def case(name, script="exact"):
    if (name, script) not in _cases:
        _cases[(name, script)] = E.build_case(E.FORMS[name], script, zlib.crc32(name.encode()) % 10000)
    return _cases[(name, script)]


def launch_and_check(name, seq=None, spoil=None, **wrong):
    c = case(name)
    b = E.buffers(c, M)
    before = {k: t.clone() for k, t in b.items()}
    E.model_launch(c, M, b, seq=seq, **wrong)
    if spoil:
        spoil(b)
    return E.check(c, M, b, before, seq=seq)


def must_fail(name, **kw):
    launch_and_check(name, **{k: v for k, v in kw.items() if k == "seq"})          # the unbroken launch passes
    with pytest.raises(AssertionError):
        launch_and_check(name, **kw)


# ------------------------------------------------------------------------------------------ the scripts' own conditions
@pytest.mark.parametrize("name", SMALL)
def test_exact_script_partial_sums_stay_below_2_to_the_24_units(name):
    """build_case asserts it on the accumulator it computes; here also the operands' ranges and exact representability"""
    c, f = case(name), E.FORMS[name]
    assert E.exact_units(f.K) < 2 ** 24 and E.exact_units(2048) == 34816
    A, W = c["A"].double(), c["Wt"].double()
    assert bool((A == A.round()).all()) and float(A.abs().max()) <= 8
    assert bool((2 * W == (2 * W).round()).all()) and float(W.abs().max()) <= 1
    for t in (c["out0"], c["pos"]):
        if t is not None:
            assert bool((2 * t == (2 * t).round()).all()) and float(t.abs().max()) <= 1024
    assert 2 * float(c["acc"].abs().max()) + 2048 <= E.exact_units(f.K)


@pytest.mark.parametrize("K", sorted({f.K for f in E.FORMS.values() if f.norm == 2}))
def test_scripted_dominant_group_visits_every_float4_of_a_tile(K):
    n = K // 16
    ss = E.scripted_partial_sums(256, n, 7)
    idx = E.dominant_index(256, n)
    assert torch.equal(ss.argmax(-1), idx)
    assert float((ss.gather(1, idx[:, None])[:, 0] / (ss.sum(-1) - ss.gather(1, idx[:, None])[:, 0])).min()) > 14
    for tile in (idx[:128], idx[128:]):
        assert set((tile // 4).tolist()) == set(range(K // 64)), "a float4 of the row never holds the dominant group"
        assert set(tile.tolist()) == set(range(n))


@pytest.mark.parametrize("name", SMALL)
def test_error_model_worst_row_is_below_half_the_bound(name):
    """random script: the float64 result rounded to the output type, worst single row, against half of the bound the GPU
    tests assert per row (so the bound leaves the kernel as much again for its accumulation order)"""
    c = case(name, "random")
    worst = E.model_worst_row(c, E.FORMS[name].rows)
    print(f"{name}: error model worst row {worst:.3e}, bound {E.FORMS[name].bound:.0e}")
    assert worst < 0.5 * E.FORMS[name].bound


def test_gelu_fast_error_term():
    """G of the GEGLU interval, from the f32 evaluation of gelu_tanh_fast's formula on the CPU: printed for the record
    (the module docstring quotes it), and small against the bf16 half ulp it sits beside"""
    for name in ("enc_geglu", "base_geglu", "single_geglu", "mfma_geglu", "split_geglu_f32"):
        print(f"{name}: G = {case(name)['G']:.3e}")
        assert 0 < case(name)["G"] < 4 * 2.0 ** -23


# ------------------------------------------------------------------------------------------ correct launches must pass
@pytest.mark.parametrize("script", ["exact", "random"])
@pytest.mark.parametrize("name", SMALL)
def test_a_correct_launch_passes(name, script):
    c = case(name, script)
    b = E.buffers(c, M)
    before = {k: t.clone() for k, t in b.items()}
    E.model_launch(c, M, b)
    figs = E.check(c, M, b, before)
    print(name, script, figs)


def test_a_correct_heads_launch_with_segments_passes():
    launch_and_check("enc_cross_kv", seq=100)


def test_rolled_case_is_the_same_launch_on_rolled_rows():
    for name in ("enc_qkv", "enc_wo", "enc_in", "enc_cross_kv"):
        c = E.rolled(case(name), M)
        b = E.buffers(c, M)
        before = {k: t.clone() for k, t in b.items()}
        E.model_launch(c, M, b)
        E.check(c, M, b, before)


# ---------------------------------------------------------------------------------------------- wrong launches must not
@pytest.mark.parametrize("name", ["enc_wo", "enc_qkv", "score_logits", "enc_geglu", "enc_in", "ring_store_k64"])
@pytest.mark.parametrize("times", [-1, 1], ids=["left_out", "counted_twice"])
def test_a_k_slice_left_out_or_counted_twice_in_one_tile(name, times):
    c = case(name)
    k0 = c["form"].K - 32
    acc = c["acc"][:M].clone()
    cols = slice(0, 128) if c["form"].N == 128 else slice(T0, T1)
    a = (c["A"].to(c["form"].ct) if c["form"].a_f32 else c["A"]).double()
    acc[T0:T1, cols] += times * (a[T0:T1, k0:k0 + 32] @ c["Wt"].double()[cols, k0:k0 + 32].T)
    must_fail(name, acc=acc)


@pytest.mark.parametrize("name", ["enc_wo", "enc_qkv", "score_logits", "enc_geglu", "mfma_cross_kv"])
def test_two_row_fragments_of_one_tile_swapped(name):
    acc = case(name)["acc"][:M].clone()
    acc[T0 + 16:T0 + 32, T0:T1], acc[T0 + 32:T0 + 48, T0:T1] = (case(name)["acc"][T0 + 32:T0 + 48, T0:T1],
                                                                case(name)["acc"][T0 + 16:T0 + 32, T0:T1])
    must_fail(name, acc=acc)


@pytest.mark.parametrize("name", ["enc_qkv", "score_logits", "enc_geglu", "base_qkv", "wide_qkv", "k576"])
def test_one_float4_of_partial_sums_dropped_from_one_row(name):
    """the float4 that holds the row's dominant group (a kernel that drops float4 u drops it for every row: the rows
    whose dominant group sits there are the ones that show it)"""
    c = case(name)
    ss = c["a_ss"][:M].clone()
    u = int(E.dominant_index(M, c["form"].K // 16)[200]) // 4
    ss[200, 4 * u:4 * u + 4] = 0
    must_fail(name, a_ss=ss)


@pytest.mark.parametrize("name", ["enc_qkv", "score_logits", "base_qkv"])
@pytest.mark.parametrize("u", [0, 3, 7])
def test_one_float4_index_dropped_in_every_row(name, u):
    ss = case(name)["a_ss"][:M].clone()
    ss[:, 4 * u:4 * u + 4] = 0
    must_fail(name, a_ss=ss)


@pytest.mark.parametrize("name", ["enc_qkv", "score_logits", "enc_geglu"])
def test_partial_sums_of_row_r_taken_from_row_r_plus_1(name):
    ss = case(name)["a_ss"][:M].clone()
    ss[131] = case(name)["a_ss"][132]
    must_fail(name, a_ss=ss)


@pytest.mark.parametrize("name", ["enc_qkv", "enc_wo", "enc_geglu", "enc_cross_kv", "enc_in"])
def test_one_element_written_in_the_guard_row(name):
    def spoil(b):
        for t in b.values():
            t.view(-1)[M * (t.numel() // (M + E.GUARD)) + 5] = 1.0
    must_fail(name, spoil=spoil)


def test_guard_of_every_by_product_is_watched():
    for k in ("out_ss", "out_ct"):
        def spoil(b, k=k):
            b[k][M, 3] = 1.0
        must_fail("enc_wo", spoil=spoil)


def test_one_heads_row_stored_at_t_plus_1():
    c = case("enc_cross_kv")
    N, seq = c["form"].N, 100

    def spoil(b):
        h = b["out"][:M * N].view(2, M // seq, N // 128, seq, 64)
        row = h[:, 1, :, 41].clone()
        h[:, 1, :, 41] = 7777.0          # what the buffer held
        h[:, 1, :, 42] = row
    must_fail("enc_cross_kv", seq=seq, spoil=spoil)


def test_resid_second_pass_added_to_the_first_passes_residual_rows():
    c = case("enc_wo")
    out0 = c["out0"][:M].clone()
    out0[T0 + 64:T1, T0:T1] = c["out0"][T0:T0 + 64, T0:T1]
    must_fail("enc_wo", out0=out0)


def test_out_ct_that_is_not_the_rounding_of_the_rows():
    def spoil(b):
        b["out_ct"][17, 40] = b["out_ct"][17, 41]
    must_fail("enc_wo", spoil=spoil)
