"""CPU tests of tests/mx8_gemm_ref.py: every script through a plain-torch emulation of the kernel's contract
(model_launch) must be accepted by the checkers, every planted fault must be rejected by the checker named for it, and
the references alone must meet the caps the GPU tests rely on (exact sums, ties, every k of a K step hit)."""
import functools
import zlib

import pytest
import torch

from tests import mx8_gemm_ref as X
from tests import mx8_ref


@functools.lru_cache(maxsize=None)
def case(name, script):
    return X.build_case(X.FORMS[name], script, zlib.crc32(name.encode()) % 10000 + X.SCRIPTS.index(script))


def run(c, M, seq=None, spoil=None, **fault):
    b = X.buffers(c, M, seq)
    before = {k: t.clone() for k, t in b.items()}
    X.model_launch(c, M, b, seq, **fault)
    if spoil:
        spoil(b)
    return X.check(c, M, b, before, seq)


def rows_of(name):
    return (150, 50) if X.FORMS[name].epi == X.EPI_HEADS else (X.LADDER_M if "ladder" in name or "plain" in name else 129, None)


@pytest.mark.parametrize("script", X.SCRIPTS)
@pytest.mark.parametrize("name", list(X.FORMS))
def test_checkers_accept_a_correct_launch(name, script):
    M, seq = rows_of(name)
    figs = run(case(name, script), M, seq)
    print(name, script, figs)
    assert figs["share"] is None or figs["share"] <= 1.0


@pytest.mark.parametrize("name", X.ROW_FORMS)
def test_one_row_launches_are_accepted_and_resid_meets_ties(name):
    figs = run(case(name, "exact"), 1)
    if X.FORMS[name].epi == X.EPI_RESID:
        assert figs["ties"] > 0


@pytest.mark.parametrize("name", list(X.FORMS))
def test_exact_sums_are_exact_in_f32(name):
    c, f = case(name, "exact"), X.FORMS[name]
    assert X.exact_units(f.K) < 2 ** 24
    units = c["acc"] / torch.ldexp(torch.ones(1, dtype=torch.float64), c["r"][:, None] + c["c"][None])
    assert torch.equal(units, units.round()) and float(units.abs().max()) <= 16 * f.K <= 2 ** 15
    # worst partial sum of ANY order: the sum of the magnitudes
    ad, wd = mx8_ref.dequantize(c["aq"], c["asc"]), mx8_ref.dequantize(c["wq"], c["wsc"])
    assert torch.equal(c["acc"], ad @ wd.T)       # the integer route and the product of the dequantised operands agree
    mag = ad.abs() @ wd.abs().T
    assert float((mag / torch.ldexp(torch.ones(1, dtype=torch.float64), c["r"][:, None] + c["c"][None])).max()) <= 16 * f.K
    if f.epi == X.EPI_RESID:
        unit = torch.ldexp(torch.ones(1, dtype=torch.float64), (c["r"][:, None] + c["c"][None]).clamp(max=0))
        assert float(((mag + c["x0"].abs().double()) / unit).max()) <= X.exact_units(f.K)
    d = X.exact_offsets(f.K).view(-1, 4)
    assert all(len(set(step.tolist())) == 4 for step in d) and bool((d[1:] != d[:-1]).all())


@pytest.mark.parametrize("K", sorted({f.K for f in X.FORMS.values()}))
def test_onehot_rows_hit_every_k(K):
    hit = set(X.onehot_k(torch.arange(K), K).tolist())
    steps = K // 128
    for step in {0, steps // 2, steps - 1}:
        assert set(range(128 * step, 128 * step + 128)) <= hit
    assert len(set(X.onehot_k(torch.arange(min(K, 300)), K).tolist())) == min(K, 300)      # the row-count cases: no k twice


def test_onehot_products_are_normal_and_every_code_appears():
    c = case("enc_cross_kv", "onehot")
    assert set(c["wq"].reshape(-1).tolist()) == set(X.CODES.tolist())
    assert torch.equal(c["acc"] + 0.0, mx8_ref.dequantize(c["aq"], c["asc"]) @ mx8_ref.dequantize(c["wq"], c["wsc"]).T + 0.0)
    nz = c["acc"][c["acc"] != 0].abs()
    assert float(nz.min()) >= 2.0 ** -126 and torch.equal(nz.float().to(torch.bfloat16).double(), nz)
    assert bool((c["asc"][:, 0::2] != c["asc"][:, 1::2]).all()) and bool((c["wsc"][:, 0::2] != c["wsc"][:, 1::2]).all())


# ------------------------------------------------------------------------------------------------ the planted faults
@pytest.mark.parametrize("operand", ["a", "w"])
@pytest.mark.parametrize("name", ["plain_store_k256", "enc_wo", "enc_cross_kv", "base_qkv"])
def test_swapped_block_scales_are_caught_by_exact(name, operand):
    c = case(name, "exact")
    M, seq = rows_of(name)
    step = c["form"].K // 128 // 2
    if operand == "a":
        asc = c["asc"][:M].clone()
        asc[:, [4 * step, 4 * step + 1]] = asc[:, [4 * step + 1, 4 * step]]
        with pytest.raises(AssertionError):
            run(c, M, seq, asc=asc)
    else:
        wrong = dict(c)
        wrong["wsc"] = c["wsc"].clone()
        wrong["wsc"][:, [4 * step + 2, 4 * step + 3]] = c["wsc"][:, [4 * step + 3, 4 * step + 2]]
        with pytest.raises(AssertionError):
            run(wrong, M, seq, asc=c["asc"][:M])


@pytest.mark.parametrize("by", [16, 64])
@pytest.mark.parametrize("name", ["enc_qkv", "enc_wo_mlp", "base_cross_kv", "plain_store_k128"])
def test_a_displaced_k_is_caught_by_onehot(name, by):
    c = case(name, "onehot")
    M, seq = rows_of(name)
    k0 = int(X.onehot_k(torch.tensor(M - 1), c["form"].K))
    aq = c["aq"][:M].clone()
    aq[:, [k0, k0 ^ by]] = aq[:, [k0 ^ by, k0]]
    with pytest.raises(AssertionError):
        run(c, M, seq, aq=aq)


@pytest.mark.parametrize("name", ["enc_qkv", "enc_wo", "base_cross_kv", "plain_store_k128"])
def test_the_neighbouring_blocks_scale_is_caught_by_onehot(name):
    c = case(name, "onehot")
    M, seq = rows_of(name)
    asc = c["asc"][:M].view(M, -1, 2).flip(-1).reshape(M, -1)
    with pytest.raises(AssertionError):
        run(c, M, seq, asc=asc)


@pytest.mark.parametrize("name,key", [("enc_qkv", "out"), ("enc_wo", "out"), ("enc_wo", "out_q"), ("enc_wo", "out_sc"),
                                      ("enc_wo", "out_ss"), ("enc_geglu", "out_q"), ("enc_geglu", "out_sc"),
                                      ("enc_cross_kv", "out")])
def test_a_stored_row_behind_m_is_caught_by_the_guards(name, key):
    c = case(name, "random")
    M, seq = rows_of(name)

    def spoil(b):
        if c["form"].epi == X.EPI_HEADS:
            b[key][M * c["form"].N + 3] = 1.0
        else:
            b[key][M + X.GUARD - 1, -1] = 1

    with pytest.raises(AssertionError, match="behind row"):
        run(c, M, seq, spoil=spoil)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_tie_rounded_away_from_even_is_caught(dtype):
    x = X.tie_rows(dtype)
    q, sc = mx8_ref.quantize(x)
    X.check_quantiser(x, q, sc)
    y = X.scaled(x.float(), sc)
    ties = X.tie_mask(y)
    assert int(ties.sum(1).min()) >= 112           # every midpoint of the grid in every row (and the amax never is one)
    v = q.view(torch.float8_e4m3fn).double()
    away = torch.where(ties, v + 2 * (y - v), v).float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert int((away != q).sum()) == int(ties.sum())
    with pytest.raises(AssertionError, match="elements"):
        X.check_quantiser(x, away, sc)
    one = q.clone()
    r, col = [int(t[0]) for t in torch.nonzero(ties, as_tuple=True)]
    one[r, col] = away[r, col]
    with pytest.raises(AssertionError, match="elements"):
        X.check_quantiser(x, one, sc)
    # the neighbours one ulp to either side round to DIFFERENT e4m3 values: they are no ties
    assert int(ties.sum()) * 3 <= x.numel()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_copied_second_scale_byte_is_caught(dtype):
    x = X.position_rows(dtype)
    q, sc = mx8_ref.quantize(x)
    X.check_quantiser(x, q, sc)
    assert bool((sc[:, 0] != sc[:, 1]).all())
    where = x.float().abs().argmax(1)
    assert sorted(where.tolist()) == sorted(list(range(64)) * 2)                # every position, both signs
    assert sorted(x.float()[torch.arange(128), where].tolist()) == [-3072.0] * 64 + [3072.0] * 64
    wrong = sc.clone()
    wrong[:, 1] = sc[:, 0]
    with pytest.raises(AssertionError, match="scale bytes"):
        X.check_quantiser(x, q, wrong)


@pytest.mark.parametrize("script", list(X.QUANT_SCRIPTS))
def test_wrong_sums_of_squares_are_caught_where_they_are_finite(script):
    x = X.QUANT_SCRIPTS[script](torch.float32)
    q, sc = mx8_ref.quantize(x)
    ref = (x.double() ** 2).view(x.shape[0], x.shape[1] // 16, 16).sum(-1)
    ss = ref.float()                                     # inf where the squares overflow: not held against the kernel
    X.check_quantiser(x, q, sc, ss)
    assert bool((ref < 1e38).any()) and (script != "position" or bool((ref < 1e38).all()))
    r, col = [int(v[0]) for v in torch.nonzero((ref < 1e38) & (ref > 1e-30), as_tuple=True)]
    ss[r, col] *= 1 + 4e-6
    with pytest.raises(AssertionError, match="sums of squares"):
        X.check_quantiser(x, q, sc, ss)


def test_range_rows_reach_the_edges_of_the_rule():
    x = X.range_rows(torch.float32)
    q, sc = mx8_ref.quantize(x)
    assert bool(torch.isfinite(x).all())
    assert int(sc.min()) == 0 and int(sc.max()) == 247
    assert sc[2, 1] == 0 and sc[3, 0] == 0 and sc[3, 1] == 0                    # below 2^-120, exactly 2^-120, subnormals
    assert q[3, 0] == e4m3_byte(128.0) and bool((q[3, 32:] != 0).any())         # the rule does not flush f32 subnormals
    assert bool((x[3, 32:] != 0).all()) and float(x[3, 32:].abs().max()) < 2.0 ** -126
    assert bool((q[0, [0, 32]] == e4m3_byte(224.0)).all()) and q[1, 0] == e4m3_byte(224.0)      # 448 2^k: nothing saturates
    assert bool(((q[4, :32] & 0x7F) == 0).all()) and sc[4, 0] == 0             # a zero block: byte 0, zeros


def e4m3_byte(v):
    return int(X.e4m3(torch.tensor([v]))[0])


@pytest.mark.parametrize("script", ["onehot", "exact"])
@pytest.mark.parametrize("K", X.LADDER_K)
@pytest.mark.parametrize("kind", ["store", "geglu"])
def test_a_norm_one_float4_short_is_caught_by_the_ladder(kind, K, script):
    c = case(f"ladder_{kind}_k{K}", script)
    a_ss = c["a_ss"][:X.LADDER_M].clone()
    a_ss[:, -4:] = 0                               # rs from K - 64 columns
    with pytest.raises(AssertionError):
        run(c, X.LADDER_M, a_ss=a_ss)


@pytest.mark.parametrize("script", X.SCRIPTS)
@pytest.mark.parametrize("name", X.HEAD_FORMS + ("heads_normed",))
def test_a_batch_index_per_64_row_pass_is_caught(name, script):
    c = case(name, script)
    run(c, 150, 50)
    with pytest.raises(AssertionError):
        run(c, 150, 50, heads_stride64=True)


def test_rolls_move_the_reference_with_the_operands():
    for name in ("enc_wo", "enc_geglu"):
        c = case(name, "random")
        r = X.rolled_rows(c, 129)
        run(r, 129)
        w = X.rolled_w(c, X.w_roll(c["form"]))
        run(w, 129)
        assert torch.equal(w["acc"], torch.roll(c["acc"], X.w_roll(c["form"]), 1))
