"""tests/encoder_attention_ref.py on the CPU: the reference against a second formulation (torch.softmax), the plane split
against the host rule, the properties each scripted case is built for (running-maximum counts, the one_hot margin, the
known shifts of uniform, the exact logits of large), and the bounds: on every case the six-product emulation is under a
quarter of its bound and each five-product emulation above it, or the case is one of CANNOT_TELL_FIVE_FROM_SIX."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import encoder_attention_ref as R
from tests.test_three_plane_arithmetic import split3

SCRIPTED = [(3, 256, 6), (1, 512, 12)]                   # (B, T, H): both (B, H) pairs and both T of the GPU file
RANDOM = [(1, 256, 1), (3, 256, 6), (1, 512, 12)]
GEO = {name: (RANDOM if name == "random" else SCRIPTED) for name in R.CASES}
ALL = [(name, *g) for name in R.CASES for g in GEO[name]]


@functools.lru_cache(maxsize=None)
def case(name, B, T, H):
    qkv = R.make_case(name, B, T, H)
    return qkv, R.attention_ref(*R.split_qkv(qkv))


def test_reference_is_softmax_attention_and_the_models_without_rounding_are_the_reference():
    qkv, ref = case("random", 3, 256, 6)
    q, k, v = (t.double() for t in R.split_qkv(qkv))
    w = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k), -1)
    dense = torch.einsum("bhqk,bkhd->bqhd", w, v)
    assert float((ref - dense).abs().max()) < 1e-13
    assert torch.equal(R.attention_ref(q, k, v, p_dtype=None, out_dtype=None), ref)
    # every f32 input IS the sum of nine plane products up to 2^-26: all nine give the reference to 1e-7
    nine = [(i, j) for i in range(3) for j in range(3)]
    s = R._plane_product("nkd,nqd->nqk", R.planes(R._heads(k)[:2]), R.planes(R._heads(q)[:2]), nine)
    exact = torch.einsum("nqd,nkd->nqk", R._heads(q)[:2], R._heads(k)[:2])
    assert float((s - exact).abs().max()) < 64 * 5 * 5 * 2.0 ** -25
    assert sorted(R.SIX) == sorted(set(nine) - {(1, 2), (2, 1), (2, 2)}) and set(R.DROPS.values()) < set(R.SIX)


def test_planes_are_the_host_split():
    x = R.make_case("random", 1, 256, 1).flatten()
    x = torch.cat([x, x * 1e-20, x * 1e20, torch.tensor([0.0, -0.0, 1 + 2.0 ** -17, 16 - 2.0 ** -20])])
    for got, want in zip(R.planes(x), split3(x.numpy())[:3]):
        assert np.array_equal(got.numpy(), want.astype(np.float64))


@pytest.mark.parametrize("name", ["rising", "falling"])
@pytest.mark.parametrize("B,T,H", SCRIPTED)
def test_running_maximum_moves_in_one_query_and_stays_in_its_neighbour(name, B, T, H):
    qkv, _ = case(name, B, T, H)
    q, k, _ = R.split_qkv(qkv)
    moves = R.running_max_moves(R.logits(q, k))                        # [B * H][T][T / 64 - 1]
    every, never = moves.all(-1), ~moves.any(-1)
    print(f"{name} B {B} T {T} H {H}: the running maximum changes at every chunk boundary in {float(every.double().mean()):.3f} "
          f"of the queries, never after the first chunk in {float(never.double().mean()):.3f}")
    assert float(every.double().mean()) >= 0.25 and float(never.double().mean()) >= 0.25
    tiles_e, tiles_n = every.view(B * H, T // 16, 16), never.view(B * H, T // 16, 16)
    assert bool(tiles_e.any(-1).all()) and bool(tiles_n.any(-1).all())  # both kinds inside every 16-query tile
    # and they are neighbours: the kind alternates with the query's parity
    assert float((every[:, 0::2] | every[:, 1::2]).double().mean()) >= 0.9
    assert not bool((every[:, 0::2] & every[:, 1::2]).any())


@pytest.mark.parametrize("T", [256, 512])
def test_permutation_separates_neighbouring_queries(T):
    pi = R.permutation(T)
    assert sorted(pi.tolist()) == list(range(T))
    nxt = torch.roll(pi, -1)
    for part in (64, 128, T // 2):                                     # the 64-key chunks, and every staged part size
        assert bool((pi // part != nxt // part).all()), part
    # a 16-query tile reaches every 64-key chunk of T = 256, and at least half of them at T = 512
    chunks = (pi.view(T // 16, 16) // 64)
    assert all(len(set(row.tolist())) >= 4 for row in chunks)


@pytest.mark.parametrize("B,T,H", SCRIPTED)
def test_one_hot_margin_and_expected_rows(B, T, H):
    qkv, ref = case("one_hot", B, T, H)
    q, k, v = R.split_qkv(qkv)
    s = R.logits(q, k)
    pi = R.permutation(T)
    top = s[:, torch.arange(T), pi]
    assert bool((top == R.ONE_HOT_LOGIT).all())
    others = s.clone()
    others[:, torch.arange(T), pi] = -math.inf
    margin = float((top - others.amax(-1)).min())
    weight = float(torch.softmax(s, -1).masked_fill(torch.isinf(others), 0).amax())
    print(f"one_hot B {B} T {T} H {H}: smallest margin {margin:.1f}, largest weight of another key 2^{math.log2(weight):.1f}")
    assert margin > 40 * math.log(2) and weight < 2.0 ** -40
    want = v[:, pi].double()
    assert float(((ref - want).abs() / want.abs().clamp_min(1e-30)).max()) < 2.0 ** -30   # far inside one f32 ulp
    assert torch.equal(q.bfloat16().float(), q) and torch.equal(k.bfloat16().float(), k)  # the same case at bf16


@pytest.mark.parametrize("B,T,H", SCRIPTED)
def test_uniform_rows_are_the_mean_and_a_lost_key_moves_them_by_a_known_amount(B, T, H):
    qkv, ref = case("uniform", B, T, H)
    v = R.split_qkv(qkv)[2].double()
    mean = v.mean(1, keepdim=True)
    assert float((ref - mean).abs().max()) < 1e-14
    # key k dropped: (sum - v_k) / (T - 1) - mean = (mean - v_k) / (T - 1); doubled: (v_k - mean) / (T + 1)
    k0 = 37
    dropped = (v.sum(1, keepdim=True) - v[:, k0:k0 + 1]) / (T - 1)
    assert float((dropped - mean - (mean - v[:, k0:k0 + 1]) / (T - 1)).abs().max()) < 1e-15
    shift = (mean - v).norm(dim=-1) / (T + 1) / mean.norm(dim=-1)       # [B][T keys][H]: the row error a lost or doubled key leaves
    print(f"uniform B {B} T {T} H {H}: a lost key moves a row by {float(shift.min()):.2e} .. {float(shift.max()):.2e} of its norm")
    assert float(shift.min()) > R.F32_TOL                              # every single key shows at f32
    assert float((shift > 2 * R.BF16_TOL).double().mean()) > 0.3       # and a third of them even at bf16


@pytest.mark.parametrize("B,T,H", SCRIPTED)
def test_large_logits_are_exact_wide_and_in_half_the_heads_far_below_zero(B, T, H):
    qkv, ref = case("large", B, T, H)
    q, k, v = R.split_qkv(qkv)
    s = R.logits(q, k).view(B, H, T, T)
    assert torch.isfinite(ref).all()
    plain, shifted = s[:, 0::2], s[:, 1::2]
    print(f"large B {B} T {T} H {H}: logit sd {float(plain.std()):.1f} / {float(shifted.std()):.1f}, shifted heads' largest "
          f"logit {float(shifted.max()):.1f}, plain heads' range {float(plain.min()):.1f} .. {float(plain.max()):.1f}")
    assert 25 < float(plain.std()) < 35 and 25 < float(shifted.std()) < 35
    assert float(shifted.max()) < -200
    # exact: multiples of 1/16 below 2^24 / 16 in magnitude (every partial sum in any order is such a number), and the
    # inputs are bf16 values, so the bf16 kernels run the same case
    assert bool((s * 16 == torch.round(s * 16)).all()) and float(s.abs().max()) * 16 < 2 ** 24
    assert float((q.double().abs().amax(-1) * k.double().abs().amax(-1).amax()).max()) * 64 * 16 < 2 ** 24
    assert torch.equal(qkv.bfloat16().float(), qkv)


@pytest.mark.parametrize("name,B,T,H", ALL)
def test_six_products_pass_and_five_fail_or_the_case_is_named(name, B, T, H):
    qkv, ref = case(name, B, T, H)
    b = R.x6_bounds(qkv, ref)
    five = ", ".join(f"{n} {e[0]:.2e} / {e[1]:.2e}" for n, e in b["five"].items())
    print(f"{name} B {B} T {T} H {H}: bounds {b['whole']:.2e} whole, {b['row']:.2e} row; six products {b['six'][0]:.2e} / "
          f"{b['six'][1]:.2e}; without {five}")
    assert b["distinguishes"] == (name not in R.CANNOT_TELL_FIVE_FROM_SIX), b
    assert b["whole"] <= R.F32_TOL and b["row"] <= R.F32_TOL           # never looser than today's figure
    assert b["six"][0] < b["whole"] / 4 and b["six"][1] < b["row"] / 4
    if b["distinguishes"]:
        for n, (whole, row) in b["five"].items():
            assert whole >= 2 * b["whole"] and row >= 2 * b["row"], (n, whole, row)
    if name == "random" and T == 256:
        assert 2e-6 < b["half_five"][0] < 3e-6, b["half_five"]        # about 2.5e-6 on the old test's inputs


@pytest.mark.parametrize("name,B,T,H", ALL)
def test_bf16_model_leaves_room_under_the_bound(name, B, T, H):
    qkv = case(name, B, T, H)[0].bfloat16()
    factor, whole, row = R.bf16_row_factor(*R.split_qkv(qkv))
    print(f"{name} B {B} T {T} H {H}: bf16 error model {whole:.2e} whole, {row:.2e} worst row: row bound "
          f"{R.BF16_TOL * factor:.2e} (factor {factor:.2f})")
    assert 1.0 <= factor < 4.0 and whole < R.BF16_TOL / 2 and row < R.BF16_TOL * factor / 2
