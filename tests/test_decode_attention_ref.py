"""tests/decode_attention_ref.py pinned on cases that can be checked by hand (CPU only): the reference of the GPU tests
in tests/test_gpu_decode_attention_forms.py must itself be right."""
import pytest

torch = pytest.importorskip("torch")
from tests import decode_attention_ref as R  # noqa: E402

H = 2


def _caches(rows, cap, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, H, cap, 64, generator=g).to(dtype), torch.randn(rows, H, cap, 64, generator=g).to(dtype))


def _unit_sums(B, n):
    """partial sums whose mean over 16 n columns is 1 - 1e-6: rs is 1 (to float64 round-off)"""
    return torch.full((B, n), 16.0 * (1.0 - 1e-6), dtype=torch.float64)


def test_unit_row_scale_reduces_to_plain_softmax_attention():
    B, cap = 3, 9
    kc, vc = _caches(B, cap, 0)
    g = torch.Generator().manual_seed(1)
    raw = torch.randn(B, 3, H, 64, generator=g) * 0.5
    step = torch.tensor([0, 4, 8])
    out, K, V, S, rs = R.decode_attention_ref(torch.float32, kc, vc, q_f32=raw[:, 0], q_ss=_unit_sums(B, 8),
                                              new_k=raw[:, 1], new_v=raw[:, 2], step=step)
    assert S is None and torch.allclose(rs, torch.ones(B, dtype=torch.float64), rtol=0, atol=1e-15)
    for b in range(B):
        n = int(step[b]) + 1
        k = torch.cat([kc[b, :, : n - 1], raw[b, 1][:, None]], 1).double()          # by hand: the cache, then the new row
        v = torch.cat([vc[b, :, : n - 1], raw[b, 2][:, None]], 1).double()
        logits = (raw[b, 0].double()[:, None, :] * k).sum(-1)
        p = torch.exp(logits - logits.amax(-1, keepdim=True))
        ref = ((p / p.sum(-1, keepdim=True))[..., None] * v).sum(1)
        assert torch.allclose(out[b], ref, rtol=1e-12, atol=1e-14)
        assert torch.equal(K[b, :, n - 1], raw[b, 1]) and torch.equal(V[b, :, n - 1], raw[b, 2])
        keep = [i for i in range(cap) if i != n - 1]
        assert torch.equal(K[b][:, keep], kc[b][:, keep]) and torch.equal(V[b][:, keep], vc[b][:, keep])
    # the plain form of the same rows is the same launch
    out2, K2, V2, _, _ = R.decode_attention_ref(torch.float32, kc, vc, q=raw[:, 0], new_k=raw[:, 1], new_v=raw[:, 2], step=step)
    assert torch.allclose(out, out2, rtol=1e-12, atol=1e-14) and torch.equal(K, K2) and torch.equal(V, V2)


def test_row_scale_rule_and_rounding():
    # sums 16 n (1/4 - 1e-6): rs = 2 exactly in exact arithmetic; bf16 rounding of raw * rs is round-to-nearest-even
    n = 4
    ss = torch.full((1, n), 16.0 * (0.25 - 1e-6), dtype=torch.float64)
    assert abs(float(R.row_scales(ss)[0]) - 2.0) < 1e-14
    assert float(R.round_ct(torch.tensor(1.00390625), torch.bfloat16)) == 1.0         # 1 + 2^-8: a tie, to even
    assert float(R.round_ct(torch.tensor(1.01171875), torch.bfloat16)) == 1.015625    # 1 + 3 * 2^-8: a tie, to even
    assert float(R.round_ct(torch.tensor(1.0 + 2.0 ** -30), torch.float32)) == 1.0
    kc, vc = _caches(1, 4, 2, torch.bfloat16)
    raw = torch.full((1, H, 64), 0.501953125)                                          # x 2 = 1 + 2^-8 -> 1.0 in bf16
    _, K, V, _, rs = R.decode_attention_ref(torch.bfloat16, kc, vc, q_f32=raw, q_ss=ss, new_k=raw, new_v=raw,
                                            step=torch.tensor([2]))
    assert torch.equal(K[0, :, 2].float(), torch.ones(H, 64)) and torch.equal(V[0, :, 2].float(), torch.ones(H, 64))


def test_single_key_returns_the_v_row():
    B = 2
    kc, vc = _caches(B, 5, 3, torch.bfloat16)
    g = torch.Generator().manual_seed(4)
    raw = torch.randn(B, 3, H, 64, generator=g)
    ss = R.scripted_partial_sums(B, 8, seed=0)
    step = torch.zeros(B, dtype=torch.int64)
    out, K, V, _, rs = R.decode_attention_ref(torch.bfloat16, kc, vc, q_f32=raw[:, 0], q_ss=ss, new_k=raw[:, 1],
                                              new_v=raw[:, 2], step=step)
    assert torch.equal(out, V[:, :, 0].double())
    assert torch.equal(V[:, :, 0], (raw[:, 2].double() * rs[:, None, None]).to(torch.bfloat16))
    # cross form, one key: the cached V row whatever the query
    out, _, _, _, _ = R.decode_attention_ref(torch.bfloat16, kc, vc, q=raw[:, 0].to(torch.bfloat16), n_keys=1)
    assert torch.equal(out, vc[:, :, 0].double())
    # e4m3: the DEQUANTISED stored row
    kb, ks, _ = R._fp8_quant_ref(kc)
    vb, vs, _ = R._fp8_quant_ref(vc)
    sc = torch.stack([ks, vs], -1)
    out, K8, V8, S8, _ = R.decode_attention_ref(torch.bfloat16, kb, vb, kv_scale=sc, q_f32=raw[:, 0], q_ss=ss,
                                                new_k=raw[:, 1], new_v=raw[:, 2], step=step)
    want = R._fp8_quant_ref((raw[:, 2].double() * rs[:, None, None]).to(torch.bfloat16))
    assert torch.equal(V8[:, :, 0], want[0]) and torch.equal(S8[:, :, 0, 1], want[1]) and torch.equal(out, want[2])
    assert torch.equal(K8[:, :, 1:], kb[:, :, 1:]) and torch.equal(S8[:, :, 1:], sc[:, :, 1:])


def test_cache_row_selects_the_row_and_done_slots_are_left_alone():
    rows, cap = 5, 6
    kc, vc = _caches(rows, cap, 5)
    g = torch.Generator().manual_seed(6)
    q = torch.randn(3, 3, H, 64, generator=g)
    cache_row, done = torch.tensor([4, 1, 2]), torch.tensor([0, 1, 0])
    step = torch.tensor([3, -1, 0])                                                  # the done slot's entry is garbage
    out, K, V, _, _ = R.decode_attention_ref(torch.float32, kc, vc, q=q[:, 0], new_k=q[:, 1], new_v=q[:, 2], step=step,
                                             done=done, cache_row=cache_row)
    assert torch.isnan(out[1]).all()
    # slot 0 alone over cache row 4 moved to row 0 of a one-row cache: the same numbers
    o0, K0, _, _, _ = R.decode_attention_ref(torch.float32, kc[4:5], vc[4:5], q=q[:1, 0], new_k=q[:1, 1], new_v=q[:1, 2],
                                             step=step[:1])
    assert torch.equal(out[0], o0[0]) and torch.equal(K[4], K0[0])
    assert torch.equal(out[2], q[2, 2].double())                                     # one key: its own V row
    assert torch.equal(K[2, :, 0], q[2, 1]) and torch.equal(V[2, :, 0], q[2, 2])
    for r in (0, 1, 3):                                                              # unmapped rows and the done slot's row
        assert torch.equal(K[r], kc[r]) and torch.equal(V[r], vc[r])
    # done without a map: the identity
    out, K, _, _, _ = R.decode_attention_ref(torch.float32, kc, vc, q=q[:, 0], new_k=q[:, 1], new_v=q[:, 2], step=step,
                                             done=done)
    assert torch.equal(K[0, :, 3], q[0, 1]) and torch.equal(K[1], kc[1]) and torch.equal(K[4], kc[4])


@pytest.mark.parametrize("n", [4, 32, 48, 64])
def test_scripted_partial_sums_put_a_dominant_group_on_every_float4(n):
    B = 12
    lanes = set()
    for shift in (0, 8):
        ss = R.scripted_partial_sums(B, n, seed=n, shift=shift).double()
        idx = R.dominant_index(B, n, shift)
        assert torch.equal(ss.argmax(-1), idx)
        dom = ss[torch.arange(B), idx]
        rest = ss.sum(-1) - dom
        assert torch.allclose(dom, 15.0 * rest, rtol=1e-6)                           # without it the sum shrinks 16-fold
        others = ss[ss < dom[:, None]]
        assert others.min() >= 1e-4 * (1 - 1e-6) and others.max() <= 1.0
        lanes |= {int(i) // 4 for i in idx}
        if shift == 0 and n <= 32:
            assert lanes == set(range(n // 4))
    assert lanes == set(range(n // 4))                                               # every lane's float4, both DPP half rows
