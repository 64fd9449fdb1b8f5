"""score_attn_kernel alone (mt3_op_score_attention, include/mt3_hip.h) in the two stride forms score_impl launches --
causal self-attention on [rows][3][H][64] qkv rows with key targets, cross-attention on a [2][Bc][H][T][64] cache --
against the float64 reference of tests/score_prefill_ref.py.  B = 3 segments, H = 3 heads; every self-form launch carries
three different key-target rows, one of them with a 0 at position 0.

What each check would catch:
  reference, whole tensor and per row   a key wrongly visible or hidden (diagonal off by one, a target test other than
                                        != 0, the segment's target row taken from another segment), a masked chunk that
                                        enters the running maximum or sum, wrong head / batch strides
  zero rows                             a query without a visible key that divides by l = 0 or keeps stale accumulators
  NaN / Inf in target-0 K and V rows    a masked row that is loaded and multiplied by a zero probability (NaN), or whose
                                        score enters the maximum
  causal leak (p = 100)                 any dependence of query i on a key j > i, however small: bit-identity
  placement                             a segment's result depending on the launch it sits in (b-indexed addressing)
  sentinels                             a store outside the B * Lq out rows

Bounds: whole-tensor rel-L2 under the figures tests/test_gpu_kernels.py states for the encoder attention, which uses the
same MFMA arrangement (1e-2 bf16: P rounded to bf16 before P V and a bf16 output; 3e-5 f32), and every (segment, query,
head) row under that figure times the factor by which the worst row exceeds the whole tensor in the error model of the
same inputs (score_prefill_ref: P and the output rounded to the compute type) -- computed, not measured.
MEASURED on MI355X over all cases of this file (every case prints its own): see MEASURED below.  The bf16 rows sit ON
the error model (worst row 3.15e-3 measured and modelled: the rounding of P and of the output is the whole error); the
f32 rows are 50 - 70 times above the model's 4.5e-8 (it leaves out the f32 accumulation and expf) and 15 times under
their bound.  No NaN / Inf, leak, placement or sentinel check found a difference.
"""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import score_prefill_ref as R  # noqa: E402

H, HD, B = 3, 3 * 64, 3
GUARD = 4                                                   # sentinel rows in front of and behind the out rows
SENTINEL = -7.5
TOL = {"bf16": 1e-2, "f32": 3e-5}                           # tests/test_gpu_kernels.py: test_encoder_attention
# worst whole-tensor rel-L2, worst row rel-L2 (smallest per-row bound it was held to)
MEASURED = {"bf16": "1.77e-3, 3.15e-3 (1.52e-2)", "f32": "6.7e-7, 3.1e-6 (4.7e-5)"}
GROUPS = [("all", "tail70", "first0"), ("seam", "chunk1", "first0"), ("first0", "none", "tail70")]


def ct_of(kind):
    return torch.float32 if kind == "f32" else torch.bfloat16


def dt_of(kind):
    return _lib.MT3_F32 if kind == "f32" else _lib.MT3_BF16


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def key_targets(name, Lq, seed):
    """[Lq] int32: non-zero ids with the scripted zeros of `name` (positions past Lq do not exist)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, 1500, (Lq,), generator=g, dtype=torch.int32)
    zeros = {"all": [], "tail70": range(70, Lq), "first0": [0], "seam": [63, 64, 65], "chunk1": range(64, 128),
             "none": range(Lq)}[name]
    for j in zeros:
        if j < Lq:
            t[j] = 0
    return t


def launch(kind, **f):
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    ptrs = ("q", "k", "v", "key_tgt", "out")
    v = _lib.ScoreAttnView(**{k: (ptr(x) if k in ptrs else int(x)) for k, x in f.items()})
    rc = _lib.load().mt3_op_score_attention(dt_of(kind), C.byref(v), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(rc)


def guarded_out(kind, rows):
    full = torch.full((rows + 2 * GUARD, HD), SENTINEL, device="cuda", dtype=ct_of(kind))
    return full, full[GUARD:GUARD + rows]


def guards_intact(full, rows):
    return bool((full[:GUARD] == SENTINEL).all()) and bool((full[GUARD + rows:] == SENTINEL).all())


def run_self(kind, qkv, tgt, Lq, seg=None):
    """the launch of score_impl over all B segments, or over segment `seg` alone (B = 1); -> out [n][Lq][H][64]"""
    n, b0 = (B, 0) if seg is None else (1, seg)
    es = qkv.element_size()
    full, out = guarded_out(kind, n * Lq)
    base = qkv.data_ptr() + b0 * Lq * 3 * HD * es
    launch(kind, q=base, q_stride=3 * HD, k=base + HD * es, v=base + 2 * HD * es, kv_stride=3 * HD, kv_bstride=Lq * 3 * HD,
           kv_hstride=64, key_tgt=tgt.data_ptr() + b0 * Lq * 4, out=out, out_stride=HD, B=n, H=H, Lq=Lq, n_keys=Lq, causal=1)
    assert guards_intact(full, n * Lq), "a store outside the out rows"
    return out.clone().view(n, Lq, H, 64)


def check(kind, what, out, ref, model, worst):
    """whole tensor and every (segment, query, head) row against the reference; rows the reference has as zeros are 0"""
    assert torch.isfinite(out.float()).all(), what
    o, r, m = (t.reshape(-1, 64).double().cpu() for t in (out, ref, model))
    empty = r.abs().amax(-1) == 0
    assert bool((o[empty] == 0).all()), (what, "a query without a visible key must write zeros")
    if bool(empty.all()):
        print(f"{what}: every row is exactly 0")
        return
    o, r, m = o[~empty], r[~empty], m[~empty]
    row_err = lambda x: (x - r).norm(dim=-1) / r.norm(dim=-1)
    whole, rows = rel(o, r), float(row_err(o).max())
    m_whole, m_rows = rel(m, r), float(row_err(m).max())
    factor = max(1.0, m_rows / max(m_whole, 1e-300))
    print(f"{what}: rel-L2 {whole:.3e} (bound {TOL[kind]:.0e}), worst row {rows:.3e} (bound {TOL[kind] * factor:.3e}: "
          f"error model worst row / whole = {m_rows:.3e} / {m_whole:.3e} = {factor:.2f})")
    worst.append((whole, rows, TOL[kind] * factor))
    assert whole < TOL[kind], (what, whole)
    assert rows < TOL[kind] * factor, (what, rows, factor)


def self_inputs(kind, Lq, group, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * Lq, 3, H, 64, generator=g)
    qkv[:, 0] *= 0.35                                       # unscaled logits: keep the softmax non-degenerate
    qkv = qkv.to(ct_of(kind)).cuda()
    tgt = torch.stack([key_targets(n, Lq, seed + i) for i, n in enumerate(group)]).cuda()
    return qkv, tgt


@pytest.mark.parametrize("group", GROUPS, ids=["-".join(g) for g in GROUPS])
@pytest.mark.parametrize("Lq", [64, 192])
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_self_form(kind, Lq, group):
    what = f"self {kind} Lq {Lq} masks {'/'.join(group)}"
    qkv, tgt = self_inputs(kind, Lq, group, seed=Lq + len(group[0]))
    out = run_self(kind, qkv, tgt, Lq)
    # the reference over the same (already rounded) values
    x = qkv.view(B, Lq, 3, H, 64)
    ref = R.prefill_attention_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], True, tgt)
    model = R.prefill_attention_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], True, tgt, p_dtype=ct_of(kind), out_dtype=ct_of(kind))
    worst = []
    check(kind, what, out, ref, model, worst)
    for b, name in enumerate(group):
        if name == "first0":                                # query 0 sees nothing; query 1 sees key 1 alone: its V row
            assert bool((out[b, 0] == 0).all()), what
            assert same(out[b, 1], x[b, 1, 2]), (what, "one visible key: out is its V row")
        if name == "none":
            assert bool((out[b] == 0).all()), what
        if name == "all":                                   # query 0 sees key 0 alone
            assert same(out[b, 0], x[b, 0, 2]), what
    # K and V rows of target-0 keys hold NaN / Inf patterns: same bits, all finite
    hidden = (tgt == 0).view(B * Lq)
    for kpat, vpat in ((float("nan"), float("inf")), (float("-inf"), float("nan"))):
        bad = qkv.clone()
        bad[hidden, 1] = kpat
        bad[hidden, 2] = vpat
        got = run_self(kind, bad, tgt, Lq)
        assert torch.isfinite(got.float()).all(), (what, kpat, vpat)
        assert same(got, out), (what, "poisoned target-0 rows changed the result", kpat, vpat)
    # placement: each segment alone
    for b in range(B):
        assert same(run_self(kind, qkv, tgt, Lq, seg=b)[0], out[b]), (what, "segment alone differs", b)


@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_self_form_has_no_causal_leak(kind):
    """K and V rows of every position > 100 replaced: the outputs of queries <= 100 keep their bits (a later key has
    probability exactly 0 and a finite V row, so even the diagonal chunk's products with it add +0)"""
    Lq, p = 192, 100
    qkv, tgt = self_inputs(kind, Lq, GROUPS[0], seed=5)
    out = run_self(kind, qkv, tgt, Lq)
    g = torch.Generator().manual_seed(6)
    other = qkv.clone().view(B, Lq, 3, H, 64)
    other[:, p + 1:, 1:] = (torch.randn(B, Lq - p - 1, 2, H, 64, generator=g) * 3.0).to(ct_of(kind)).cuda()
    got = run_self(kind, other.view(B * Lq, 3, H, 64), tgt, Lq)
    assert same(got[:, :p + 1], out[:, :p + 1]), "a query saw a key behind it"
    assert not same(got[:, p + 1:], out[:, p + 1:])         # (the change is visible where it should be)


@pytest.mark.parametrize("T", [128, 256])
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_cross_form(kind, T):
    what = f"cross {kind} T {T}"
    Bc, Lq, row0 = 4, 128, 1
    ct = ct_of(kind)
    g = torch.Generator().manual_seed(T)
    cache = torch.randn(2, Bc, H, T, 64, generator=g).to(ct).cuda()
    q = (torch.randn(B * Lq, H, 64, generator=g) * 0.35).to(ct).cuda()
    cache0 = cache.clone()
    es = cache.element_size()

    def run(seg=None):
        n, b0 = (B, 0) if seg is None else (1, seg)
        full, out = guarded_out(kind, n * Lq)
        launch(kind, q=q.data_ptr() + b0 * Lq * HD * es, q_stride=HD, k=cache[0, row0 + b0].data_ptr(),
               v=cache[1, row0 + b0].data_ptr(), kv_stride=64, kv_bstride=H * T * 64, kv_hstride=T * 64, key_tgt=None, out=out,
               out_stride=HD, B=n, H=H, Lq=Lq, n_keys=T, causal=0)
        assert guards_intact(full, n * Lq), "a store outside the out rows"
        return out.clone().view(n, Lq, H, 64)

    out = run()
    assert same(cache, cache0), "the launch wrote to the cache"
    k, v = (cache[i, row0:row0 + B].permute(0, 2, 1, 3) for i in (0, 1))          # [B][T][H][64]
    ref = R.prefill_attention_ref(q.view(B, Lq, H, 64), k, v, False)
    model = R.prefill_attention_ref(q.view(B, Lq, H, 64), k, v, False, p_dtype=ct, out_dtype=ct)
    check(kind, what, out, ref, model, [])
    for b in range(B):
        assert same(run(seg=b)[0], out[b]), (what, "segment alone differs", b)
