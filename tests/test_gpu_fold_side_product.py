"""The qkv-fold as two launches (round 7): the product that feeds the NEXT consumer of a decoder layer's output row,

    out2 = y2 . Wext + h . (Wo_mlp . Wext)        (h = GEGLU output, y2 = the residual row the GEGLU launch reads)

is split where its inputs become ready: `P = y2 . Wext` is a side product of the GEGLU launch (extra column tiles:
no 1/rms, no GELU, plain f32 store), and the MLP out-projection launch adds `h . (Wo_mlp . Wext)` to it over K = mlp.
Both launches through the C ABI (mt3_op_gemm_side) against float64 on the same (already rounded) operands, with the
tolerances tests/test_gpu_kernels.py uses for the same epilogues and K (GEGLU 8e-3 bf16 / 3e-5 f32; RESID and f32
outputs 2e-5 rel-L2), then the f32 engine against the oracle network and against its own separate-projection path
with the bounds tests/test_gpu_parity_r3.py states for them (1e-4 and 2e-5 per (step, row)).
"""
import dataclasses
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, network  # noqa: E402

BF16, F32 = _lib.MT3_BF16, _lib.MT3_F32
EMB, MLP = 512, 1024


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rel(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _gelu_tanh(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _side(dtype, A, Wt, out, M, n_split, n_side, K, epi, side, a_ss=None, out_ct=None, out_ss=None, concurrent=0):
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.check(_lib.load().mt3_op_gemm_side(dtype, A.data_ptr(), Wt.data_ptr(), out.data_ptr(), M, n_split, n_side, K, epi,
                                            p(a_ss), p(out_ct), p(out_ss), side.data_ptr(), concurrent, _stream()))
    torch.cuda.synchronize()


def _case(dtype, M, nx, seed, concurrent=0):
    """Operands of one layer's ops 6 and 7 at the MT3 shape; the rows have an rms between 12 and 42 so that
    a 1/rms factor applied where it does not belong, or left out where it does, is an error of order one."""
    ct = torch.bfloat16 if dtype == BF16 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, EMB, device="cuda", generator=g) * (12 + 30 * torch.rand(M, 1, device="cuda", generator=g))
    xc = x.to(ct)
    ss = (x.double() ** 2).view(M, EMB // 16, 16).sum(-1).float()
    w0 = (torch.randn(EMB, MLP, device="cuda", generator=g) / math.sqrt(EMB)).to(ct)
    w1 = (torch.randn(EMB, MLP, device="cuda", generator=g) / math.sqrt(EMB)).to(ct)
    wext = (torch.randn(nx, EMB, device="cuda", generator=g) / math.sqrt(EMB)).to(ct)
    nx64 = (nx + 63) // 64 * 64
    wi = torch.full((2 * MLP + nx64, EMB), 1.0e30, device="cuda").to(ct)      # padding rows: never stored
    wi[:2 * MLP].view(MLP // 16, 2, 16, EMB)[:, 0] = w0.T.reshape(MLP // 16, 16, EMB)
    wi[:2 * MLP].view(MLP // 16, 2, 16, EMB)[:, 1] = w1.T.reshape(MLP // 16, 16, EMB)
    wi[2 * MLP:2 * MLP + nx] = wext
    wfold = (torch.randn(EMB + nx, MLP, device="cuda", generator=g) / math.sqrt(MLP)).to(ct)
    y0 = torch.randn(M, EMB, device="cuda", generator=g)
    return ct, x, xc, ss, w0, w1, wext, wi, wfold, y0


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("nx", [1536, 1664, 1568])       # 4 * HD, the ismir2021 vocabulary, a width that ends mid-tile
@pytest.mark.parametrize("M", [1, 31, 64, 65])
def test_geglu_side_product_then_fold_against_float64(dtype, nx, M):
    ct, x, xc, ss, w0, w1, wext, wi, wfold, y0 = _case(dtype, M, nx, 1000 * M + nx)
    sentinel = -12345.0
    h = torch.zeros(M, MLP, device="cuda", dtype=ct)
    side = torch.full((M + 1, nx), sentinel, device="cuda")                  # row M: guard behind the last row
    _side(dtype, xc, wi, h, M, 2 * MLP, nx, EMB, _lib.EPI_GEGLU, side, a_ss=ss)
    rs = torch.rsqrt((x.double() ** 2).mean(-1, keepdim=True) + 1e-6)
    h_ref = _gelu_tanh((xc.double() @ w0.double()) * rs) * ((xc.double() @ w1.double()) * rs)
    p_ref = xc.double() @ wext.double().T
    e_h, e_p = _rel(h, h_ref), _rel(side[:M], p_ref)
    print(f"dtype {dtype} M {M} nx {nx}: GEGLU columns rel-L2 {e_h:.3e}, side product rel-L2 {e_p:.3e}")
    assert e_h < (8e-3 if dtype == BF16 else 3e-5), e_h
    assert e_p < 2e-5, e_p
    assert bool((side[M] == sentinel).all()), "the side product wrote past its last row (edge tile)"
    # no 1/rms on the side columns, row by row: the row with the largest norm would be off by its rms (>= 10)
    worst = ((side[:M].double() - p_ref).norm(dim=1) / p_ref.norm(dim=1)).max()
    assert float(worst) < 1e-4, float(worst)
    assert float(rs.max()) < 0.1                                             # (every row of this case has an rms >= 10)
    # ---- op 7: y += h . Wo^T, side += h . (Wo . Wext)^T over K = mlp
    y = y0.clone()
    y_ct = torch.zeros(M, EMB, device="cuda", dtype=torch.bfloat16) if dtype == BF16 else None
    y_ss = torch.zeros(M, EMB // 16, device="cuda")
    p_got = side[:M].clone()
    _side(dtype, h, wfold, y, M, EMB, nx, MLP, _lib.EPI_RESID, side, out_ct=y_ct, out_ss=y_ss)
    y_ref = y0.double() + h.double() @ wfold[:EMB].double().T
    o_ref = p_got.double() + h.double() @ wfold[EMB:].double().T
    e_y, e_o = _rel(y, y_ref), _rel(side[:M], o_ref)
    print(f"dtype {dtype} M {M} nx {nx}: RESID columns rel-L2 {e_y:.3e}, joined second product rel-L2 {e_o:.3e}")
    assert e_y < 2e-5 and e_o < 2e-5, (e_y, e_o)
    assert bool((side[M] == sentinel).all())
    ssr = (y.double() ** 2).view(M, EMB // 16, 16).sum(-1)
    assert float(((y_ss.double() - ssr).abs() / ssr).max()) < 1e-5
    if y_ct is not None:
        assert torch.equal(y_ct, y.to(torch.bfloat16))
    # the whole second product against the one-launch formula of rounds 3-6 in float64: [h | y2] . [Wo.Wext ; Wext]
    two_source = torch.cat([h.double(), xc.double()], 1) @ torch.cat([wfold[EMB:].double(), wext.double()], 1).T
    assert _rel(side[:M], two_source) < 2e-5


def test_large_concurrent_row_groups_take_the_same_bits():
    """>= 256 rows with `concurrent`: the 64 x 32 x 128 tiles get the same two kinds of column tiles and must agree bit
    for bit with the 32-row tiles (same K order per output element)."""
    M, nx = 300, 1536
    ct, x, xc, ss, w0, w1, wext, wi, wfold, y0 = _case(F32, M, nx, 7)
    out = {}
    for conc in (0, 1):
        h = torch.zeros(M, MLP, device="cuda")
        side = torch.zeros(M, nx, device="cuda")
        _side(F32, xc, wi, h, M, 2 * MLP, nx, EMB, _lib.EPI_GEGLU, side, a_ss=ss, concurrent=conc)
        y = y0.clone()
        y_ss = torch.zeros(M, EMB // 16, device="cuda")
        _side(F32, h, wfold, y, M, EMB, nx, MLP, _lib.EPI_RESID, side, out_ss=y_ss, concurrent=conc)
        out[conc] = (h, side, y, y_ss)
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)
    ref = xc.double() @ wext.double().T + out[0][0].double() @ wfold[EMB:].double().T
    assert _rel(out[0][1], ref) < 2e-5


def test_side_launch_argument_errors():
    lib = _lib.load()
    t = torch.zeros(64, 64, device="cuda")
    p = t.data_ptr()
    # GEGLU without partial sums; an epilogue that has no side product; a_ss with K below one float4 of partials
    assert lib.mt3_op_gemm_side(F32, p, p, p, 1, 64, 64, 64, _lib.EPI_GEGLU, None, None, None, p, 0, None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_op_gemm_side(F32, p, p, p, 1, 64, 64, 64, _lib.EPI_STORE, None, None, None, p, 0, None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_op_gemm_ex(F32, p, 0, 2, p, p, 1, 64, 32, _lib.EPI_STORE, None, 0, 1, p, None, None, None) == _lib.MT3_ERR_INVALID


def test_f32_engine_step_with_the_split_fold_against_the_oracle_and_the_separate_projections():
    """Two decoder layers, so both kinds of side product run in every step (layer 0: 4HD columns into the next layer's
    q | k | v | cross-q row; layer 1: the vocabulary's columns into the logits), MT3 shape, f32.  The logits of a step
    are a function of every layer's projected row, so they check both.  Bounds as stated in tests/test_gpu_parity_r3.py
    for the same comparison: 1e-4 rel-L2 per (step, row) against the f32 oracle, 2e-5 against the engine's own path
    with separate q / k / v launches (norm-fused GEMMs on the finished row: the parent's formula without the fold).
    The measured values are printed (MI355X, round 7: 9.5e-7 against the oracle, 9.9e-7 against the separate launches)."""
    from oracle import frontend as OF
    from oracle import network as ON
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    cfg = dataclasses.replace(network.T5Config(dtype="float32"), num_encoder_layers=2, num_decoder_layers=2)
    params = network.init_random_params(cfg, seed=3, norm_scale_jitter=0.2)
    B, S = 3, 12
    audio = OF.synth_audio(B, seed=17).reshape(B, -1)
    x = np.stack([OF.compute_logmel(a, np.float32) for a in audio])
    forced = np.random.default_rng(5).integers(3, 3 + 1388, size=(B, S)).astype(np.int32)
    orc = ON.Oracle(params, ON.T5Config(vocab_size=cfg.vocab_size, emb_dim=cfg.emb_dim, num_heads=cfg.num_heads,
                                        num_encoder_layers=2, num_decoder_layers=2, mlp_dim=cfg.mlp_dim))
    with torch.no_grad():
        enc = orc.encode(x)
        dec_in = np.concatenate([np.zeros((B, 1), np.int32), forced[:, :-1]], 1)
        ref = np.ascontiguousarray(orc.decode_logits(enc, dec_in).numpy().transpose(1, 0, 2)).astype(np.float64)
    outs = {}
    for name, opt in (("split fold", 0), ("separate q/k/v", _lib.OPT_SEPARATE_QKV_PROJECTION)):
        eng = network.Transformer(cfg, input_length=256, max_decode_length=64, max_batch=B, options=opt)
        eng.load_params(params)
        assert eng.status(_lib.STATUS_QKV_FOLD) == (1 if opt == 0 else 0)
        eng.encode(torch.from_numpy(x).cuda())
        _, logits = eng.decode_forced(forced, num_steps=S)
        outs[name] = logits.cpu().numpy().astype(np.float64)
        if opt == 0:
            _, l2 = eng.decode_forced(forced, num_steps=S, use_graph=False)
            assert torch.equal(l2.cpu(), logits.cpu())
            assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0
        del eng

    def rel_rows(a, b):
        return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-30)

    r = rel_rows(outs["split fold"], ref)
    d = rel_rows(outs["split fold"], outs["separate q/k/v"])
    print(f"f32 engine, split fold: logits vs f32 oracle max rel-L2 {r.max():.3e}; vs separate q/k/v launches {d.max():.3e}")
    assert r.max() < 1e-4, r.max()
    assert d.max() < 2e-5, d.max()
