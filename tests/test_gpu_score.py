"""Teacher-forced scoring on the GPU (mt3_engine_score, include/mt3_hip.h): oracle parity in f32 and bf16 through
tests/score_ref.py, the same function as the cached teacher-forced decode, the link to the k-beam search's scores,
causality, batch invariance across chunks, repeatability, the decode state left alone, the e4m3-cache refusal, and the
end-to-end InferenceModel.score on the trained fixture."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, inference, models, network, synthetic  # noqa: E402
from oracle import frontend as OF  # noqa: E402
from oracle import network as ON  # noqa: E402

from . import score_ref  # noqa: E402

T, L, V = 256, 1024, 1536
CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")


def _inputs(B, seed):
    audio = OF.synth_audio(B, seed=seed)
    return np.stack([OF.compute_logmel(a, np.float32) for a in audio])


def _engine(dtype, params, B, Lmax=L, kv_dtype=""):
    eng = network.Transformer(network.T5Config(dtype=dtype, kv_dtype=kv_dtype), input_length=T,
                              max_decode_length=Lmax, max_batch=B)
    eng.load_params(params)
    return eng


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-30)


@pytest.fixture(scope="module")
def case():
    params = network.init_random_params(network.T5Config(dtype="float32"), seed=0, norm_scale_jitter=0.2)
    B = 8
    x = _inputs(B, seed=21)
    x[5, 77:] = 0.0                                           # a short segment (zero rows after the log)
    rng = np.random.default_rng(5)
    tgt = rng.integers(3, 3 + 1388, size=(B, L)).astype(np.int32)
    tgt[1, 300:] = 0                                          # a row padded after 300 tokens
    tgt[2, ::7] = 1                                           # EOS ids as inputs
    tgt[3, 200] = 0                                           # a 0 inside the targets
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    orc = ON.Oracle(params, ON.T5Config())
    enc = orc.encode(x)
    ref = score_ref.teacher_forced_logits(orc, enc, tgt).numpy()
    tok, seq = score_ref.scores_from_logits(ref, tgt)
    eng = _engine("float32", params, B)
    eng.encode(torch.from_numpy(x).cuda())
    s, ts, lg = eng.score(tgt, return_token_scores=True, return_logits=True)
    return dict(params=params, x=x, tgt=tgt, ref=ref, tok=tok, seq=seq, eng=eng,
                s=s.cpu().numpy(), ts=ts.cpu().numpy(), lg=lg.cpu().numpy())


def test_f32_scores_match_the_oracle(case):
    c = case
    valid = c["tgt"] > 0
    r = _rel(c["lg"], c["ref"])[valid]
    assert r.max() < 1e-4, f"f32 score logits: worst rel-L2 {r.max():.3e}"
    assert np.abs(c["ts"] - c["tok"]).max() < 1e-3
    assert np.all(c["ts"][~valid] == 0)
    np.testing.assert_allclose(c["s"], c["seq"], rtol=1e-5)


def test_bf16_scores_match_the_oracle(case):
    c = case
    eng = _engine("bfloat16", c["params"], 8)
    eng.encode(torch.from_numpy(c["x"]).cuda())
    s, lg = eng.score(c["tgt"], return_logits=True)
    r = _rel(lg.cpu().numpy(), c["ref"])[c["tgt"] > 0]
    assert r.max() < 3e-2, f"bf16 score logits: worst rel-L2 {r.max():.3e}"
    np.testing.assert_allclose(s.cpu().numpy(), c["s"], rtol=1e-2)


def test_score_logits_equal_the_cached_teacher_forced_decode(case):
    c = case
    eng, tgt = c["eng"], c["tgt"]
    _, steps = eng.decode_forced(tgt)                         # input of step t+1 = tgt[:, t]
    steps = steps.cpu().numpy().transpose(1, 0, 2)            # [B, L, V]
    # the cached decode attends padding inputs as keys; the score path masks them: compare up to each row's first 0
    for b in range(tgt.shape[0]):
        zeros = np.flatnonzero(tgt[b] == 0)
        n = zeros[0] if zeros.size else L
        r = _rel(c["lg"][b, :n], steps[b, :n])
        assert r.max() < 1e-4, f"row {b}: worst rel-L2 {r.max():.3e}"


def test_causality_repeatability_and_decode_state(case):
    c = case
    eng, tgt = c["eng"], c["tgt"].copy()
    ids0 = eng.decode(num_steps=32).cpu().numpy()
    s1, t1 = eng.score(tgt, return_token_scores=True)
    s2, t2 = eng.score(tgt, return_token_scores=True)
    assert np.array_equal(s1.cpu().numpy().view(np.uint32), s2.cpu().numpy().view(np.uint32))
    assert np.array_equal(t1.cpu().numpy().view(np.uint32), t2.cpu().numpy().view(np.uint32))
    ids1 = eng.decode(num_steps=32).cpu().numpy()
    assert np.array_equal(ids0, ids1), "a score call changed what the next decode returns"
    p = 500
    alt = tgt.copy()
    alt[:, p + 1:] = np.random.default_rng(9).integers(3, 1000, size=(alt.shape[0], L - p - 1))
    _, t3 = eng.score(alt, return_token_scores=True)
    a, b = t1.cpu().numpy()[:, : p + 1], t3.cpu().numpy()[:, : p + 1]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_scores_match_the_k_beam_search():
    params = network.init_random_params(network.T5Config(dtype="float32"), seed=1)
    k, steps, B = 4, 64, 4
    x = torch.from_numpy(_inputs(B, seed=33)).cuda()
    eng = _engine("float32", params, B * k, Lmax=128)
    eng.encode(x, num_beams=k)
    all_ids, scores = eng.decode_beams(k, num_steps=steps, return_all=True)
    all_ids, scores = all_ids.cpu().numpy()[:, :, :steps], scores.cpu().numpy()
    eng.encode(x, num_beams=k)                                # row b*k + j = segment b, as the decodes are laid out
    s = eng.score(all_ids.reshape(B * k, steps)).cpu().numpy().reshape(B, k)
    checked = 0
    for b in range(B):
        for j in range(k):
            ids, sc = all_ids[b, j], float(scores[b, j])
            if sc < -1e6:
                continue                                      # unfilled finished entry
            eos = np.flatnonzero(ids == 1)
            n = int(eos[0]) + 1 if eos.size else steps
            if np.any(ids[:n] == 0):
                continue                                      # a decoded id 0 would be padding to the score path
            want = sc * ((5.0 + n) / 6.0) ** 0.6 if eos.size else sc
            assert abs(s[b, j] - want) <= 1e-5 * abs(want), (b, j, s[b, j], want)
            checked += 1
    assert checked >= B * k // 2


def test_batch_invariance_across_chunks():
    params = network.init_random_params(network.T5Config(dtype="float32"), seed=2)
    x = _inputs(40, seed=44)
    tgt = np.random.default_rng(3).integers(3, 1000, size=(40, 100)).astype(np.int32)
    tgt[::3, 60:] = 0
    eng = _engine("float32", params, 40, Lmax=128)
    eng.debug_set_score_chunk(16)
    eng.encode(torch.from_numpy(x).cuda())
    s40, t40 = eng.score(tgt, return_token_scores=True)
    assert eng.status(_lib.STATUS_SCORE_CHUNKS) == 3
    eng.encode(torch.from_numpy(x[:8]).cuda())
    s8, t8 = eng.score(tgt[:8], return_token_scores=True)
    assert eng.status(_lib.STATUS_SCORE_CHUNKS) == 1
    assert np.array_equal(s40.cpu().numpy()[:8].view(np.uint32), s8.cpu().numpy().view(np.uint32))
    assert np.array_equal(t40.cpu().numpy()[:8].view(np.uint32), t8.cpu().numpy().view(np.uint32))
    perm = np.random.default_rng(4).permutation(8)
    eng.encode(torch.from_numpy(x[:8][perm]).cuda())
    sp = eng.score(tgt[:8][perm]).cpu().numpy()
    assert np.array_equal(sp.view(np.uint32), s8.cpu().numpy()[perm].view(np.uint32))


def test_e4m3_caches_are_refused():
    params = network.init_random_params(network.T5Config(dtype="bfloat16"), seed=0)
    eng = _engine("bfloat16", params, 2, Lmax=64, kv_dtype="fp8_e4m3")
    eng.encode(torch.from_numpy(_inputs(2, seed=1)).cuda())
    with pytest.raises(ValueError):
        eng.score(np.full((2, 8), 5, np.int32))
    tgt = torch.full((2, 8), 5, device="cuda", dtype=torch.int32)
    seq = torch.empty(2, device="cuda")
    assert eng._lib.mt3_engine_score(eng._h, 2, 8, tgt.data_ptr(), None, None, seq.data_ptr(), None, None,
                                     None) == _lib.MT3_ERR_INVALID


def test_score_batch_and_inference_model_end_to_end():
    trained = checkpoints.load_compact_npz(CKPT)
    _, wav = synthetic.synth_music(3 * 2.048 + 0.5, seed=13, device="cpu")
    m = inference.InferenceModel(trained, "mt3", dtype="float32")
    examples, x = m._examples(wav, 16000)
    net = network.Transformer(m.model_config, input_length=T, max_decode_length=L, max_batch=8)
    net.load_params(trained)
    net.encode(x)
    ids = net.decode().cpu().numpy()                          # the model's own greedy decoding
    targets = []
    for row in ids:
        eos = np.flatnonzero(row == 1)
        targets.append(row[: int(eos[0]) + 1] if eos.size else row)
    n = max(len(t) for t in targets)
    tgt = np.zeros((len(targets), n), np.int32)
    for i, t in enumerate(targets):
        tgt[i, : len(t)] = t
    s_net, lg = net.score(tgt, return_logits=True)
    s_inf = m.score(wav, targets)
    assert s_inf.shape == (len(examples),) and s_inf.dtype == np.float64
    assert np.array_equal(s_inf, s_net.cpu().numpy().astype(np.float64))
    # greedy ids are the arg-max of the score path's logits wherever the top-2 margin is clear
    lg = lg.cpu().numpy()
    top2 = np.sort(lg, -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0] > 1e-3) & (tgt > 0)
    assert clear.sum() > 0
    assert np.array_equal(lg.argmax(-1)[clear], tgt[clear])
    # models.score_batch on the converter's dict of the same segments: the same scores
    feats = {"encoder_input_tokens": x.cpu().numpy(), "decoder_target_tokens": tgt,
             "decoder_input_tokens": score_ref.shift_right(tgt).astype(np.int32),
             "decoder_loss_weights": (tgt > 0).astype(np.int32)}
    s_b, inter = models.score_batch(net, feats, return_intermediates=True)
    assert np.array_equal(s_b, s_net.cpu().numpy())
    assert inter["decoder"]["token_scores"][0].shape == tgt.shape
