"""k-beam search on the engine (mt3_engine_decode_beams, Transformer.decode_beams, InferenceModel(decoding="beam"))
against the CPU reference of tests/beam_search_ref.py and against MT3_DECODE_BEAM1 at k = 1."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, inference, network, synthetic  # noqa: E402
from oracle import frontend as OF  # noqa: E402
from oracle import network as ON  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import beam_search_ref as BR  # noqa: E402

CKPT = os.path.join(HERE, "golden", "mt3_synthetic_ckpt.npz")
F32 = network.T5Config(dtype="float32")
SEG = 32768                      # samples of one 256-frame segment


def _logmel(audio):
    return np.stack([OF.compute_logmel(np.asarray(a), np.float64).astype(np.float32) for a in audio])


def _oracle(params):
    c = F32
    return ON.Oracle(params, ON.T5Config(vocab_size=c.vocab_size, emb_dim=c.emb_dim, num_heads=c.num_heads,
                                         num_encoder_layers=c.num_encoder_layers,
                                         num_decoder_layers=c.num_decoder_layers, head_dim=c.head_dim,
                                         mlp_dim=c.mlp_dim, input_depth=c.input_depth))


def _engine(params, rows, dtype="float32"):
    eng = network.Transformer(network.T5Config(dtype=dtype), input_length=256, max_decode_length=1024, max_batch=rows)
    eng.load_params(params)
    return eng


@pytest.fixture(scope="module")
def boosted():
    """the case set of test_gpu_engine.py::test_beam1_decode_matches_oracle: flat logits, boosted EOS"""
    params = network.init_random_params(F32, seed=1, norm_scale_jitter=0.2)
    k = params["decoder/logits_dense/kernel"].copy() * 0.3
    k[:, 1] *= 1.5
    params["decoder/logits_dense/kernel"] = k
    x = _logmel(OF.synth_audio(6, seed=3))
    x[2, 100:] = 0.0
    return params, x


@pytest.fixture(scope="module")
def trained():
    params = checkpoints.load_compact_npz(CKPT)
    _, wav = synthetic.synth_music(4 * SEG / 16000.0 + 0.5, seed=21)
    wav = np.asarray(wav, np.float32).reshape(-1)[: 4 * SEG].reshape(4, SEG)
    return params, _logmel(wav)


def test_k1_equals_beam1(boosted, trained):
    for params, x, steps in ((*boosted, 32), (*trained, 1024)):
        eng = _engine(params, x.shape[0])
        eng.encode(torch.from_numpy(x).cuda())
        for kw in ({}, dict(use_graph=False), dict(early_exit=True), dict(early_exit=True, use_graph=False)):
            ref = eng.decode(num_steps=steps, beam1=True, **kw).cpu().numpy()
            ids, scores = eng.decode_beams(1, num_steps=steps, **kw)
            assert np.array_equal(ids.cpu().numpy(), ref), kw
            assert torch.isfinite(scores).all()
        del eng


@pytest.mark.parametrize("k", [2, 4])
def test_f32_matches_the_cpu_reference(boosted, k):
    params, x = boosted
    steps = 48
    orc = _oracle(params)
    with torch.no_grad():
        enc = orc.encode(x)
    ref, ref_scores, _ = BR.oracle_beam_search(orc, enc, k, steps)
    beam1 = orc.beam1_decode(enc, steps)
    best = ref[:, -1]
    # the case set discriminates: beam-k differs from beam-1, fills a finished set before L, and leaves a row unfinished
    assert (best != beam1).any(axis=1).sum() >= 2
    assert ((ref == 1).any(axis=2).sum(axis=1) == k).any()
    assert (~(ref == 1).any(axis=(1, 2))).any()
    eng = _engine(params, x.shape[0] * k)
    eng.encode(torch.from_numpy(x).cuda(), num_beams=k)
    all_ids, scores = eng.decode_beams(k, num_steps=steps, return_all=True)
    assert eng.status(_lib.STATUS_LAST_DECODE_FORKS) > 0
    all_ids, scores = all_ids.cpu().numpy(), scores.cpu().numpy()
    assert (all_ids[:, :, steps:] == 0).all()
    assert np.array_equal(all_ids[:, :, :steps], ref)
    # within 1e-5, or 1e-6 of the score: an f32 running sum of up to 48 log-probs, |score| ~300 on a row that never finishes
    assert (np.abs(scores - ref_scores) <= 1e-5 + 1e-6 * np.abs(ref_scores)).all()
    ids, top = eng.decode_beams(k, num_steps=steps, use_graph=False)
    assert np.array_equal(ids.cpu().numpy()[:, :steps], best)
    assert (np.abs(top.cpu().numpy() - ref_scores[:, -1]) <= 1e-5 + 1e-6 * np.abs(ref_scores[:, -1])).all()


def test_invalid_calls_are_rejected(boosted):
    params, x = boosted
    eng = _engine(params, 8)
    eng.encode(torch.from_numpy(x[:2]).cuda(), num_beams=4)
    ids = torch.empty((2, 1024), device="cuda", dtype=torch.int32)
    lib, h, s = eng._lib, eng._h, torch.cuda.current_stream().cuda_stream
    for batch, k, flags in ((2, 4, _lib.DECODE_BEAM1), (2, 4, _lib.DECODE_ASYNC), (2, 4, 1 << 8), (1, 9, 0),
                            (2, 0, 0), (4, 4, 0), (1, 4, 0)):
        assert lib.mt3_engine_decode_beams(h, batch, k, 8, flags, ids.data_ptr(), None, None, None, s) == \
            _lib.MT3_ERR_INVALID, (batch, k, flags)
    assert lib.mt3_engine_decode_beams(h, 2, 4, 8, 0, ids.data_ptr(), None, None, None, s) == _lib.MT3_OK


def test_schedules_agree():
    """B * k = 128 rows: the row-group schedule (2 groups) equals one stream, graph replay equals direct launches"""
    params = network.init_random_params(F32, seed=1, norm_scale_jitter=0.2)
    kern = params["decoder/logits_dense/kernel"].copy() * 0.3
    kern[:, 1] *= 1.5
    params["decoder/logits_dense/kernel"] = kern
    x = _logmel(OF.synth_audio(32, seed=5))
    eng = _engine(params, 128)
    eng.encode(torch.from_numpy(x).cuda(), num_beams=4)
    runs = {}
    for name, kw in (("groups", {}), ("single", dict(single_stream=True)), ("direct", dict(use_graph=False)),
                     ("groups_early", dict(early_exit=True))):
        a, s = eng.decode_beams(4, num_steps=64, return_all=True, **kw)
        runs[name] = (a.cpu().numpy(), s.cpu().numpy(), eng.status(_lib.STATUS_LAST_DECODE_GROUPS))
    assert runs["groups"][2] == 2 and runs["single"][2] == 1
    for name in ("single", "direct", "groups_early"):
        assert np.array_equal(runs[name][0], runs["groups"][0]), name
        assert np.array_equal(runs[name][1], runs["groups"][1]), name


def test_early_exit_is_exact_on_the_trained_fixture(trained):
    params, x = trained
    eng = _engine(params, x.shape[0] * 4)
    eng.encode(torch.from_numpy(x).cuda(), num_beams=4)
    full, fs = eng.decode_beams(4, return_all=True)
    early, es = eng.decode_beams(4, return_all=True, early_exit=True)
    print("beam-4 steps_run with early exit:", eng.steps_run)
    assert eng.steps_run < 1024
    assert np.array_equal(full.cpu().numpy(), early.cpu().numpy())
    assert np.array_equal(fs.cpu().numpy(), es.cpu().numpy())


def test_inference_model_beam4_matches_the_cpu_reference(trained):
    params, x = trained
    x = x[:2]
    m = inference.InferenceModel(params, "mt3", dtype="float32", decoding="beam", num_beams=4, max_slots=8)
    got = m.predict_tokens({"encoder_input_tokens": x})
    orc = _oracle(params)
    with torch.no_grad():
        enc = orc.encode(x)
    ref, _, _ = BR.oracle_beam_search(orc, enc, 4, 1024)
    want = m.vocabulary.decode_tf(ref[:, -1])
    assert np.array_equal(got, np.asarray(want))         # same tokens, hence the same notes


def test_bf16_beam4_agrees_with_f32(trained):
    """bf16 beam-4 against f32 beam-4 on the trained fixture: the fraction of segments whose best decode is identical
    (published as measured; a token-level stand-in for the note F1 bar, which needs longer audio)"""
    params, x = trained
    out = {}
    for dtype in ("float32", "bfloat16"):
        eng = _engine(params, x.shape[0] * 4, dtype)
        eng.encode(torch.from_numpy(x).cuda(), num_beams=4)
        ids, _ = eng.decode_beams(4, early_exit=True)
        out[dtype] = ids.cpu().numpy()
        del eng
    same = np.mean([np.array_equal(a, b) for a, b in zip(out["float32"], out["bfloat16"])])
    print("bf16 vs f32 beam-4: identical rows", same)
    assert same >= 0.5
