"""mt3_engine_score_segments on the GPU (include/mt3_hip.h): 19 segments through an engine of 8 slots -- chunks of 8, 8
and 3 -- at length 70 (padded to 128 rows).  Bit-identity with encode(chunk) + score(chunk) in f32 and bf16 (the last
bf16 chunk inside a padded pass of 8), the top-1 statistics against the logits of score(..., return_logits=True),
repeatability, the decode state left alone, the chunk count and the e4m3 refusal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, network  # noqa: E402
from oracle import frontend as OF  # noqa: E402

T, LMAX, V, B, N, LEN = 256, 128, 1536, 8, 19, 70


def _bits(a):
    return a.cpu().numpy().view(np.uint32)


def _engine(dtype, params, kv_dtype=""):
    eng = network.Transformer(network.T5Config(dtype=dtype, kv_dtype=kv_dtype), input_length=T,
                              max_decode_length=LMAX, max_batch=B)
    eng.load_params(params)
    return eng


@pytest.fixture(scope="module")
def case():
    params = network.init_random_params(network.T5Config(dtype="float32"), seed=0, norm_scale_jitter=0.2)
    audio = OF.synth_audio(N, seed=21)
    x = np.stack([OF.compute_logmel(a, np.float32) for a in audio])
    x[5, 77:] = 0.0                                           # a short segment
    rng = np.random.default_rng(5)
    tgt = rng.integers(3, 3 + 1388, size=(N, LEN)).astype(np.int32)      # drawn as in test_gpu_score.py
    tgt[1, 30:] = 0                                           # a row padded after 30 tokens
    tgt[4, :] = 0                                             # an all-zero row
    tgt[10, 20] = 0                                           # a 0 inside the targets
    tgt[17, ::7] = 1                                          # EOS ids as inputs (in the last chunk)
    tgt[12, :] = 1                                            # a row of EOS ids
    xd = torch.from_numpy(x).cuda()
    f32 = _engine("float32", params)
    # the per-chunk reference, computed once: encode(chunk) + score(chunk)
    seq, tok, lg = [], [], []
    for s in range(0, N, B):
        f32.encode(xd[s:s + B])
        a, b, c = f32.score(tgt[s:s + B], return_token_scores=True, return_logits=True)
        seq.append(a), tok.append(b), lg.append(c.cpu().numpy())
    return dict(params=params, x=xd, tgt=tgt, eng=f32, seq=torch.cat(seq), tok=torch.cat(tok), lg=np.concatenate(lg))


def test_f32_scores_are_the_bits_of_encode_plus_score(case):
    c = case
    seq, tok = c["eng"].score_segments(c["x"], c["tgt"], return_token_scores=True)
    assert c["eng"].status(_lib.STATUS_SCORE_CHUNKS) == 3
    assert seq.shape == (N,) and tok.shape == (N, LEN)
    assert np.array_equal(_bits(seq), _bits(c["seq"]))
    assert np.array_equal(_bits(tok), _bits(c["tok"]))
    # ... and with the top-1 outputs the other reduction kernel runs: same bits again
    seq2, tok2, ids, top = c["eng"].score_segments(c["x"], c["tgt"], return_token_scores=True, return_top1=True)
    assert c["eng"].status(_lib.STATUS_SCORE_CHUNKS) == 3
    assert np.array_equal(_bits(seq2), _bits(c["seq"])) and np.array_equal(_bits(tok2), _bits(c["tok"]))
    only = c["eng"].score_segments(c["x"], c["tgt"])
    assert np.array_equal(_bits(only), _bits(c["seq"]))
    tok_np = tok.cpu().numpy()
    assert np.all(tok_np[c["tgt"] == 0] == 0) and float(seq[4]) == 0.0


def test_top1_is_the_argmax_of_the_score_logits(case):
    c = case
    _, tok, ids, top = c["eng"].score_segments(c["x"], c["tgt"], return_token_scores=True, return_top1=True)
    ids, top, tok = ids.cpu().numpy(), top.cpu().numpy(), tok.cpu().numpy()
    live = c["tgt"] > 0
    lg = c["lg"].astype(np.float64)
    assert ids.dtype == np.int32 and np.array_equal(ids[live], c["lg"].argmax(-1)[live])      # numpy: the first maximum
    assert np.all(ids[~live] == 0) and np.all(top[~live] == 0)
    m = lg.max(-1)
    lse = m + np.log(np.exp(lg - m[..., None]).sum(-1))
    err = np.abs(top - (m - lse))[live]
    print("top1_score: worst |err| against the float64 log-softmax %.3e" % err.max())
    assert err.max() <= 1e-5
    margin = tok - top
    assert np.all(margin[live] <= 0) and np.all(margin[live & (ids == c["tgt"])] == 0)


def test_two_calls_give_the_same_bits_and_the_decode_state_is_left_alone(case):
    c = case
    eng = c["eng"]
    eng.encode(c["x"][16:])                                   # the last chunk
    ids0 = eng.decode(num_steps=16).cpu().numpy()
    a = eng.score_segments(c["x"], c["tgt"], return_token_scores=True, return_top1=True)
    b = eng.score_segments(c["x"], c["tgt"], return_token_scores=True, return_top1=True)
    for u, v in zip(a, b):
        assert np.array_equal(u.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32))
    # the call leaves the engine encoded with its last chunk: a decode right after it is the decode of that chunk
    ids1 = eng.decode(num_steps=16).cpu().numpy()
    assert ids1.shape[0] == N - 16 and np.array_equal(ids0, ids1)


def test_bf16_scores_are_the_bits_of_padded_chunks(case):
    c = case
    eng = _engine("bfloat16", c["params"])
    seq, tok = eng.score_segments(c["x"], c["tgt"], return_token_scores=True)
    assert eng.status(_lib.STATUS_SCORE_CHUNKS) == 3
    for s in (0, 8):
        eng.encode(c["x"][s:s + 8])
        a, b = eng.score(c["tgt"][s:s + 8], return_token_scores=True)
        assert np.array_equal(_bits(seq[s:s + 8]), _bits(a)) and np.array_equal(_bits(tok[s:s + 8]), _bits(b))
    # the last 3 segments encoded inside a pass of 8 (segments 11 .. 18): rows 5 .. 7 of that pass
    eng.encode(c["x"][11:19])
    a, b = eng.score(c["tgt"][11:19], return_token_scores=True)
    assert np.array_equal(_bits(seq[16:]), _bits(a[5:])) and np.array_equal(_bits(tok[16:]), _bits(b[5:]))
    np.testing.assert_allclose(seq.cpu().numpy(), c["seq"].cpu().numpy(), rtol=1e-2)
    seq2, tok2, ids, top = eng.score_segments(c["x"], c["tgt"], return_token_scores=True, return_top1=True)
    assert np.array_equal(_bits(seq2), _bits(seq)) and np.array_equal(_bits(tok2), _bits(tok))
    assert np.all((tok2 - top).cpu().numpy() <= 0)


def test_e4m3_caches_are_refused():
    params = network.init_random_params(network.T5Config(dtype="bfloat16"), seed=0)
    eng = _engine("bfloat16", params, kv_dtype="fp8_e4m3")
    x = torch.zeros((2, T, 512), device="cuda")
    with pytest.raises(ValueError):
        eng.score_segments(x, np.full((2, 8), 5, np.int32))
    tgt = torch.full((2, 8), 5, device="cuda", dtype=torch.int32)
    seq = torch.empty(2, device="cuda")
    assert eng._lib.mt3_engine_score_segments(eng._h, x.data_ptr(), 2, 8, tgt.data_ptr(), seq.data_ptr(), None, None, None,
                                              None) == _lib.MT3_ERR_INVALID
    assert b"mt3_engine_score_segments: engines with e4m3" in eng._lib.mt3_last_error()
