"""mt3_engine_score_candidates on the GPU (include/mt3_hip.h): `per` target rows on every segment's ONE encoder pass.
The contract is bit-identity with mt3_engine_score_segments on the job with every segment repeated `per` times -- sequence
scores, token scores, top-1 ids and top-1 scores, torch.equal -- on the random-weight engine of tests/test_gpu_score_segments.py
(8 slots, length 70 padded to 128 rows)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, network  # noqa: E402
from oracle import frontend as OF  # noqa: E402

T, LMAX, B, N, LEN = 256, 128, 8, 11, 70


def _engine(dtype, params):
    eng = network.Transformer(network.T5Config(dtype=dtype), input_length=T, max_decode_length=LMAX, max_batch=B)
    eng.load_params(params)
    return eng


def _targets(rows, seed):
    """ragged rows: lengths 0 (all padding) .. LEN, ids drawn as in tests/test_gpu_score_segments.py, some ending in EOS"""
    rng = np.random.default_rng(seed)
    tgt = rng.integers(3, 3 + 1388, size=(rows, LEN)).astype(np.int32)
    lengths = rng.integers(1, LEN + 1, rows)
    lengths[rows // 2] = 0                                    # an all-padding row
    lengths[0] = LEN
    for r, n in enumerate(lengths):
        tgt[r, n:] = 0
        if n and r % 2:
            tgt[r, n - 1] = 1
    return torch.from_numpy(tgt).cuda()


@pytest.fixture(scope="module")
def case():
    params = network.init_random_params(network.T5Config(dtype="float32"), seed=0, norm_scale_jitter=0.2)
    x = np.stack([OF.compute_logmel(a, np.float32) for a in OF.synth_audio(N, seed=33)])
    x[2, 90:] = 0.0                                           # a short segment
    return dict(params=params, x=torch.from_numpy(x).cuda(), eng=_engine("float32", params))


def _same(eng, x, tgt, per):
    """both calls with every output; -> (encoder passes, prefill pieces) of the candidates call"""
    got = eng.score_candidates(x, tgt, per, return_token_scores=True, return_top1=True)
    passes, pieces = eng.status(_lib.STATUS_SCORE_ENCODER_PASSES), eng.status(_lib.STATUS_SCORE_CHUNKS)
    want = eng.score_segments(x.repeat_interleave(per, 0), tgt, return_token_scores=True, return_top1=True)
    assert eng.status(_lib.STATUS_SCORE_ENCODER_PASSES) == -(-x.shape[0] * per // B)
    for name, a, b in zip(("sequence scores", "token scores", "top-1 ids", "top-1 scores"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), name
    only = eng.score_candidates(x, tgt, per)
    assert torch.equal(only, want[0])                         # without a top-1 output the other reduction runs
    return passes, pieces


@pytest.mark.parametrize("per", [1, 5])
def test_three_segments(case, per):
    passes, pieces = _same(case["eng"], case["x"][:3], _targets(3 * per, per), per)
    assert passes == 1 and pieces == -(-3 * per // B)         # one pass; pieces of 8 rows (the workspace default)


def test_rows_cross_a_prefill_piece_inside_a_segment(case):
    eng = case["eng"]
    eng.debug_set_score_chunk(4)                              # pieces of 4 rows: segment 0's five rows span two pieces
    try:
        passes, pieces = _same(eng, case["x"][:3], _targets(15, 7), 5)
    finally:
        eng.debug_set_score_chunk(0)
    assert passes == 1 and pieces == 4


def test_two_encoder_chunks(case):
    passes, pieces = _same(case["eng"], case["x"], _targets(N * 3, 9), 3)
    assert passes == 2                                        # 8 + 3 segments, not ceil(33 / 8) = 5 passes
    assert pieces == 3 + 2                                    # 24 rows and 9 rows in pieces of 8


def test_the_decode_state_is_left_alone(case):
    eng, x = case["eng"], case["x"]
    eng.encode(x[8:])                                         # the last chunk of the call below
    before = eng.decode(num_steps=16).cpu().numpy()
    eng.score_candidates(x, _targets(N * 2, 3), 2)
    after = eng.decode(num_steps=16).cpu().numpy()
    assert after.shape[0] == N - 8 and np.array_equal(before, after)


def test_bf16_is_exact_when_every_pass_holds_eight_segments(case):
    """8 segments, 3 candidates: one pass of 8 here, three passes of 8 on the replicated job (the condition
    mt3_engine_encode documents)"""
    eng = _engine("bfloat16", case["params"])
    passes, pieces = _same(eng, case["x"][:8], _targets(24, 4), 3)
    assert passes == 1 and pieces == 3


def test_python_refusals(case):
    eng, x = case["eng"], case["x"]
    with pytest.raises(ValueError):
        eng.score_candidates(x[:2], _targets(5, 1), 3)        # 5 rows for 2 * 3
    with pytest.raises(ValueError):
        eng.score_candidates(x[:2], _targets(6, 1), 0)
