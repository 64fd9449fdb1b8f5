"""mt3_engine_score on a box without a GPU: exported and typed, argument errors come back as MT3_ERR_INVALID, the
scoring reference's masks, and models.score_batch's input contract."""
import ctypes as C

import numpy as np
import pytest

from mt3_amd import _lib, models, network

torch = pytest.importorskip("torch")
from oracle import network as ON  # noqa: E402

from . import score_ref  # noqa: E402


def test_score_is_exported_and_typed():
    lib = _lib.load()
    assert "mt3_engine_score" in _lib.SIGNATURES and hasattr(lib, "mt3_engine_score")
    assert "mt3_debug_engine_set_score_chunk" in _lib.SIGNATURES and hasattr(lib, "mt3_debug_engine_set_score_chunk")
    assert _lib.STATUS_SCORE_CHUNKS == 11
    assert lib.mt3_abi_version() == 4


def _engine(L=64):
    lib = _lib.load()
    ec = _lib.EngineConfig(1536, 512, 6, 64, 1024, 1, 1, 512, 256, L, 4, _lib.MT3_F32, 0, 0, 0, 0)
    h = C.c_void_p()
    _lib.check(lib.mt3_engine_create(C.byref(ec), C.byref(h)))
    return lib, h


def test_bad_calls_are_rejected_with_the_function_name():
    lib, h = _engine(L=64)
    tgt = (C.c_int32 * 64)()
    seq = (C.c_float * 4)()
    try:
        calls = [
            (None, 1, 8, tgt, seq),          # null engine
            (h, 1, 0, tgt, seq),             # length 0
            (h, 1, 65, tgt, seq),            # length above L
            (h, 1, 8, None, seq),            # null targets
            (h, 1, 8, tgt, None),            # null sequence scores
            (h, 1, 8, tgt, seq),             # engine not finalized
        ]
        for eng, b, n, t, s in calls:
            rc = lib.mt3_engine_score(eng, b, n, C.cast(t, C.c_void_p) if t else None, None, None,
                                      C.cast(s, C.c_void_p) if s else None, None, None, None)
            assert rc == _lib.MT3_ERR_INVALID
            assert b"mt3_engine_score" in lib.mt3_last_error()
        assert lib.mt3_debug_engine_set_score_chunk(None, 1) == _lib.MT3_ERR_INVALID
        assert b"mt3_debug_engine_set_score_chunk" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)


def _tiny():
    cfg = network.T5Config(dtype="float32", vocab_size=32, emb_dim=32, num_heads=2, head_dim=16, mlp_dim=64,
                           num_encoder_layers=1, num_decoder_layers=2, input_depth=16)
    params = network.init_random_params(cfg, seed=3, norm_scale_jitter=0.2)
    ocfg = ON.T5Config(vocab_size=32, emb_dim=32, num_heads=2, num_encoder_layers=1, num_decoder_layers=2, head_dim=16,
                       mlp_dim=64, input_depth=16, max_pos=64)
    orc = ON.Oracle(params, ocfg, dtype=torch.float64)
    enc = torch.randn(2, 8, 32, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    return orc, enc


def test_masked_pass_equals_the_causal_pass_when_padding_is_trailing():
    orc, enc = _tiny()
    rng = np.random.default_rng(0)
    tgt = rng.integers(3, 32, size=(2, 12))
    tgt[0, 9:] = 0                                        # trailing padding only
    masked = score_ref.teacher_forced_logits(orc, enc, tgt).numpy()
    plain = orc.decode_logits(enc, score_ref.shift_right(tgt)).numpy()
    valid = tgt > 0
    np.testing.assert_allclose(masked[valid], plain[valid], rtol=1e-10, atol=1e-10)
    # the scores of the plain pass are then the same as well
    a, sa = score_ref.scores_from_logits(masked, tgt)
    b, sb = score_ref.scores_from_logits(plain, tgt)
    np.testing.assert_allclose(sa, sb, rtol=1e-12)
    assert np.all(a[~valid] == 0)


def test_masked_pass_differs_where_a_zero_sits_inside_a_row():
    orc, enc = _tiny()
    rng = np.random.default_rng(0)
    tgt = rng.integers(3, 32, size=(2, 12))
    tgt[1, 4] = 0                                         # a 0 inside the row: masked as a key from position 5 on
    masked = score_ref.teacher_forced_logits(orc, enc, tgt).numpy()
    plain = orc.decode_logits(enc, score_ref.shift_right(tgt)).numpy()
    np.testing.assert_allclose(masked[1, :4], plain[1, :4], rtol=1e-10, atol=1e-10)
    assert np.abs(masked[1, 5:] - plain[1, 5:]).max() > 1e-6
    np.testing.assert_allclose(masked[0], plain[0], rtol=1e-10, atol=1e-10)


def test_score_batch_needs_every_converter_key():
    feats = models.convert_features([{"inputs": np.zeros((4, 512), np.float32), "targets": np.array([5, 6, 1])}],
                                    {"inputs": 256, "targets": 16})
    for key in models.SCORE_KEYS:
        bad = {k: v for k, v in feats.items() if k != key}
        with pytest.raises(ValueError, match=key):
            models.score_batch(None, bad)
