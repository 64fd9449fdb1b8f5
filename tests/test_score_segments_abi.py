"""mt3_engine_score_segments, mt3_op_score_token_stats and mt3_notes_decode_traced on a box without a GPU: exported and
typed, and every argument error that needs no device comes back as MT3_ERR_INVALID with the function's name."""
import ctypes as C

import pytest

from mt3_amd import _lib

NEW = ("mt3_engine_score_segments", "mt3_op_score_token_stats", "mt3_notes_decode_traced")


def test_the_three_symbols_are_exported_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4
    assert _lib.STATUS_SCORE_CHUNKS == 11


def _engine(L=64, dtype=_lib.MT3_F32, kv=0):
    lib = _lib.load()
    ec = _lib.EngineConfig(1536, 512, 6, 64, 1024, 1, 1, 512, 256, L, 4, dtype, 0, kv, 0, 0)
    h = C.c_void_p()
    _lib.check(lib.mt3_engine_create(C.byref(ec), C.byref(h)))
    return lib, h


def _call(lib, eng, x, n, length, tgt, seq):
    p = (lambda a: C.cast(a, C.c_void_p) if a is not None else None)
    return lib.mt3_engine_score_segments(eng, p(x), n, length, p(tgt), p(seq), None, None, None, None)


def test_score_segments_rejects_bad_calls_before_any_device_work():
    lib, h = _engine(L=64)
    x = (C.c_float * 16)()                   # never read: every call below fails first
    tgt = (C.c_int32 * 64)()
    seq = (C.c_float * 4)()
    try:
        calls = [
            (None, x, 1, 8, tgt, seq),       # null engine
            (h, None, 1, 8, tgt, seq),       # null inputs
            (h, x, 1, 8, None, seq),         # null targets
            (h, x, 1, 8, tgt, None),         # null sequence scores
            (h, x, 0, 8, tgt, seq),          # no segments
            (h, x, -3, 8, tgt, seq),
            (h, x, 1, 0, tgt, seq),          # length 0
            (h, x, 1, 65, tgt, seq),         # length above max_decode_len
            (h, x, 1, 8, tgt, seq),          # engine not finalized
        ]
        for args in calls:
            assert _call(lib, *args) == _lib.MT3_ERR_INVALID, args[2:4]
            assert b"mt3_engine_score_segments" in lib.mt3_last_error()
        assert b"not finalized" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)


def test_score_segments_refuses_e4m3_caches_in_the_style_of_score():
    lib, h = _engine(L=64, dtype=_lib.MT3_BF16, kv=_lib.MT3_FP8_E4M3)
    x, tgt, seq = (C.c_float * 16)(), (C.c_int32 * 64)(), (C.c_float * 4)()
    try:
        assert _call(lib, h, x, 1, 8, tgt, seq) == _lib.MT3_ERR_INVALID
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_engine_score_segments: engines with e4m3 K/V caches")
        rc = lib.mt3_engine_score(h, 1, 8, C.cast(tgt, C.c_void_p), None, None, C.cast(seq, C.c_void_p), None, None, None)
        assert rc == _lib.MT3_ERR_INVALID
        assert lib.mt3_last_error() == msg.replace(b"mt3_engine_score_segments", b"mt3_engine_score")
    finally:
        lib.mt3_engine_destroy(h)


def test_token_stats_op_rejects_bad_calls():
    lib = _lib.load()
    lg, tgt = (C.c_float * 8)(), (C.c_int32 * 4)()
    p = (lambda a: C.cast(a, C.c_void_p) if a is not None else None)
    for logits, targets, rows, vocab in [(None, tgt, 1, 8), (lg, None, 1, 8), (lg, tgt, 0, 8), (lg, tgt, 1, 1),
                                         (lg, tgt, -1, 8), (lg, tgt, 1, 0)]:
        rc = lib.mt3_op_score_token_stats(p(logits), p(targets), None, rows, vocab, None, None, None, None)
        assert rc == _lib.MT3_ERR_INVALID
        assert b"mt3_op_score_token_stats" in lib.mt3_last_error()


def test_python_wrapper_refuses_e4m3_without_touching_the_engine():
    from mt3_amd import network
    torch = pytest.importorskip("torch")
    eng = network.Transformer(network.T5Config(dtype="bfloat16", kv_dtype="fp8_e4m3", num_encoder_layers=1,
                                               num_decoder_layers=1), max_batch=1)
    with pytest.raises(ValueError, match="kv_dtype"):
        eng.score_segments(torch.zeros(1, 256, 512), torch.zeros(1, 8, dtype=torch.int32))
