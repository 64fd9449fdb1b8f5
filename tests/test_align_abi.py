"""mt3_engine_score_candidates and mt3_op_align_paths on a box without a GPU: exported and typed, declared in the header,
and every argument error that needs no device comes back as MT3_ERR_INVALID with a text that starts with the function's
name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mt3_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mt3_engine_score_candidates", "mt3_op_align_paths")


def test_the_symbols_are_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mt3_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"^int %s\(" % name, header, re.M), name
    # the prototypes: one argument of the binding per parameter of the declaration
    for name in NEW:
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.STATUS_SCORE_ENCODER_PASSES == 17 and "MT3_STATUS_SCORE_ENCODER_PASSES = 17" in header
    assert _lib.ALIGN_MAX_SHIFTS == 64 and "#define MT3_ALIGN_MAX_SHIFTS 64" in header
    assert lib.mt3_abi_version() == 4


def _engine(L=64, dtype=_lib.MT3_F32, kv=0):
    lib = _lib.load()
    ec = _lib.EngineConfig(1536, 512, 6, 64, 1024, 1, 1, 512, 256, L, 4, dtype, 0, kv, 0, 0)
    h = C.c_void_p()
    _lib.check(lib.mt3_engine_create(C.byref(ec), C.byref(h)))
    return lib, h


def _p(a):
    return C.cast(a, C.c_void_p) if a is not None else None


def _candidates(lib, eng, x, n, per, length, tgt, seq):
    return lib.mt3_engine_score_candidates(eng, _p(x), n, per, length, _p(tgt), _p(seq), None, None, None, None)


def test_score_candidates_rejects_bad_calls_before_any_device_work():
    lib, h = _engine(L=64)
    x = (C.c_float * 16)()                   # never read: every call below fails first
    tgt = (C.c_int32 * 64)()
    seq = (C.c_float * 4)()
    try:
        calls = [
            ((None, x, 1, 2, 8, tgt, seq), b"null engine"),
            ((h, None, 1, 2, 8, tgt, seq), b"null inputs"),
            ((h, x, 1, 2, 8, None, seq), b"null inputs, targets"),
            ((h, x, 1, 2, 8, tgt, None), b"sequence scores"),
            ((h, x, 0, 2, 8, tgt, seq), b"n_segments must be >= 1"),
            ((h, x, -3, 2, 8, tgt, seq), b"n_segments must be >= 1"),
            ((h, x, 1, 0, 8, tgt, seq), b"per must be >= 1"),
            ((h, x, 1, -5, 8, tgt, seq), b"per must be >= 1"),
            ((h, x, 1 << 16, 1 << 15, 8, tgt, seq), b"must fit int32"),       # 2^31 rows
            ((h, x, 3, 715827883, 8, tgt, seq), b"must fit int32"),
            ((h, x, 1, 2, 0, tgt, seq), b"length must be in 1 .. max_decode_len"),
            ((h, x, 1, 2, 65, tgt, seq), b"length must be in 1 .. max_decode_len"),
            ((h, x, 1, 2, 8, tgt, seq), b"engine not finalized"),
        ]
        for args, what in calls:
            assert _candidates(lib, *args) == _lib.MT3_ERR_INVALID, args[2:5]
            msg = lib.mt3_last_error()
            assert msg.startswith(b"mt3_engine_score_candidates: ") and what in msg, msg
    finally:
        lib.mt3_engine_destroy(h)


def test_score_candidates_refuses_what_score_segments_refuses_in_its_words():
    lib, h = _engine(L=64, dtype=_lib.MT3_BF16, kv=_lib.MT3_FP8_E4M3)
    x, tgt, seq = (C.c_float * 16)(), (C.c_int32 * 64)(), (C.c_float * 4)()
    try:
        assert _candidates(lib, h, x, 1, 2, 8, tgt, seq) == _lib.MT3_ERR_INVALID
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_engine_score_candidates: engines with e4m3 K/V caches")
        assert lib.mt3_engine_score_segments(h, _p(x), 1, 8, _p(tgt), _p(seq), None, None, None, None) == _lib.MT3_ERR_INVALID
        assert lib.mt3_last_error() == msg.replace(b"mt3_engine_score_candidates", b"mt3_engine_score_segments")
    finally:
        lib.mt3_engine_destroy(h)


def test_python_wrappers_refuse_before_touching_the_engine():
    from mt3_amd import network
    torch = pytest.importorskip("torch")
    eng = network.Transformer(network.T5Config(dtype="bfloat16", kv_dtype="fp8_e4m3", num_encoder_layers=1,
                                               num_decoder_layers=1), max_batch=1)
    with pytest.raises(ValueError, match="kv_dtype"):
        eng.score_candidates(torch.zeros(1, 256, 512), torch.zeros(2, 8, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="per must be"):
        eng.score_candidates(torch.zeros(1, 256, 512), torch.zeros(2, 8, dtype=torch.int32), 0)


def _align(lib, scores="ok", total=4, K=2, files=((0, 4),), n_files=None, grid=(0.0, 0.1), lam=1.0, max_jump=float("inf"),
           back="ok", path="ok", out="ok"):
    """the call with host arrays standing in for the device arrays: none is read before the arguments are refused"""
    buf = lambda v, n, t: None if v is None else (t * max(n, 1))()           # noqa: E731
    f = None if files is None else np.ascontiguousarray(np.asarray(files, np.int32).reshape(-1, 2))
    g = None if grid is None else np.ascontiguousarray(np.asarray(grid, np.float64))
    n_files = (0 if f is None else len(f)) if n_files is None else n_files
    return lib.mt3_op_align_paths(_p(buf(scores, 64, C.c_float)), total, K, None if f is None else f.ctypes.data, n_files,
                                  None if g is None else g.ctypes.data, lam, max_jump, _p(buf(back, 64, C.c_uint8)),
                                  _p(buf(path, 64, C.c_int32)), _p(buf(out, 8, C.c_double)), None)


def test_align_paths_rejects_bad_calls_before_any_device_work():
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    calls = [
        (dict(scores=None), b"null scores"),
        (dict(back=None), b"null scores, back-pointer scratch"),
        (dict(path=None), b"path or totals"),
        (dict(out=None), b"path or totals"),
        (dict(files=None, n_files=1), b"null file table"),
        (dict(grid=None), b"null grid"),
        (dict(K=0), b"K must be 1 .. 64"),
        (dict(K=65), b"K must be 1 .. 64"),
        (dict(K=-1), b"K must be 1 .. 64"),
        (dict(grid=(0.0, 0.0)), b"strictly increasing"),
        (dict(grid=(0.1, 0.0)), b"strictly increasing"),
        (dict(grid=(0.0, nan)), b"grid must be finite"),
        (dict(grid=(-inf, 0.0)), b"grid must be finite"),
        (dict(lam=-1e-9), b"smoothness"),
        (dict(lam=nan), b"smoothness"),
        (dict(lam=inf), b"smoothness"),
        (dict(max_jump=-0.5), b"max_jump"),
        (dict(max_jump=nan), b"max_jump"),
        (dict(total=-1), b"total_segments"),
        (dict(n_files=-2), b"n_files"),
        (dict(files=((0, 0),)), b"at least 1 segment"),
        (dict(files=((0, -3),)), b"at least 1 segment"),
        (dict(files=((-1, 2),)), b"inside [0, total_segments]"),
        (dict(files=((2, 3),)), b"inside [0, total_segments]"),
        (dict(files=((4, 1),)), b"inside [0, total_segments]"),
        (dict(files=((0, 3), (2, 2))), b"overlap or are out of order"),
        (dict(files=((2, 2), (0, 2))), b"overlap or are out of order"),
    ]
    for kw, what in calls:
        assert _align(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_align_paths: ") and what in msg, (kw, msg)
    # no files: nothing to do, whatever the device pointers are
    assert _align(lib, files=np.zeros((0, 2)), scores=None, back=None, path=None, out=None) == _lib.MT3_OK


def test_best_paths_wants_a_device_table():
    from mt3_amd import alignment
    with pytest.raises(ValueError, match="CUDA"):
        alignment.best_paths(np.zeros((4, 2), np.float32), [4], [0.0, 0.1], 1.0)
