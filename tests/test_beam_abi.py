"""mt3_engine_decode_beams on a box without a GPU: exported, typed, and argument errors come back as MT3_ERR_INVALID."""
import ctypes as C

from mt3_amd import _lib


def test_decode_beams_is_exported_and_rejects_bad_calls():
    lib = _lib.load()
    assert "mt3_engine_decode_beams" in _lib.SIGNATURES and hasattr(lib, "mt3_engine_decode_beams")
    assert _lib.STATUS_LAST_DECODE_FORKS == 10 and _lib.MAX_BEAMS == 8
    ran = C.c_int32(-1)
    for k, flags in ((4, 0), (0, 0), (9, 0), (2, _lib.DECODE_BEAM1), (2, _lib.DECODE_ASYNC), (2, 1 << 8)):
        assert lib.mt3_engine_decode_beams(None, 1, k, 8, flags, None, None, None, C.byref(ran), None) == \
            _lib.MT3_ERR_INVALID
        assert b"mt3_engine_decode_beams" in lib.mt3_last_error()
    assert ran.value == -1                     # nothing is reported for a rejected call
    assert lib.mt3_engine_status(None, _lib.STATUS_LAST_DECODE_FORKS) == _lib.MT3_ERR_INVALID
