"""The encoder's kernel-alone entry point mt3_op_rmsnorm on a box without a GPU: exported, typed, and every rejection
include/mt3_hip.h lists comes back as MT3_ERR_INVALID, with the entry point's name in mt3_last_error(), before anything
touches a device (the pointers are dummies nobody may dereference)."""
import ctypes as C

from mt3_amd import _lib

X = 0x1000                                     # a non-NULL, 16-byte aligned pointer nobody dereferences
INVALID = _lib.MT3_ERR_INVALID
BF16, F32 = _lib.MT3_BF16, _lib.MT3_F32
_P = C.c_void_p


def rejected(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc == INVALID and name.encode() in lib.mt3_last_error()


def rmsnorm(**kw):
    f = dict(dtype=BF16, x=X, scale=X, out_ct=X, out_f32=X, rows=130, dim=512)
    f.update(kw)
    return rejected("mt3_op_rmsnorm", f["dtype"], f["x"], f["scale"], f["out_ct"], f["out_f32"], f["rows"], f["dim"], None)


def test_entry_point_is_exported_and_typed():
    lib = _lib.load()
    assert "mt3_op_rmsnorm" in _lib.SIGNATURES and hasattr(lib, "mt3_op_rmsnorm")
    fn = lib.mt3_op_rmsnorm
    assert fn.restype == C.c_int
    assert fn.argtypes == _lib.SIGNATURES["mt3_op_rmsnorm"][1]
    # int32 dtype, x, scale, out_ct, out_f32, int32 rows, int32 dim, stream
    assert fn.argtypes == [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, _P]
    assert lib.mt3_abi_version() == 4                                  # an additive entry point


def test_rmsnorm_rejections():
    for dtype in (BF16, F32):
        for outs in (dict(), dict(out_ct=None), dict(out_f32=None)):   # which outputs are given changes nothing
            bad = [dict(x=None), dict(scale=None), dict(x=None, scale=None), dict(rows=0), dict(rows=-1), dict(rows=-130),
                   dict(dim=1), dict(dim=2), dict(dim=3), dict(dim=510), dict(dim=513), dict(dim=767), dict(dim=0),
                   dict(dim=-4), dict(dim=-512)]
            assert all(rmsnorm(dtype=dtype, **c, **outs) for c in bad), (dtype, outs)
    lib = _lib.load()
    for dtype in (2, 7, -1):
        assert rmsnorm(dtype=dtype) and b"dtype" in lib.mt3_last_error()
