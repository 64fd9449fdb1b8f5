"""mt3_op_decode_attention_ex on a box without a GPU: exported, typed, the view has the layout of the C struct, and every
argument error -- what the entry point adds and what launch_decode_attention refuses for the engine too -- comes back as
MT3_ERR_INVALID before anything touches a device."""
import ctypes as C

from mt3_amd import _lib

X = 0x1000                                     # a non-NULL pointer nobody dereferences: the calls are rejected first
INVALID = _lib.MT3_ERR_INVALID
BF16, F32 = _lib.MT3_BF16, _lib.MT3_F32


def view(**kw):
    """a complete plain-form append launch; keywords override fields"""
    f = dict(q=X, q_stride=384, cap=64, kcache=X, vcache=X, new_k=X, new_v=X, kv_stride=384, n_keys=0, step=X, out=X, B=4,
             H=6, kv_scale=None, q_f32=None, q_ss=None, q_ss_n=0, reserved=0, done=None, cache_row=None)
    f.update(kw)
    return C.byref(_lib.DecAttnView(**f))


def folded(**kw):
    """the folded form of the same launch: unnormalised f32 rows and the partial sums"""
    f = dict(q=None, q_f32=X, q_ss=X, q_ss_n=32, q_stride=1536, kv_stride=1536)
    f.update(kw)
    return view(**f)


def call(v, dtype=BF16):
    return _lib.load().mt3_op_decode_attention_ex(dtype, v, None)


def test_entry_point_is_exported_and_typed():
    lib = _lib.load()
    name = "mt3_op_decode_attention_ex"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4                                  # an additive entry point
    # LP64 layout of mt3_dec_attn_view: 12 pointers, 4 int32 pairs, no hidden padding
    assert C.sizeof(_lib.DecAttnView) == 128
    offs = {n: getattr(_lib.DecAttnView, n).offset for n, _ in _lib.DecAttnView._fields_}
    assert offs == dict(q=0, q_stride=8, cap=12, kcache=16, vcache=24, new_k=32, new_v=40, kv_stride=48, n_keys=52,
                        step=56, out=64, B=72, H=76, kv_scale=80, q_f32=88, q_ss=96, q_ss_n=104, reserved=108, done=112,
                        cache_row=120)


def test_rejections_the_entry_point_adds():
    lib = _lib.load()
    bad = [lib.mt3_op_decode_attention_ex(BF16, None, None)]
    assert bad == [INVALID] and b"decode_attention_ex" in lib.mt3_last_error()
    assert call(view(cache_row=X)) == INVALID and b"cache_row" in lib.mt3_last_error()      # the map without the flags
    assert call(folded(cache_row=X)) == INVALID
    for dtype in (BF16, F32):
        bad = [call(folded(q_stride=1538), dtype), call(folded(q_stride=1537), dtype), call(folded(kv_stride=1538), dtype),
               call(folded(new_k=None, new_v=None, q_stride=386), dtype),
               call(folded(kv_scale=X if dtype == BF16 else None, q_stride=6), dtype)]
        assert bad == [INVALID] * len(bad)
        assert b"multiples of 4" in lib.mt3_last_error()
        assert call(folded(q=X), dtype) == INVALID and b"both query forms" in lib.mt3_last_error()
        assert call(folded(q=X, new_k=None, new_v=None), dtype) == INVALID
    assert call(view(kv_scale=X), F32) == INVALID and b"fp8" in lib.mt3_last_error()
    assert call(folded(kv_scale=X), F32) == INVALID
    assert call(view(), 7) == INVALID and b"dtype" in lib.mt3_last_error()


def test_rejections_of_the_launcher():
    lib = _lib.load()
    for v in (view, folded):
        bad = [call(v(kcache=None)), call(v(vcache=None)), call(v(out=None)), call(v(B=0)), call(v(B=-1)), call(v(H=0)),
               call(v(H=-6)), call(v(cap=0)), call(v(cap=-64))]
        bad += [call(v(step=None, n_keys=n)) for n in (0, -1, 65)]
        bad += [call(v(step=None, n_keys=n, new_k=None, new_v=None)) for n in (0, 65)]
        bad += [call(v(new_v=None))]
        assert bad == [INVALID] * len(bad)
    assert call(view(q=None)) == INVALID                                # no query at all
    bad = [call(folded(q_ss_n=n)) for n in (0, -4, 2, 3, 6, 30, 66, 68, 128)] + [call(folded(q_ss=None))]
    assert bad == [INVALID] * len(bad)
    assert b"partial sums" in lib.mt3_last_error()
