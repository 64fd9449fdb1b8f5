"""mt3_op_gemm_decode on a box without a GPU: exported, typed, the view has the layout of the C struct, and every argument
error -- what the entry point adds and what launch_gemm / launch_typed / launch_cfg refuse for the engine too -- comes back
as MT3_ERR_INVALID before anything touches a device."""
import ctypes as C

from mt3_amd import _lib

X = 0x1000                                     # a non-NULL pointer nobody dereferences: the calls are rejected first
INVALID = _lib.MT3_ERR_INVALID
BF16, F32 = _lib.MT3_BF16, _lib.MT3_F32
HD, EMB = 384, 512


def view(**kw):
    """op 2 of the q-fold at the MT3 shape, complete: RESID over K = HD with the second product behind the emb columns;
    keywords override fields"""
    f = dict(A=X, Wt=X, out=X, M=4, N=EMB + HD, K=HD, lda=0, ldo=EMB, a_is_f32=0, norm=0, epilogue=_lib.EPI_RESID,
             a_ss=None, out_ct=None, out_ss=None, out2=X, n_split=EMB, ld2=4 * HD, concurrent=0, reserved=0)
    f.update(kw)
    return C.byref(_lib.GemmView(**f))


def plain(**kw):
    """op 0 without a fold: STORE of the normalised rows (norm 2)"""
    f = dict(out2=None, n_split=0, ld2=0, epilogue=_lib.EPI_STORE, norm=2, a_ss=X, N=3 * HD, K=EMB, ldo=3 * HD)
    f.update(kw)
    return view(**f)


def call(v, dtype=F32):
    return _lib.load().mt3_op_gemm_decode(dtype, v, None)


def test_entry_point_is_exported_and_typed():
    lib = _lib.load()
    name = "mt3_op_gemm_decode"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4                                  # an additive entry point
    # LP64 layout of mt3_gemm_view: 3 pointers, 8 int32, 4 pointers, 4 int32, no hidden padding
    assert C.sizeof(_lib.GemmView) == 104
    offs = {n: getattr(_lib.GemmView, n).offset for n, _ in _lib.GemmView._fields_}
    assert offs == dict(A=0, Wt=8, out=16, M=24, N=28, K=32, lda=36, ldo=40, a_is_f32=44, norm=48, epilogue=52, a_ss=56,
                        out_ct=64, out_ss=72, out2=80, n_split=88, ld2=92, concurrent=96, reserved=100)


def test_rejections_the_entry_point_adds():
    lib = _lib.load()
    assert lib.mt3_op_gemm_decode(F32, None, None) == INVALID and b"gemm_decode: null view" in lib.mt3_last_error()
    for dtype in (BF16, F32):
        # a second product with an epilogue that has none
        for epi in (_lib.EPI_F32, _lib.EPI_POS, _lib.EPI_HEADS):
            assert call(view(epilogue=epi), dtype) == INVALID and b"out2 needs" in lib.mt3_last_error()
        # a row stride of the side region below its width (STORE / RESID); negative for every epilogue
        bad = [call(view(ld2=HD - 1), dtype), call(view(ld2=1), dtype), call(view(ld2=-1), dtype),
               call(view(epilogue=_lib.EPI_STORE, norm=2, a_ss=X, N=4 * HD, K=EMB, n_split=3 * HD, ldo=3 * HD, ld2=HD - 32),
                    dtype),
               call(view(epilogue=_lib.EPI_GEGLU, norm=2, a_ss=X, N=2048 + 1536, K=EMB, n_split=2048, ldo=1024, ld2=-8),
                    dtype)]
        assert bad == [INVALID] * len(bad) and b"ld2" in lib.mt3_last_error()
        bad = [call(view(norm=3), dtype), call(view(norm=-1), dtype)]
        assert bad == [INVALID] * len(bad) and b"norm" in lib.mt3_last_error()
        bad = [call(view(epilogue=6), dtype), call(view(epilogue=7), dtype), call(view(epilogue=9), dtype),
               call(view(epilogue=-1), dtype), call(plain(epilogue=6), dtype)]        # the internal constants stay internal
        assert bad == [INVALID] * len(bad) and b"MT3_EPI_" in lib.mt3_last_error()
        bad = [call(view(lda=HD - 8), dtype), call(view(ldo=EMB - 1), dtype), call(view(ldo=0), dtype),
               call(plain(ldo=3 * HD - 1), dtype), call(plain(epilogue=_lib.EPI_GEGLU, N=2048, ldo=1023), dtype)]
        assert bad == [INVALID] * len(bad) and b"lda" in lib.mt3_last_error()
    # the by-products as mt3_op_gemm_ex takes them
    bad = [call(view(out_ct=X), BF16), call(view(out_ss=X), BF16), call(view(out_ct=X), F32), call(view(out_ct=X, out_ss=X), F32)]
    assert bad == [INVALID] * len(bad) and b"out_ct" in lib.mt3_last_error()


def test_rejections_of_the_launcher():
    lib = _lib.load()
    for dtype in (BF16, F32):
        for v in (view, plain):
            bad = [call(v(A=None), dtype), call(v(Wt=None), dtype), call(v(out=None), dtype), call(v(M=0), dtype),
                   call(v(M=-3), dtype), call(v(K=0), dtype)]
            assert bad == [INVALID] * len(bad) and b"bad shape or null pointer" in lib.mt3_last_error()
        bad = [call(view(n_split=0), dtype), call(view(n_split=EMB + HD, ldo=EMB + HD), dtype), call(view(n_split=EMB - 32, ldo=EMB - 32), dtype),
               call(view(n_split=-64, ldo=EMB), dtype)]
        assert bad == [INVALID] * len(bad) and b"split epilogue" in lib.mt3_last_error()
        # the GEGLU side product: whole 64-column tiles of weight rows, ld2 inside them
        g = dict(epilogue=_lib.EPI_GEGLU, norm=2, a_ss=X, K=EMB, n_split=2048, ldo=1024)
        bad = [call(view(N=2048 + 1536, ld2=1537, **g), dtype), call(view(N=2048 + 1568, ld2=1568, **g), dtype)]
        assert bad == [INVALID] * len(bad) and b"GEGLU side product" in lib.mt3_last_error()
        # no tile for the shape
        bad = [call(plain(N=3 * HD + 16, ldo=3 * HD + 16), dtype), call(view(K=HD + 8, lda=HD + 8), dtype)]
        assert bad == [INVALID] * len(bad) and b"multiple of the tile" in lib.mt3_last_error()
        # norm 2 / a_ss
        bad = [call(plain(a_ss=None), dtype), call(plain(a_is_f32=1), dtype), call(plain(K=1024), dtype),
               call(plain(epilogue=_lib.EPI_RESID), dtype)]
        assert bad == [INVALID] * len(bad)
        assert call(plain(norm=0), dtype) == INVALID and b"a_ss without norm 2" in lib.mt3_last_error()
        assert call(plain(norm=1, a_ss=None), dtype) == INVALID and b"f32 A operand" in lib.mt3_last_error()
        assert call(view(a_is_f32=1), dtype) == INVALID and b"unsupported" in lib.mt3_last_error()
        # epilogues whose extra arguments the view does not carry
        assert call(plain(epilogue=_lib.EPI_POS, norm=0, a_ss=None, a_is_f32=1), dtype) == INVALID
        assert b"POS" in lib.mt3_last_error()
        assert call(plain(epilogue=_lib.EPI_HEADS, norm=0, a_ss=None), dtype) == INVALID and b"HEADS" in lib.mt3_last_error()
    assert call(view(), 7) == INVALID and b"dtype" in lib.mt3_last_error()
