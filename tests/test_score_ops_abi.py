"""The scoring path's kernel entry points (mt3_op_score_attention, mt3_op_score_embed, mt3_op_score_reduce,
mt3_op_planes, mt3_op_gemm_x6, mt3_op_encoder_attention_x6) on a box without a GPU: exported, typed, the view has the
layout of the C struct, and every rejection include/mt3_hip.h lists comes back as MT3_ERR_INVALID, with the entry point's
name in mt3_last_error(), before anything touches a device (the pointers are dummies nobody may dereference)."""
import ctypes as C

from mt3_amd import _lib

X = 0x1000                                     # a non-NULL, 16-byte aligned pointer nobody dereferences
INVALID = _lib.MT3_ERR_INVALID
BF16, F32 = _lib.MT3_BF16, _lib.MT3_F32
NAMES = ("mt3_op_score_attention", "mt3_op_score_embed", "mt3_op_score_reduce", "mt3_op_planes", "mt3_op_gemm_x6",
         "mt3_op_encoder_attention_x6")


def rejected(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    return rc == INVALID and name.encode() in lib.mt3_last_error()


def test_entry_points_are_exported_and_typed():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(lib, name).restype == C.c_int
    assert lib.mt3_abi_version() == 4                                  # additive entry points
    # LP64 layout of mt3_score_attn_view: the two int32 that follow a pointer are padded out by name
    V = _lib.ScoreAttnView
    assert C.sizeof(V) == 96
    assert {n: getattr(V, n).offset for n, _ in V._fields_} == dict(
        q=0, q_stride=8, reserved0=12, k=16, v=24, kv_stride=32, reserved1=36, kv_bstride=40, kv_hstride=48, key_tgt=56,
        out=64, out_stride=72, B=76, H=80, Lq=84, n_keys=88, causal=92)


# ------------------------------------------------------------------------------------------------------- attention
def self_view(**kw):
    """the causal self-attention launch of score_impl: B = 3 segments of 128 rows, H = 6"""
    f = dict(q=X, q_stride=1152, k=X + 768, v=X + 1536, kv_stride=1152, kv_bstride=128 * 1152, kv_hstride=64, key_tgt=X,
             out=X, out_stride=384, B=3, H=6, Lq=128, n_keys=128, causal=1)
    f.update(kw)
    return C.byref(_lib.ScoreAttnView(**f))


def cross_view(**kw):
    """the cross-attention launch against a cache [2][4][6][256][64]"""
    f = dict(q=X, q_stride=384, k=X, v=X + 4096, kv_stride=64, kv_bstride=6 * 256 * 64, kv_hstride=256 * 64, key_tgt=None,
             out=X, out_stride=384, B=3, H=6, Lq=128, n_keys=256, causal=0)
    f.update(kw)
    return C.byref(_lib.ScoreAttnView(**f))


def attn(v, dtype=BF16):
    return rejected("mt3_op_score_attention", dtype, v, None)


def test_score_attention_rejections_the_entry_point_adds():
    lib = _lib.load()
    assert attn(None) and b"null view" in lib.mt3_last_error()
    for dtype in (2, 7, -1):
        assert attn(self_view(), dtype) and b"dtype" in lib.mt3_last_error()
    assert attn(cross_view(key_tgt=X)) and b"key_tgt" in lib.mt3_last_error()
    for dtype, off in ((BF16, 4), (F32, 2)):                           # half of 16 bytes, in elements
        for view, field, value in ((self_view, "q_stride", 1152), (self_view, "kv_stride", 1152),
                                   (self_view, "kv_bstride", 128 * 1152), (self_view, "kv_hstride", 64),
                                   (cross_view, "kv_stride", 64), (cross_view, "kv_hstride", 256 * 64),
                                   (cross_view, "kv_bstride", 6 * 256 * 64)):
            assert attn(view(**{field: value + off}), dtype), (dtype, field)
            assert b"16 bytes" in lib.mt3_last_error()
        for field in ("q", "k", "v"):
            assert attn(self_view(**{field: X + 8}), dtype) and b"16 bytes" in lib.mt3_last_error()
    assert attn(self_view(q_stride=376)) and b"H * 64" in lib.mt3_last_error()
    assert attn(self_view(out_stride=383)) and attn(self_view(out_stride=0)) and attn(cross_view(kv_stride=56))
    assert attn(cross_view(kv_stride=0)) and attn(self_view(q_stride=-1152))


def test_score_attention_rejections_of_the_launcher():
    for dtype in (BF16, F32):
        for view in (self_view, cross_view):
            bad = [view(q=None), view(k=None), view(v=None), view(out=None), view(B=0), view(B=-3), view(H=0), view(H=-6),
                   view(Lq=0), view(Lq=-64), view(Lq=100), view(Lq=65)]
            assert all(attn(v, dtype) for v in bad), (dtype, view.__name__)
        assert all(attn(self_view(n_keys=n), dtype) for n in (0, 64, 192, 127))          # causal: n_keys == Lq
        assert all(attn(cross_view(n_keys=n), dtype) for n in (0, -64, 100, 255))        # cross: whole 64-key chunks


# -------------------------------------------------------------------------------------------------- embed, reduce
def embed(**kw):
    f = dict(table=X, pos=X, targets=X, dec_in=None, tgt_pad=X, y=X, rows=256, Lp=128, length=70, seg0=0, dim=512, vocab=37)
    f.update(kw)
    return rejected("mt3_op_score_embed", f["table"], f["pos"], f["targets"], f["dec_in"], f["tgt_pad"], f["y"], f["rows"],
                    f["Lp"], f["length"], f["seg0"], f["dim"], f["vocab"], None)


def reduce_(**kw):
    f = dict(logits=X, tgt_pad=X, weights=None, tok_pad=X, token_scores=None, seq_scores=X, rows=256, Lp=128, length=70,
             seg0=0, vocab=257, top1_ids=None, top1_scores=None)
    f.update(kw)
    return rejected("mt3_op_score_reduce", f["logits"], f["tgt_pad"], f["weights"], f["tok_pad"], f["token_scores"],
                    f["seq_scores"], f["rows"], f["Lp"], f["length"], f["seg0"], f["vocab"], f["top1_ids"], f["top1_scores"],
                    None)


CHUNKS = [dict(rows=0), dict(rows=-128), dict(rows=200), dict(rows=64), dict(Lp=0), dict(Lp=-128), dict(Lp=32, rows=64),
          dict(Lp=100, rows=200), dict(length=0), dict(length=-1), dict(length=129), dict(seg0=-1)]


def test_score_embed_rejections():
    assert all(embed(**c) for c in CHUNKS)
    bad = [dict(table=None), dict(pos=None), dict(targets=None), dict(tgt_pad=None), dict(y=None), dict(dim=0), dict(dim=-4),
           dict(dim=2), dict(dim=510), dict(vocab=0), dict(vocab=-5), dict(table=X + 4), dict(pos=X + 8), dict(y=X + 12)]
    assert all(embed(**c) for c in bad)
    assert embed(dec_in=X, dim=6)                                      # dec_in given changes nothing about the checks


def test_score_reduce_rejections():
    for top in (dict(), dict(top1_ids=X), dict(top1_scores=X), dict(top1_ids=X, top1_scores=X)):
        assert all(reduce_(**c, **top) for c in CHUNKS), top
        bad = [dict(logits=None), dict(tgt_pad=None), dict(tok_pad=None), dict(seq_scores=None), dict(vocab=0),
               dict(vocab=-3)]
        assert all(reduce_(**c, **top) for c in bad), top
    assert reduce_(vocab=1, top1_ids=X) and reduce_(vocab=1, top1_scores=X)          # an arg-max needs two candidates


# ------------------------------------------------------------------------------------------------ three-plane ops
def test_planes_rejections():
    bad = [(None, X, X, X, 8), (X, None, X, X, 8), (X, X, None, X, 8), (X, X, X, None, 8), (X, X, X, X, 0),
           (X, X, X, X, -1), (X, X, X, X, (1 << 39) + 1)]
    assert all(rejected("mt3_op_planes", *a, None) for a in bad)


def x6(**kw):
    f = dict(A=X, hi=X, mid=X, lo=X, norm=0, epi=_lib.EPI_RESID, out=X, M=130, N=512, K=512, aux=None, seq_len=0)
    f.update(kw)
    return rejected("mt3_op_gemm_x6", f["A"], f["hi"], f["mid"], f["lo"], f["norm"], f["epi"], f["out"], f["M"], f["N"],
                    f["K"], f["aux"], f["seq_len"], None)


def test_gemm_x6_rejections():
    bad = [dict(M=0), dict(M=-1), dict(N=0), dict(N=-128), dict(N=64), dict(N=200), dict(K=0), dict(K=32), dict(K=-64),
           dict(K=96), dict(A=None), dict(hi=None), dict(mid=None), dict(lo=None), dict(out=None),
           dict(M=1 << 21, K=512),                                     # A of 4 GB
           dict(N=1 << 21, K=1024)]                                    # a plane of 4 GB
    assert all(x6(**c) for c in bad)
    pos, heads = dict(epi=_lib.EPI_POS, aux=X, seq_len=65), dict(epi=_lib.EPI_HEADS, seq_len=65, N=768)
    assert x6(**dict(pos, aux=None)) and x6(**dict(pos, seq_len=0)) and x6(**dict(pos, seq_len=-1))
    assert x6(**dict(heads, seq_len=0)) and x6(**dict(heads, seq_len=-65)) and x6(**dict(heads, seq_len=64))   # 130 % 64
    # (norm, epilogue) pairs the kernel is not built for
    E = _lib
    pairs = [(0, E.EPI_STORE), (0, E.EPI_GEGLU), (1, E.EPI_RESID), (1, E.EPI_POS), (1, E.EPI_HEADS), (0, E.EPI_F32),
             (1, E.EPI_F32), (0, 6), (1, 9), (0, -1)]
    assert all(x6(norm=n, epi=e, aux=X, seq_len=65) for n, e in pairs)


def test_encoder_attention_x6_rejections():
    bad = [(None, X, 2, 256, 6), (X, None, 2, 256, 6), (X, X, 0, 256, 6), (X, X, -2, 512, 6), (X, X, 2, 256, 0),
           (X, X, 2, 256, -6), (X, X, 2, 0, 6), (X, X, 2, 128, 6), (X, X, 2, 384, 6), (X, X, 2, 1024, 6)]
    assert all(rejected("mt3_op_encoder_attention_x6", *a, None) for a in bad)
