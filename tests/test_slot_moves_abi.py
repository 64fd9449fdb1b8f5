"""The slot-move drivers (mt3_op_embed_rows, mt3_op_slot_compact, mt3_op_slot_refill, mt3_op_beam_refill,
mt3_op_beam_stream_init) on a box without a GPU: exported, typed, and every argument error comes back as MT3_ERR_INVALID
before anything touches a device."""
import ctypes as C

from mt3_amd import _lib

X = 0x1000                                     # a non-NULL pointer nobody dereferences: the calls are rejected first
INVALID = _lib.MT3_ERR_INVALID


def row(**kw):
    """a complete split-form input row with its projection; keywords override fields"""
    f = dict(table=X, pos=X, max_pos=8, dim=32, y=X, y_ct=X, y_ss=X, ew=X, pw=X, q_out=X, q_n=8)
    f.update(kw)
    return C.byref(_lib.InputRowView(**f))


def state(**kw):
    f = dict(done=X, slot_row=X, slot_seg=X, step=X, cur_tok=X, n_done=X)
    f.update(kw)
    return C.byref(_lib.SlotStateView(**f))


TWO = (C.c_void_p * 2)(X, X)
HOLE = (C.c_void_p * 2)(X, None)


def cross(**kw):
    f = dict(n_layers=2, src_batch=4, src_entry0=1, dst_batch=8, row_bytes=32, sc_bytes=16, src=TWO, dst=TWO, src_sc=None,
             dst_sc=None)
    f.update(kw)
    return C.byref(_lib.StagedCrossView(**f))


def bad_cross(n_new):
    """staging chunks that cannot serve n_new segments"""
    return [None, cross(n_layers=0), cross(n_layers=17), cross(row_bytes=0), cross(row_bytes=24), cross(sc_bytes=8),
            cross(src_batch=0), cross(dst_batch=0), cross(src_entry0=-1), cross(src_entry0=4 - n_new + 1), cross(src=None),
            cross(dst=None), cross(src=HOLE), cross(dst=HOLE), cross(src_sc=TWO), cross(src_sc=HOLE, dst_sc=(C.c_void_p * 2)()),
            cross(src_sc=TWO, dst_sc=TWO, sc_bytes=0)]


def test_slot_move_drivers_are_exported_and_typed():
    lib = _lib.load()
    for name in ("mt3_op_embed_rows", "mt3_op_slot_compact", "mt3_op_slot_refill", "mt3_op_beam_refill",
                 "mt3_op_beam_stream_init"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4                                  # additive entry points
    # the views have the layout of the C structs (LP64: pointers 8-byte aligned, no hidden padding)
    assert C.sizeof(_lib.InputRowView) == 80 and C.sizeof(_lib.SlotStateView) == 48
    assert C.sizeof(_lib.StagedCrossView) == 64 and C.sizeof(_lib.BeamKView) == 72


def test_embed_rows_rejections():
    lib = _lib.load()

    def embed(in_=None, tok=X, t=X, rows=4):
        return lib.mt3_op_embed_rows(in_ if in_ is not None else row(), tok, t, rows, None)

    bad = [lib.mt3_op_embed_rows(None, X, X, 4, None), embed(tok=None), embed(t=None), embed(rows=0), embed(rows=-1),
           embed(rows=65537), embed(row(y=None)), embed(row(table=None)), embed(row(pos=None)), embed(row(max_pos=0)),
           embed(row(dim=0)), embed(row(dim=-16)), embed(row(dim=24)),               # the split form: dim % 16
           embed(row(dim=18, y_ct=None, y_ss=None)),                               # f32 only: dim % 4
           embed(row(y_ss=None)),                                                  # a bf16 copy without the sums
           embed(row(ew=None)), embed(row(pw=None)), embed(row(q_n=6)), embed(row(q_n=0)), embed(row(q_n=-4))]
    assert bad == [INVALID] * len(bad)
    assert b"embed" in lib.mt3_last_error()


def test_slot_compact_rejections():
    lib = _lib.load()

    def compact(st=None, in_=None, f=None, beam_rows=0, len_=None, rows=5):
        return lib.mt3_op_slot_compact(st if st is not None else state(), in_ if in_ is not None else row(), f, beam_rows,
                                       len_, rows, None, None)

    bad = [lib.mt3_op_slot_compact(None, row(), None, 0, None, 5, None, None),
           lib.mt3_op_slot_compact(state(), None, None, 0, None, 5, None, None),
           compact(state(done=None)), compact(state(slot_row=None)), compact(state(step=None)), compact(state(cur_tok=None)),
           compact(in_=row(y=None)), compact(rows=0), compact(rows=65537), compact(in_=row(dim=0)), compact(in_=row(dim=20)),
           compact(in_=row(q_n=6)), compact(in_=row(q_n=0)), compact(in_=row(y_ss=None)),
           compact(f=X, beam_rows=5), compact(f=X, beam_rows=4, len_=X), compact(len_=X)]
    assert bad == [INVALID] * len(bad)
    assert b"mt3_op_slot_compact" in lib.mt3_last_error()


def test_slot_refill_rejections():
    lib = _lib.load()

    def refill(st=None, in_=None, f=None, beam_rows=0, len_=None, len_row=None, ids=X, stride=16, out=X, rows=5, n_new=2,
               first_seg=0, x=0):
        return lib.mt3_op_slot_refill(st if st is not None else state(), in_ if in_ is not None else row(), f, beam_rows,
                                      len_, len_row, ids, stride, out, rows, n_new, first_seg, cross() if x == 0 else x,
                                      None, None)

    bad = [lib.mt3_op_slot_refill(None, row(), None, 0, None, None, X, 16, X, 5, 2, 0, cross(), None, None),
           lib.mt3_op_slot_refill(state(), None, None, 0, None, None, X, 16, X, 5, 2, 0, cross(), None, None)]
    bad += [refill(state(**{n: None})) for n in ("done", "slot_row", "slot_seg", "step", "cur_tok", "n_done")]
    bad += [refill(ids=None), refill(out=None), refill(rows=0), refill(rows=65537), refill(n_new=-1), refill(n_new=6),
            refill(stride=0), refill(first_seg=-1),
            refill(f=X, beam_rows=5, len_=X), refill(f=X, beam_rows=5, len_row=X), refill(f=X, beam_rows=4, len_=X, len_row=X),
            refill(len_=X), refill(len_row=X),
            refill(in_=row(y=None)), refill(in_=row(table=None)), refill(in_=row(pos=None)), refill(in_=row(max_pos=0)),
            refill(in_=row(dim=0)), refill(in_=row(dim=24)), refill(in_=row(dim=20, y_ct=None, y_ss=None)),
            refill(in_=row(y_ss=None)), refill(in_=row(ew=None)), refill(in_=row(pw=None)), refill(in_=row(q_n=6)),
            refill(in_=row(q_n=0))]
    bad += [refill(x=x) for x in bad_cross(2)]
    assert bad == [INVALID] * len(bad)
    assert b"mt3_op_slot_refill" in lib.mt3_last_error()


def test_beam_refill_rejections():
    lib = _lib.load()

    def beamk(**kw):
        f = dict(k=2, elems=3, vocab=2048, hist_stride=6, live=X, fin_score=X, fin_step=X, fin_beam=X, hist_par=X, hist_tok=X,
                 fork_src=X)
        f.update(kw)
        return C.byref(_lib.BeamKView(**f))

    def refill(b=None, st=None, in_=None, L=16, steps=16, out=X, n_new=2, first_seg=0, x=0):
        return lib.mt3_op_beam_refill(b if b is not None else beamk(), st if st is not None else state(),
                                      in_ if in_ is not None else row(), L, steps, out, None, None, n_new, first_seg,
                                      cross() if x == 0 else x, None, None)

    # what the issue names: vocab = 2049, k = 9, num_steps > L, (num_steps + L) * k * 2 > 65536
    named = [refill(beamk(vocab=2049)), refill(beamk(k=9, hist_stride=27)), refill(L=16, steps=17),
             refill(beamk(k=8, hist_stride=24), L=2049, steps=2048), refill(beamk(k=2, hist_stride=6), L=8193, steps=8192)]
    assert named == [INVALID] * len(named)
    assert b"64 KB" in lib.mt3_last_error()
    bad = [lib.mt3_op_beam_refill(None, state(), row(), 16, 16, X, None, None, 2, 0, cross(), None, None),
           lib.mt3_op_beam_refill(beamk(), None, row(), 16, 16, X, None, None, 2, 0, cross(), None, None),
           lib.mt3_op_beam_refill(beamk(), state(), None, 16, 16, X, None, None, 2, 0, cross(), None, None)]
    bad += [refill(beamk(**{n: None})) for n in ("live", "fin_score", "fin_step", "fin_beam", "hist_par", "hist_tok",
                                                  "fork_src")]
    bad += [refill(st=state(**{n: None})) for n in ("done", "slot_row", "slot_seg", "step", "cur_tok", "n_done")]
    bad += [refill(out=None), refill(beamk(k=0)), refill(beamk(vocab=0)), refill(beamk(elems=0)), refill(beamk(elems=8193)),
            refill(beamk(hist_stride=5)), refill(n_new=-1), refill(n_new=4), refill(first_seg=-1), refill(L=0, steps=0),
            refill(steps=0),
            refill(in_=row(y=None)), refill(in_=row(table=None)), refill(in_=row(pos=None)), refill(in_=row(max_pos=0)),
            refill(in_=row(dim=24)), refill(in_=row(dim=20, y_ct=None, y_ss=None)), refill(in_=row(y_ss=None)),
            refill(in_=row(ew=None)), refill(in_=row(pw=None)), refill(in_=row(q_n=6))]
    bad += [refill(x=x) for x in bad_cross(2)]
    assert bad == [INVALID] * len(bad)
    assert b"mt3_op_beam_refill" in lib.mt3_last_error()


def test_beam_stream_init_rejections():
    lib = _lib.load()
    gs = (C.c_int32 * 4)(1, 1, 1, 1)

    def init(done=X, seg=X, fork=X, srow=X, n_done=X, slots=4, groups=4, h=gs):
        return lib.mt3_op_beam_stream_init(done, seg, fork, srow, n_done, slots, groups, h, None)

    bad = [init(done=None), init(seg=None), init(fork=None), init(srow=None), init(n_done=None), init(h=None), init(slots=0),
           init(slots=65537), init(groups=0), init(groups=5)]
    assert bad == [INVALID] * len(bad)
    assert b"mt3_op_beam_stream_init" in lib.mt3_last_error()
