"""The scripted token-rule drivers on a box without a GPU: exported, typed, and every argument error comes back as
MT3_ERR_INVALID before anything touches a device."""
import ctypes as C

from mt3_amd import _lib

X = C.c_void_p(0x1000)                         # a non-NULL pointer nobody dereferences: the calls are rejected first


def test_scripted_drivers_are_exported_and_reject_bad_calls():
    lib = _lib.load()
    for name in ("mt3_op_beam_search_scripted", "mt3_op_token_steps_scripted", "mt3_op_beam_reorder"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mt3_abi_version() == 4                                  # additive entry points
    forks, ran = C.c_int32(-1), C.c_int32(-1)

    def beam(logits=X, k=2, vocab=16, elems=1, steps=4, ids=X, trace=X, ss=None, n_ss=0, table=None, dim_e=0, max_len=0):
        return lib.mt3_op_beam_search_scripted(logits, ss, n_ss, 16 * n_ss, elems, k, vocab, steps, max_len, table, None,
                                               dim_e, ids, X, X, None, trace, X, C.byref(forks), C.byref(ran), None)

    bad = [beam(logits=None), beam(ids=None), beam(trace=None), beam(k=0), beam(k=9), beam(k=8, vocab=15),
           beam(vocab=3), beam(vocab=2049), beam(elems=0), beam(steps=0), beam(max_len=-1), beam(ss=X, n_ss=0),
           beam(ss=X, n_ss=65), beam(table=X, dim_e=32)]              # a table without its position table / output
    assert bad == [_lib.MT3_ERR_INVALID] * len(bad)
    assert b"mt3_op_beam_search_scripted" in lib.mt3_last_error()
    assert lib.mt3_op_beam_search_scripted(X, None, 0, 0, 1, 2, 16, 4, 0, None, None, 0, X, X, X, None, X, X, None,
                                           C.byref(ran), None) == _lib.MT3_ERR_INVALID
    assert (forks.value, ran.value) == (-1, -1)                        # nothing is reported for a rejected call

    def tok(logits=X, ids=X, done=X, rows=2, vocab=16, steps=4, mode=0, max_len=0, ss=None, n_ss=0):
        return lib.mt3_op_token_steps_scripted(logits, ss, n_ss, 16 * n_ss, rows, vocab, steps, mode, max_len, ids, done,
                                               None)

    bad = [tok(logits=None), tok(ids=None), tok(done=None), tok(rows=0), tok(vocab=1), tok(steps=0), tok(mode=2),
           tok(mode=-1), tok(max_len=-1), tok(ss=X, n_ss=0), tok(ss=X, n_ss=65)]
    assert bad == [_lib.MT3_ERR_INVALID] * len(bad)
    assert b"mt3_op_token_steps_scripted" in lib.mt3_last_error()

    two = (C.c_void_p * 2)(0x1000, 0x1000)
    hole = (C.c_void_p * 2)(0x1000, None)

    def reorder(n_layers=2, H=2, cap=8, esize=2, slots=4, k=two, v=two, fork=X, row=X, step=X, done=X):
        return lib.mt3_op_beam_reorder(n_layers, H, cap, esize, slots, k, v, None, fork, row, step, done, None)

    bad = [reorder(k=None), reorder(v=None), reorder(fork=None), reorder(row=None), reorder(step=None), reorder(done=None),
           reorder(n_layers=0), reorder(n_layers=17), reorder(H=0), reorder(cap=0), reorder(slots=0), reorder(esize=3),
           reorder(esize=8), reorder(k=hole), reorder(v=hole)]
    assert bad == [_lib.MT3_ERR_INVALID] * len(bad)
    assert b"beam_reorder" in lib.mt3_last_error()
