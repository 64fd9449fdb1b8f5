"""mt3_engine_set_sampling_seeds, mt3_engine_transcribe_draws, mt3_op_token_steps_seeded and mt3_op_slot_refill_draws on a
box without a GPU: exported, typed, declared in the header, and the argument errors that need no device come back as
MT3_ERR_INVALID with the function's name before anything is written.  (What needs a finalized engine -- a decode in flight,
a table shorter than the job, sampling not set -- is in tests/test_gpu_draws_engine.py.)"""
import ctypes as C
import os

import numpy as np

from mt3_amd import _lib, sampling

X = 0x1000                                     # a non-NULL pointer nobody dereferences: the calls are rejected first
INVALID = _lib.MT3_ERR_INVALID
NEW = ("mt3_engine_set_sampling_seeds", "mt3_engine_transcribe_draws", "mt3_op_token_steps_seeded",
       "mt3_op_slot_refill_draws")


def _create(lib, **over):
    cfg = dict(vocab_size=1536, emb_dim=512, num_heads=6, head_dim=64, mlp_dim=1024, num_encoder_layers=8,
               num_decoder_layers=8, input_depth=512, input_length=256, max_decode_len=1024, max_batch=16,
               compute_dtype=_lib.MT3_F32, decode_chains=1, kv_cache_dtype=0, dense_dtype=0, options=0)
    cfg.update(over)
    ec = _lib.EngineConfig(*[cfg[n] for n, _ in _lib.EngineConfig._fields_])
    h = C.c_void_p()
    assert lib.mt3_engine_create(C.byref(ec), C.byref(h)) == _lib.MT3_OK, lib.mt3_last_error()
    return h


def test_symbols_are_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "mt3_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert "int %s(" % name in header
    sig = _lib.SIGNATURES
    assert sig["mt3_engine_set_sampling_seeds"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32])
    res, args = sig["mt3_engine_transcribe_draws"]
    assert res is C.c_int and len(args) == 9 and args[7] == C.POINTER(_lib.TranscribeStats)
    assert args[:7] == [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]
    # the scripted drivers: their neighbours' arguments plus one
    assert sig["mt3_op_token_steps_seeded"][1] == sig["mt3_op_token_steps_notes"][1] + [C.c_void_p]
    refill = sig["mt3_op_slot_refill"][1]
    assert sig["mt3_op_slot_refill_draws"][1] == refill[:13] + [C.c_int32] + refill[13:]
    assert C.sizeof(_lib.StagedCrossView) == 64                        # the view keeps its layout
    assert lib.mt3_abi_version() == 4                                  # additive entry points


def test_set_sampling_seeds_refusals_that_need_no_device():
    lib = _lib.load()
    seeds = (C.c_uint64 * 4)(9, 1 << 40, (1 << 64) - 1, 5)
    assert lib.mt3_engine_set_sampling_seeds(None, seeds, 4) == INVALID
    assert b"mt3_engine_set_sampling_seeds" in lib.mt3_last_error()
    h = _create(lib)
    try:
        for n in (0, -1):
            assert lib.mt3_engine_set_sampling_seeds(h, seeds, n) == INVALID
            assert b"mt3_engine_set_sampling_seeds: n_segments" in lib.mt3_last_error()
        # in range: the check that needs a device-side engine; clearing needs a finalized engine too
        for args in ((seeds, 4), (None, 0)):
            assert lib.mt3_engine_set_sampling_seeds(h, *args) == INVALID
            assert b"mt3_engine_set_sampling_seeds: engine not finalized" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)


def _draws_rejected(lib, h, n_segments=4, per=3, steps=8, flags=0, x=1 << 20, ids=1 << 21):
    st = _lib.TranscribeStats()
    st.slots = st.refills = -7
    rc = lib.mt3_engine_transcribe_draws(h, x, n_segments, per, steps, flags, ids, C.byref(st), None)
    return rc == INVALID and b"mt3_engine_transcribe_draws" in lib.mt3_last_error() and st.slots == -7 and st.refills == -7


def test_transcribe_draws_refusals_that_need_no_device():
    lib = _lib.load()
    assert _draws_rejected(lib, None)
    h = _create(lib)
    try:
        for flags in (_lib.DECODE_BEAM1, _lib.DECODE_EARLY_EXIT, _lib.DECODE_ASYNC, 1 << 8, 1 << 20):
            assert _draws_rejected(lib, h, flags=flags), flags
            assert b"flags" in lib.mt3_last_error()
        for per in (0, -1):
            assert _draws_rejected(lib, h, per=per), per
            assert b"per must be at least 1" in lib.mt3_last_error()
        L = 1024
        for n, per in (((1 << 31) // L, 1), (1 << 20, 2), (3, (1 << 31) // 3), ((1 << 31) - 1, (1 << 31) - 1)):
            assert _draws_rejected(lib, h, n_segments=n, per=per), (n, per)           # n * per * L past INT32_MAX
            assert b"INT32_MAX" in lib.mt3_last_error()
        assert _draws_rejected(lib, h, x=None) and _draws_rejected(lib, h, ids=None)
        for n in (0, -3):
            assert _draws_rejected(lib, h, n_segments=n), n
        for steps in (0, -1, 1025):
            assert _draws_rejected(lib, h, steps=steps), steps
        # arguments in range (the largest job there is, too) reach the check that needs a device-side engine
        for kw in (dict(flags=_lib.DECODE_NO_GRAPH | _lib.DECODE_SINGLE_STREAM), dict(n_segments=((1 << 31) - 1) // L, per=1)):
            assert _draws_rejected(lib, h, **kw)
            assert b"not finalized" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)
    h = _create(lib, num_decoder_layers=17)
    try:
        assert _draws_rejected(lib, h) and b"16 decoder layers" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)


def test_seeded_driver_checks_as_the_notes_driver_does():
    lib = _lib.load()
    good = _lib.Sampling(0.8, 0, 0.9, 3)
    fake = C.c_void_p(256)
    seeds = (C.c_uint64 * 3)(1, 2, 3)

    def call(vocab=300, mode=0, sp=good, rows=3):
        return lib.mt3_op_token_steps_seeded(fake, None, 0, 0, rows, vocab, 8, mode, 0, fake, fake, None, None, 0, None,
                                             None, 0, None, None, None, C.byref(sp), None, None, None, seeds)

    for kw, word in ((dict(vocab=2049), b"2048"), (dict(mode=1), b"beam-1"), (dict(rows=0), b"rows"),
                     (dict(sp=_lib.Sampling(0.0, 0, 0.0, 1)), b"temperature")):
        assert call(**kw) == INVALID
        assert b"mt3_op_token_steps_seeded" in lib.mt3_last_error() and word in lib.mt3_last_error(), kw
    assert lib.mt3_op_token_steps_seeded(None, None, 0, 0, 3, 300, 8, 0, 0, fake, fake, None, None, 0, None, None, 0, None,
                                         None, None, None, None, None, None, seeds) == INVALID


def test_refill_draws_rejections():
    lib = _lib.load()
    two = (C.c_void_p * 2)(X, X)
    row = C.byref(_lib.InputRowView(table=X, pos=X, max_pos=8, dim=32, y=X, y_ct=X, y_ss=X, ew=X, pw=X, q_out=X, q_n=8))
    st = C.byref(_lib.SlotStateView(done=X, slot_row=X, slot_seg=X, step=X, cur_tok=X, n_done=X))

    def cross(**kw):
        f = dict(n_layers=2, src_batch=3, src_entry0=2, dst_batch=8, row_bytes=32, sc_bytes=16, src=two, dst=two,
                 src_sc=None, dst_sc=None)
        f.update(kw)
        return C.byref(_lib.StagedCrossView(**f))

    def refill(per=3, n_new=5, rows=8, x=None, state=st):
        return lib.mt3_op_slot_refill_draws(state, row, None, 0, None, None, X, 16, X, rows, n_new, 0,
                                            x if x is not None else cross(), per, None, None)

    bad = [refill(per=0), refill(per=-2),
           refill(x=cross(src_entry0=5)),               # draws 5 .. 9 of a chunk that holds 3 * 3 = 9
           refill(per=1),                               # per = 1: entries 2 .. 6 of 3
           refill(per=2, x=cross(src_entry0=2)),        # 2 + 5 > 3 * 2
           refill(x=cross(src_batch=1 << 30)),          # src_batch * per past INT32_MAX
           refill(n_new=9), refill(rows=0), refill(state=None), refill(x=cross(row_bytes=24))]
    assert bad == [INVALID] * len(bad)
    assert b"mt3_op_slot_refill_draws" in lib.mt3_last_error()


def test_numpy_rule_takes_a_seed_per_row():
    """sampling.pick(seed=k) is the pick under params.seed = k, and without it the pick it always was"""
    rng = np.random.default_rng(3)
    x = rng.normal(size=300).astype(np.float32) * 2
    p = sampling.SamplingParams(0.9, 0, 0.0, seed=11)
    picks = set()
    for k in (0, 11, 1 << 32, (1 << 64) - 1, (1 << 40) + 7):
        q = sampling.SamplingParams(0.9, 0, 0.0, seed=k)
        for t in range(4):
            got, m = sampling.pick(x, t, 5, p, seed=k)
            want, mw = sampling.pick(x, t, 5, q)
            assert got == want and m["pick"] == mw["pick"]
            picks.add((t, got))
    assert sampling.pick(x, 2, 5, p)[0] == sampling.pick(x, 2, 5, p, seed=11)[0]
    assert len(picks) > 8                                   # different seeds do draw differently
