"""The preconditions the six job entry points share -- mt3_engine_decode, _decode_beams, _decode_forced, _transcribe,
_transcribe_beams, _transcribe_draws -- on a box without a GPU: one row per (entry point, precondition), each refused with
MT3_ERR_INVALID, the reporting function's name at the head of the message and the word that tells the check apart.

An engine cannot be finalized without a device.  The decodes and mt3_engine_transcribe check the engine's state FIRST, so
whatever else is wrong with a call they say "not finalized" here (a NULL engine included); mt3_engine_transcribe_beams and
mt3_engine_transcribe_draws check their arguments and the engine's shape first and its state last, so every argument error
of theirs is reachable.  mt3_engine_decode_forced checks its own buffer and then reports through mt3_engine_decode.  The
streaming calls leave h_stats alone, the decodes h_steps_run."""
import ctypes as C

import pytest

from mt3_amd import _lib

X, IDS = 1 << 20, 1 << 21                      # non-NULL pointers nobody dereferences: the calls are refused first
L = 1024
DECODE, BEAMS, FORCED = "mt3_engine_decode", "mt3_engine_decode_beams", "mt3_engine_decode_forced"
STREAM, STREAM_BEAMS, DRAWS = "mt3_engine_transcribe", "mt3_engine_transcribe_beams", "mt3_engine_transcribe_draws"


def _create(lib, **over):
    cfg = dict(vocab_size=1536, emb_dim=512, num_heads=6, head_dim=64, mlp_dim=1024, num_encoder_layers=8,
               num_decoder_layers=8, input_depth=512, input_length=256, max_decode_len=L, max_batch=16,
               compute_dtype=_lib.MT3_F32, decode_chains=1, kv_cache_dtype=0, dense_dtype=0, options=0)
    cfg.update(over)
    ec = _lib.EngineConfig(*[cfg[n] for n, _ in _lib.EngineConfig._fields_])
    h = C.c_void_p()
    assert lib.mt3_engine_create(C.byref(ec), C.byref(h)) == _lib.MT3_OK, lib.mt3_last_error()
    return h


def _call(lib, fn, h, st, ran, n=4, k=4, steps=8, flags=0, x=X, ids=IDS):
    """`fn` on engine `h` with good arguments unless told otherwise: n = batch / n_segments, k = num_beams / per,
    x = d_inputs / d_forced_ids"""
    if fn == DECODE:
        return lib.mt3_engine_decode(h, n, steps, flags, ids, None, C.byref(ran), None)
    if fn == BEAMS:
        return lib.mt3_engine_decode_beams(h, n, k, steps, flags, ids, None, None, C.byref(ran), None)
    if fn == FORCED:
        return lib.mt3_engine_decode_forced(h, n, steps, flags, x, None, ids, None)
    if fn == STREAM:
        return lib.mt3_engine_transcribe(h, x, n, steps, flags, ids, C.byref(st), None)
    if fn == STREAM_BEAMS:
        return lib.mt3_engine_transcribe_beams(h, x, n, k, steps, flags, ids, None, None, C.byref(st), None)
    assert fn == DRAWS
    return lib.mt3_engine_transcribe_draws(h, x, n, k, steps, flags, ids, C.byref(st), None)


# precondition -> (engine: None = a NULL handle, else the overrides of its configuration; the call's arguments)
CASES = {
    "null engine": (None, {}),
    "unknown flag": ({}, dict(flags=1 << 20)),
    "steps 0": ({}, dict(steps=0)),
    "steps L + 1": ({}, dict(steps=L + 1)),
    "null inputs": ({}, dict(x=None)),
    "null ids": ({}, dict(ids=None)),
    "n 0": ({}, dict(n=0)),
    "n -3": ({}, dict(n=-3)),
    "k 0": ({}, dict(k=0)),
    "k 9": ({}, dict(k=9)),
    "vocab < 2k": (dict(vocab_size=0), dict(k=4)),
    "17 layers": (dict(num_decoder_layers=17), {}),
    "not finalized": ({}, {}),
}
# what the two calls that check their arguments first say; k is `per` in the draws call (0 is refused, 9 is a fine count,
# and the vocabulary is no concern of the greedy path: those rows reach the engine's state)
ARGS_FIRST = {
    "null engine": b"null engine", "unknown flag": b"flags", "steps 0": b"num_steps", "steps L + 1": b"num_steps",
    "null inputs": b"null buffer", "null ids": b"null buffer", "n 0": b"no segments", "n -3": b"no segments",
    "k 0": b"num_beams must be 1 .. 8", "k 9": b"num_beams must be 1 .. 8", "vocab < 2k": b"2 * num_beams <= vocab",
    "17 layers": b"16 decoder layers", "not finalized": b"not finalized",
}
DRAWS_OWN = {"k 0": b"per must be at least 1", "k 9": b"not finalized", "vocab < 2k": b"not finalized"}


def _rows():
    for fn in (DECODE, BEAMS, FORCED, STREAM, STREAM_BEAMS, DRAWS):
        for case in CASES:
            who, word = fn, b"not finalized"                     # the engine's state comes first ...
            if fn == FORCED:
                who = DECODE                                     # ... reported by the body the two decodes share,
                if case == "null inputs":
                    who, word = FORCED, b"null forced ids"       # behind the forced call's own buffer
            elif fn in (STREAM_BEAMS, DRAWS):                    # ... or last
                word = DRAWS_OWN.get(case, ARGS_FIRST[case]) if fn == DRAWS else ARGS_FIRST[case]
            yield pytest.param(fn, case, who, word, id="%s-%s" % (fn[len("mt3_engine_"):], case.replace(" ", "_")))


@pytest.mark.parametrize("fn,case,who,word", list(_rows()))
def test_shared_precondition_is_refused_by_name(fn, case, who, word):
    lib = _lib.load()
    over, kw = CASES[case]
    h = None if over is None else _create(lib, **over)
    st = _lib.TranscribeStats()
    for name, _ in st._fields_[:9]:
        setattr(st, name, -7)
    ran = C.c_int32(-7)
    try:
        assert _call(lib, fn, h, st, ran, **kw) == _lib.MT3_ERR_INVALID
        msg = lib.mt3_last_error()
        assert msg.startswith(who.encode() + b": "), msg          # the exact name: no longer one begins with it
        assert word in msg, msg
        assert [getattr(st, name) for name, _ in st._fields_[:9]] == [-7] * 9 and ran.value == -7
    finally:
        if h is not None:
            lib.mt3_engine_destroy(h)
