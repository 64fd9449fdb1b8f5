"""Constrained decoding on a box without a GPU: the new symbols are exported and typed, mt3_engine_set_token_masks
refuses every bad argument with its name in front before it looks at the device, mt3_codec_token_mask /
vocabularies.token_mask set exactly the bits computed here from mt3_codec_encode_event, and the command line parses
--programs / --no-drums.

An engine cannot be finalized without a device, so the argument checks come first and "not finalized" last (the order
mt3_engine_score_segments uses): every argument error is reachable here.  What needs masks that ARE set -- the status
round trip, "a decode is in flight", the decode / transcribe calls' own refusals -- is in
tests/test_gpu_token_mask_engine.py.  "Bits at or past vocab" cannot be set in an engine's mask (its vocabulary is a
multiple of 128, so the last word has no spare bits); the same host check serves the masked drivers, where
tests/test_gpu_token_mask_rules.py reaches it with vocab 70."""
import ctypes as C

import numpy as np
import pytest

from mt3_amd import _lib, event_codec, transcribe, vocabularies

NEW = ("mt3_engine_set_token_masks", "mt3_codec_token_mask", "mt3_op_token_steps_masked", "mt3_op_beam_search_masked")
VOCAB = 128                                               # an engine's vocabulary is a multiple of 128: 4 whole words
WORDS = 4
FULL = [0xFFFFFFFF] * 4


def test_the_symbols_are_exported_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4
    assert _lib.STATUS_TOKEN_MASKS == 12
    for old, new in (("mt3_op_token_steps_scripted", "mt3_op_token_steps_masked"),
                     ("mt3_op_beam_search_scripted", "mt3_op_beam_search_masked")):
        assert _lib.SIGNATURES[new][1][:-3] == _lib.SIGNATURES[old][1]          # the existing arguments, plus three


@pytest.fixture()
def engine():
    lib = _lib.load()
    ec = _lib.EngineConfig(VOCAB, 128, 2, 64, 128, 1, 1, 512, 256, 64, 4, _lib.MT3_F32, 0, 0, 0, 0)
    h = C.c_void_p()
    _lib.check(lib.mt3_engine_create(C.byref(ec), C.byref(h)))
    yield lib, h
    lib.mt3_engine_destroy(h)


def _set(lib, h, masks, seg):
    m = np.ascontiguousarray(masks, np.uint32).reshape(-1, WORDS) if masks is not None else None
    s = np.ascontiguousarray(seg, np.int32) if seg is not None else None
    return lib.mt3_engine_set_token_masks(h, m.ctypes.data if m is not None else None, 0 if m is None else m.shape[0],
                                          s.ctypes.data if s is not None else None, 0 if s is None else s.size)


def test_set_token_masks_refuses_bad_arguments_before_any_device_work(engine):
    lib, h = engine
    no_eos = [0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    one = [2, 0, 0, 0]
    cases = [
        ((FULL, FULL), None, b"several masks need a per-segment index"),
        (FULL, [0, 1], b"mask index outside [-1, n_masks)"),
        (FULL, [-2], b"mask index outside [-1, n_masks)"),
        (no_eos, None, b"a mask must allow EOS (id 1)"),
        ((FULL, no_eos), [0, 1, -1], b"a mask must allow EOS (id 1)"),
        (one, None, b"a mask must allow at least 2 tokens"),
        (FULL, None, b"engine not finalized"),             # nothing wrong with the arguments: the engine's state is next
        ((FULL, FULL), [1, -1, 0], b"engine not finalized"),
        (None, None, b"engine not finalized"),             # clearing needs a finalized engine too
    ]
    for masks, seg, msg in cases:
        assert _set(lib, h, masks, seg) == _lib.MT3_ERR_INVALID, msg
        assert lib.mt3_last_error() == b"mt3_engine_set_token_masks: " + msg
    m = np.array(FULL, np.uint32)
    assert lib.mt3_engine_set_token_masks(h, m.ctypes.data, -1, None, 0) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error() == b"mt3_engine_set_token_masks: n_masks must not be negative"
    assert lib.mt3_engine_set_token_masks(None, m.ctypes.data, 1, None, 0) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_engine_set_token_masks: ")
    assert lib.mt3_engine_status(h, _lib.STATUS_TOKEN_MASKS) == 0               # nothing was set


def test_masked_drivers_refuse_a_call_without_masks():
    lib = _lib.load()
    X = (C.c_float * 64)()
    p = C.cast(X, C.c_void_p)
    assert lib.mt3_op_token_steps_masked(p, None, 0, 0, 1, 8, 2, 0, 0, p, p, None, None, 1, None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_op_token_steps_masked: ")
    assert lib.mt3_op_token_steps_masked(p, None, 0, 0, 1, 8, 2, 0, 0, p, p, None, p, 0, None) == _lib.MT3_ERR_INVALID
    n = C.c_int32()
    assert lib.mt3_op_beam_search_masked(p, None, 0, 0, 1, 2, 16, 4, 0, None, None, 0, p, p, p, None, p, p, C.byref(n),
                                         C.byref(n), None, None, 1, None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_op_beam_search_masked: ")
    assert lib.mt3_op_beam_search_masked(p, None, 0, 0, 1, 9, 16, 4, 0, None, None, 0, p, p, p, None, p, p, C.byref(n),
                                         C.byref(n), None, p, 1, None) == _lib.MT3_ERR_INVALID
    assert b"k must be 1 .. 8" in lib.mt3_last_error()


# ------------------------------------------------------------------------------------------------ the codec helper
def _expected(codec, vocab, programs, drums):
    """the allowed ids, from mt3_codec_encode_event alone: token id = 3 + event index"""
    ok = np.ones(vocab, bool)
    lo, hi = next((r.min_value, r.max_value) for r in codec._event_ranges if r.type == "program")
    for p in range(lo, hi + 1):
        if programs is not None and p not in programs:
            ok[3 + codec.encode_event(event_codec.Event("program", p))] = False
    if not drums:
        lo, hi = next((r.min_value, r.max_value) for r in codec._event_ranges if r.type == "drum")
        for d in range(lo, hi + 1):
            ok[3 + codec.encode_event(event_codec.Event("drum", d))] = False
    return ok


def _bits(mask, vocab):
    return np.array([(int(mask[i >> 5]) >> (i & 31)) & 1 for i in range(((vocab + 31) // 32) * 32)], bool)


@pytest.mark.parametrize("vocab", (1536, 1500))           # a multiple of 32, and one that is not (tail bits 0)
def test_codec_token_mask_against_encode_event(vocab):
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    assert 3 + codec.num_classes <= vocab
    for programs, drums in (({0, 33}, False), (None, True), ({5}, True), (None, False), (set(), True)):
        mask = vocabularies.token_mask(codec, vocab, None if programs is None else sorted(programs), drums)
        assert mask.dtype == np.uint32 and mask.shape == ((vocab + 31) // 32,)
        bits = _bits(mask, vocab)
        assert np.array_equal(bits[:vocab], _expected(codec, vocab, programs, drums)), (programs, drums)
        assert not bits[vocab:].any()
        if programs is None and drums:
            assert bits[:vocab].all()                      # all programs, drums on: all ones up to vocab
        # the C call itself, not only the wrapper
        raw = np.zeros_like(mask)
        prog = np.array(sorted(programs), np.int32) if programs else None
        rc = _lib.load().mt3_codec_token_mask(C.byref(codec.desc), vocab, prog.ctypes.data if prog is not None else None,
                                              -1 if programs is None else len(programs), 1 if drums else 0,
                                              raw.ctypes.data)
        assert rc == _lib.MT3_OK and np.array_equal(raw, mask)
    off = np.flatnonzero(~_bits(vocabularies.token_mask(codec, vocab, [0, 33], False), vocab)[:vocab])
    assert len(off) == 126 + 128 and 1 not in off          # 126 programs and 128 drums forbidden, never EOS


def test_codec_token_mask_refusals():
    lib = _lib.load()
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    with pytest.raises(ValueError, match="program outside the codec's range"):
        vocabularies.token_mask(codec, 1536, [0, 128])
    with pytest.raises(ValueError, match="program outside the codec's range"):
        vocabularies.token_mask(codec, 1536, [-1])
    bare = event_codec.Codec(10, 100, [event_codec.EventRange("pitch", 21, 108)])
    with pytest.raises(ValueError, match="no program range"):
        vocabularies.token_mask(bare, 128, [0])
    assert _bits(vocabularies.token_mask(bare, 128), 128).all()                 # all programs: nothing to forbid
    out = np.zeros(4, np.uint32)
    assert lib.mt3_codec_token_mask(C.byref(codec.desc), 2, None, -1, 1, out.ctypes.data) == _lib.MT3_ERR_INVALID
    assert lib.mt3_codec_token_mask(C.byref(codec.desc), 128, None, -1, 1, None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_codec_token_mask: ")


# --------------------------------------------------------------------------------------------------- command line
def test_cli_plan_parses_programs_and_no_drums(tmp_path):
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--programs", "0,33", "--no-drums", str(wav)])
    assert args.programs == [0, 33] and args.drums is False
    args, _ = transcribe.plan(["--checkpoint", "random:0", str(wav)])
    assert args.programs is None and args.drums is True
    for bad in ("0,x", "128", ""):
        with pytest.raises(SystemExit):
            transcribe.plan(["--checkpoint", "random:0", "--programs", bad, str(wav)])
