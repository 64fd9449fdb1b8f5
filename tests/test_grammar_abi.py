"""mt3_engine_set_token_grammar, mt3_codec_token_grammar and the two grammar drivers without a GPU: every MT3_ERR_INVALID
include/mt3_hip.h lists comes back before any device work (on a box without a device anything later would be
MT3_ERR_HIP), and the status item exists."""
import ctypes as C

import pytest

from mt3_amd import _lib, note_sequences, vocabularies

V = 1536
GOOD = dict(shift_first=3, shift_count=1001, max_steps=204, tie_id=1134, program_first=1135, program_count=128,
            pitch_first=1004, pitch_count=128, with_ties=1)
BAD = [dict(shift_first=2), dict(tie_id=V), dict(pitch_first=V - 100), dict(program_count=0), dict(shift_count=-1),
       dict(pitch_first=1000),                         # overlaps the shifts
       dict(tie_id=1140),                              # inside the programs
       dict(program_first=1100),                       # overlaps the pitches (and the tie)
       dict(max_steps=0), dict(max_steps=1001), dict(max_steps=-5)]


def _g(**kw):
    return _lib.TokenGrammar(**{**GOOD, **kw})


def _engine():
    lib = _lib.load()
    cfg = _lib.EngineConfig(V, 512, 6, 64, 1024, 1, 1, 512, 256, 64, 2, _lib.MT3_F32, 1)
    h = C.c_void_p()
    assert lib.mt3_engine_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def test_status_item_and_signatures():
    assert _lib.STATUS_TOKEN_GRAMMAR == 14
    lib = _lib.load()
    for name in ("mt3_engine_set_token_grammar", "mt3_codec_token_grammar", "mt3_op_token_steps_grammar",
                 "mt3_op_beam_search_grammar", "mt3_token_grammar_initial", "mt3_token_grammar_advance",
                 "mt3_token_grammar_allowed"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(_lib.TokenGrammar) == 36
    assert len(_lib.SIGNATURES["mt3_op_token_steps_grammar"][1]) == len(_lib.SIGNATURES["mt3_op_token_steps_prompted"][1]) + 2
    assert len(_lib.SIGNATURES["mt3_op_beam_search_grammar"][1]) == len(_lib.SIGNATURES["mt3_op_beam_search_prompted"][1]) + 2


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_engine_refuses_a_bad_grammar(bad):
    lib, h = _engine()
    try:
        g = _g(**bad)
        assert lib.mt3_engine_set_token_grammar(h, C.byref(g)) == _lib.MT3_ERR_INVALID
        assert b"mt3_engine_set_token_grammar" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)


def test_engine_must_be_finalized_and_null_engine():
    lib, h = _engine()
    try:
        g = _g()
        assert lib.mt3_engine_set_token_grammar(h, C.byref(g)) == _lib.MT3_ERR_INVALID
        assert b"not finalized" in lib.mt3_last_error()
        assert lib.mt3_engine_set_token_grammar(h, None) == _lib.MT3_ERR_INVALID          # clearing needs a finalized engine too
        assert lib.mt3_engine_status(h, _lib.STATUS_TOKEN_GRAMMAR) == 0
        assert lib.mt3_engine_set_token_grammar(None, C.byref(g)) == _lib.MT3_ERR_INVALID
    finally:
        lib.mt3_engine_destroy(h)


def test_codec_builder_refusals():
    lib = _lib.load()
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    out = _lib.TokenGrammar()
    ties = note_sequences.NoteEncodingWithTiesSpec.spec_id
    call = lambda c, spec, vocab, steps, o: lib.mt3_codec_token_grammar(c, spec, vocab, steps, o)      # noqa: E731
    assert call(C.byref(codec.desc), ties, V, 204, C.byref(out)) == 0
    assert call(None, ties, V, 204, C.byref(out)) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), ties, V, 204, None) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), ties, V, 0, C.byref(out)) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), ties, V, codec.max_shift_steps + 1, C.byref(out)) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), ties, V, codec.max_shift_steps, C.byref(out)) == 0
    assert call(C.byref(codec.desc), ties, codec.num_classes + 2, 204, C.byref(out)) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), ties, codec.num_classes + 3, 204, C.byref(out)) == 0
    with pytest.raises(ValueError):
        vocabularies.token_grammar(codec, V, note_sequences.NoteEncodingSpec, 5000)


@pytest.mark.parametrize("bad", BAD[:4] + BAD[-2:], ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_drivers_refuse_a_bad_grammar_before_device_work(bad):
    lib = _lib.load()
    g = _g(**bad)
    fake = C.c_void_p(256)                              # never dereferenced: the refusal comes first
    ran, forks = C.c_int32(), C.c_int32()
    rc = lib.mt3_op_token_steps_grammar(fake, None, 0, 0, 3, V, 8, 0, 0, fake, fake, None, None, 0, None, None, 0, None,
                                        C.byref(g), None)
    assert rc == _lib.MT3_ERR_INVALID and b"mt3_op_token_steps_grammar" in lib.mt3_last_error()
    rc = lib.mt3_op_beam_search_grammar(fake, None, 0, 0, 3, 2, V, 8, 0, None, None, 0, fake, fake, fake, None, fake, fake,
                                        C.byref(forks), C.byref(ran), None, None, 0, None, None, 0, None, C.byref(g), None)
    assert rc == _lib.MT3_ERR_INVALID and b"mt3_op_beam_search_grammar" in lib.mt3_last_error()
