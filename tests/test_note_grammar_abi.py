"""mt3_engine_set_note_grammar, mt3_codec_note_grammar, the exported rule functions and the two notes drivers without a
GPU: the struct's layout, mt3_note_grammar_advance / _allowed against the Python automaton of tests/note_grammar_ref.py on
random states, and every MT3_ERR_INVALID include/mt3_hip.h lists, which comes back before any device work (on a box
without a device anything later would be MT3_ERR_HIP)."""
import ctypes as C

import numpy as np
import pytest

from mt3_amd import _lib, note_sequences, vocabularies
from tests import grammar_ref as gr
from tests import note_grammar_ref as nr

V = 1536
GOOD = dict(shift_first=3, shift_count=1001, max_steps=204, tie_id=1134, program_first=1135, program_count=128,
            pitch_first=1004, pitch_count=128, with_ties=1, velocity_first=1132, velocity_count=2, drum_first=1263,
            drum_count=128)
BAD = [dict(with_ties=0), dict(velocity_count=0), dict(velocity_first=2), dict(drum_first=V - 10),
       dict(velocity_first=1133),                       # its second id is the tie
       dict(drum_first=1200),                           # overlaps the programs
       dict(drum_first=1132, drum_count=1),             # overlaps the velocities
       dict(velocity_first=500),                        # inside the shifts
       dict(shift_first=2), dict(max_steps=0),          # what the token grammar refuses in `g`
       dict(pitch_first=1000, pitch_count=129, shift_count=990, max_steps=100),      # more than 128 pitches
       dict(program_count=129, drum_first=1300)]                                     # more than 128 programs


def _n(**kw):
    d = {**GOOD, **kw}
    return _lib.NoteGrammar(_lib.TokenGrammar(**{f: d[f] for f in gr.FIELDS}),
                            *[d[f] for f in nr.FIELDS[len(gr.FIELDS):]])


def _engine():
    lib = _lib.load()
    cfg = _lib.EngineConfig(V, 512, 6, 64, 1024, 1, 1, 512, 256, 64, 2, _lib.MT3_F32, 1)
    h = C.c_void_p()
    assert lib.mt3_engine_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def test_layout_status_item_and_signatures():
    assert _lib.STATUS_NOTE_GRAMMAR == 16
    assert C.sizeof(_lib.NoteGrammar) == 36 + 16 and _lib.NoteGrammar.g.offset == 0
    assert [_lib.NoteGrammar.velocity_first.offset, _lib.NoteGrammar.velocity_count.offset,
            _lib.NoteGrammar.drum_first.offset, _lib.NoteGrammar.drum_count.offset] == [36, 40, 44, 48]
    assert C.sizeof(_lib.TokenGrammar) == 36            # the token grammar did not grow
    lib = _lib.load()
    for name in ("mt3_engine_set_note_grammar", "mt3_codec_note_grammar", "mt3_op_token_steps_notes",
                 "mt3_op_beam_search_notes", "mt3_note_grammar_advance", "mt3_note_grammar_allowed",
                 "mt3_note_grammar_table_words", "mt3_note_grammar_check"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["mt3_op_token_steps_notes"][1]) == len(_lib.SIGNATURES["mt3_op_token_steps_sampled"][1]) + 2
    assert len(_lib.SIGNATURES["mt3_op_beam_search_notes"][1]) == len(_lib.SIGNATURES["mt3_op_beam_search_grammar"][1]) + 2
    assert lib.mt3_note_grammar_check(C.byref(_n()), V) == 0
    assert lib.mt3_note_grammar_table_words(C.byref(_n())) == 128 * 4
    assert lib.mt3_note_grammar_table_words(C.byref(_n(pitch_count=40, program_count=3))) == 3 * 2


@pytest.mark.parametrize("dims", [(3, 40), (128, 128), (5, 32), (7, 33)], ids=lambda d: "%dx%d" % d)
def test_exported_rule_equals_the_python_automaton(dims):
    """random walks: at every state mt3_note_grammar_allowed over the whole vocabulary equals the Python automaton's
    vector, and mt3_note_grammar_advance (with mt3_token_grammar_advance for the packed int) leaves the Python automaton's
    state, table word for table word"""
    lib = _lib.load()
    programs, pitches = dims
    d = dict(shift_first=3, shift_count=20, max_steps=15, pitch_first=23, pitch_count=pitches, velocity_first=23 + pitches,
             velocity_count=2, tie_id=25 + pitches, program_first=26 + pitches, program_count=programs,
             drum_first=26 + pitches + programs, drum_count=5, with_ties=1)
    vocab = d["drum_first"] + 5 + 4
    n_py = nr.note_grammar(**d)
    n_c = _lib.NoteGrammar(_lib.TokenGrammar(**{f: d[f] for f in gr.FIELDS}), *[d[f] for f in nr.FIELDS[len(gr.FIELDS):]])
    assert lib.mt3_note_grammar_check(C.byref(n_c), vocab) == 0
    words = nr.table_words(n_py)
    assert lib.mt3_note_grammar_table_words(C.byref(n_c)) == words
    rng = np.random.default_rng(programs * 1000 + pitches)
    for walk in range(6):
        state = nr.initial(n_py)
        gram, note, held = gr.as_i32(nr.split(state)[0]), 0, np.zeros(words, np.uint32)
        for step in range(120):
            want = nr.allowed_vector(n_py, state, vocab)
            got = np.array([lib.mt3_note_grammar_allowed(C.byref(n_c), gram, note, held.ctypes.data, i)
                            for i in range(vocab)], bool)
            assert np.array_equal(got, want), (walk, step, np.nonzero(got != want)[0])
            # mostly allowed tokens, now and then any token at all (a prompt may force it)
            pool = np.nonzero(want)[0] if rng.random() < 0.8 else np.arange(2, vocab)
            pool = pool[pool != 1]
            focus = [i for i in pool if d["pitch_first"] <= i < d["program_first"] + programs]      # pitch .. program ids
            tok = int(rng.choice(focus if focus and rng.random() < 0.85 else pool))
            note = lib.mt3_note_grammar_advance(C.byref(n_c), gram, note, held.ctypes.data, tok)
            gram = lib.mt3_token_grammar_advance(C.byref(n_c.g), gram, tok)
            state = nr.advance(n_py, state, tok)
            g_py, note_py, _ = nr.split(state)
            assert (gram & 0xFFFFFFFF) == g_py and (note & 0xFFFFFFFF) == note_py, (walk, step, tok)
            assert np.array_equal(held, nr.held_words(n_py, state)), (walk, step, tok)
        assert nr.held_pairs(n_py, state) or walk                 # the walks do hold notes


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_engine_and_check_refuse_a_bad_note_grammar(bad):
    lib, h = _engine()
    try:
        n = _n(**bad)
        assert lib.mt3_note_grammar_check(C.byref(n), V) == _lib.MT3_ERR_INVALID
        assert lib.mt3_engine_set_note_grammar(h, C.byref(n)) == _lib.MT3_ERR_INVALID
        assert b"mt3_engine_set_note_grammar" in lib.mt3_last_error() and b"not finalized" not in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)


def test_engine_must_be_finalized_and_null_engine():
    lib, h = _engine()
    try:
        n = _n()
        assert lib.mt3_engine_set_note_grammar(h, C.byref(n)) == _lib.MT3_ERR_INVALID
        assert b"not finalized" in lib.mt3_last_error()
        assert lib.mt3_engine_set_note_grammar(h, None) == _lib.MT3_ERR_INVALID          # clearing needs a finalized engine too
        assert lib.mt3_engine_status(h, _lib.STATUS_NOTE_GRAMMAR) == 0
        assert lib.mt3_engine_set_note_grammar(None, C.byref(n)) == _lib.MT3_ERR_INVALID
    finally:
        lib.mt3_engine_destroy(h)


def test_codec_builder():
    lib = _lib.load()
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    out = _lib.NoteGrammar()
    ties, no_ties = note_sequences.NoteEncodingWithTiesSpec.spec_id, note_sequences.NoteEncodingSpec.spec_id
    call = lambda c, spec, vocab, steps, o: lib.mt3_codec_note_grammar(c, spec, vocab, steps, o)      # noqa: E731
    assert call(C.byref(codec.desc), ties, V, 204, C.byref(out)) == 0
    token = vocabularies.token_grammar(codec, V, ties, 204)
    assert bytes(out.g) == bytes(token)                 # its `g` member is the token grammar of the same codec
    assert out.velocity_count == 2 and out.drum_count == 128 and out.g.pitch_count <= 128 and out.g.program_count == 128
    assert lib.mt3_note_grammar_check(C.byref(out), V) == 0
    lo, hi = codec.event_type_range("velocity")          # event indices; token id = 3 + index
    assert (out.velocity_first, out.velocity_count) == (3 + lo, hi - lo + 1)
    lo, hi = codec.event_type_range("drum")
    assert (out.drum_first, out.drum_count) == (3 + lo, hi - lo + 1)
    assert call(None, ties, V, 204, C.byref(out)) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), ties, V, 204, None) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), ties, V, 0, C.byref(out)) == _lib.MT3_ERR_INVALID
    assert call(C.byref(codec.desc), no_ties, V, 204, C.byref(out)) == _lib.MT3_ERR_INVALID    # no tie section
    assert b"tie section" in lib.mt3_last_error()
    with pytest.raises(ValueError):
        vocabularies.note_grammar(codec, V, note_sequences.NoteEncodingSpec, 204)
    n = vocabularies.note_grammar(codec, V, note_sequences.NoteEncodingWithTiesSpec, 204)
    assert n.g.max_steps == 204 and lib.mt3_note_grammar_check(C.byref(n), V) == 0


@pytest.mark.parametrize("bad", BAD[:3] + BAD[-4:-2], ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_drivers_refuse_a_bad_note_grammar_before_device_work(bad):
    lib = _lib.load()
    n = _n(**bad)
    fake = C.c_void_p(256)                              # never dereferenced: the refusal comes first
    ran, forks = C.c_int32(), C.c_int32()
    rc = lib.mt3_op_token_steps_notes(fake, None, 0, 0, 3, V, 8, 0, 0, fake, fake, None, None, 0, None, None, 0, None,
                                      C.byref(n), None, None, None, None, None)
    assert rc == _lib.MT3_ERR_INVALID and b"mt3_op_token_steps_notes" in lib.mt3_last_error()
    rc = lib.mt3_op_beam_search_notes(fake, None, 0, 0, 3, 2, V, 8, 0, None, None, 0, fake, fake, fake, None, fake, fake,
                                      C.byref(forks), C.byref(ran), None, None, 0, None, None, 0, None, C.byref(n), None,
                                      None, None)
    assert rc == _lib.MT3_ERR_INVALID and b"mt3_op_beam_search_notes" in lib.mt3_last_error()
