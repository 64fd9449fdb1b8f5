"""The event-grammar reference (tests/grammar_ref.py) and the scripted cases (tests/grammar_script.py) without a GPU: the
automaton against the library's own rule functions, the references against prompt_ref where there is no grammar, what the
references emit against `accepts`, the caps of the scripted cases, the codec builder, and the link to the host note
decoder (mt3_notes_decode)."""
import ctypes as C

import numpy as np
import pytest

from mt3_amd import _lib, metrics_utils, note_sequences, vocabularies
from tests import beam_script as bs
from tests import grammar_ref as gr
from tests import grammar_script as gs
from tests import prompt_ref as pr
from tests.beam_search_ref import EOS

ALL = gs.beam_cases() + gs.token_cases()


def _struct(g):
    return _lib.TokenGrammar(*[getattr(g, f) for f in gr.FIELDS])


def test_python_rule_is_the_library_rule():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    for ties in (0, 1):
        g = gs.toy_grammar(ties)
        s = _struct(g)
        assert lib.mt3_token_grammar_initial(C.byref(s)) == gr.as_i32(gr.initial(g))
        for _ in range(400):
            state = int(rng.integers(0, 2)) << 31 | int(rng.integers(0, 2)) << 30 | int(rng.integers(0, 40))
            tok = int(rng.integers(0, 70))
            assert lib.mt3_token_grammar_advance(C.byref(s), gr.as_i32(state), tok) == gr.as_i32(gr.advance(g, state, tok))
            assert bool(lib.mt3_token_grammar_allowed(C.byref(s), gr.as_i32(state), tok)) == gr.allowed(g, state, tok)
    # two shifts in a row saturate at 2^29
    big = gr.PREV_SHIFT | ((1 << 29) - 3)
    assert gr.advance(g, big, gs.SHIFT0 + 9) & gr.TIME == 1 << 29
    assert lib.mt3_token_grammar_advance(C.byref(s), gr.as_i32(big), gs.SHIFT0 + 9) == gr.as_i32(gr.PREV_SHIFT | 1 << 29)


def test_without_a_grammar_the_references_are_prompt_ref():
    for case in pr.token_prompt_cases():
        ids, done, _ = gr.greedy(case.logits, case.prompts, None, None, case.max_len)
        want_ids, want_done = pr.greedy(case.logits, case.prompts, case.max_len)
        assert np.array_equal(ids, want_ids) and np.array_equal(done, want_done)
    for case in pr.beam_prompt_cases():
        a = gr.run_reference(case, None, [np.ones(case.V, bool)] * case.elems)     # the ruled path, nothing ruled out
        b = pr.run_reference(case)
        assert np.array_equal(a.decodes, b.decodes) and np.array_equal(a.scores, b.scores) and a.steps_run == b.steps_run
        assert all(np.array_equal(x, y) for x, y in zip(a.live_lp, b.live_lp))
        assert all(np.array_equal(x, y) for x, y in zip(a.index, b.index))


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_cases_are_separated_and_bite(case):
    assert case.max_tries <= bs.MAX_TRIES and all(d >= bs.GAP(s) for d, s, _ in case.gaps)
    broken = case.broken_rows()
    assert broken.any(), case.name                     # the unconstrained reference breaks the grammar in every case
    assert 2 * broken.sum() >= case.elems, case.name   # ... on at least half of its rows


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_what_the_references_emit_is_accepted(case):
    g, ref = case.g, case.ref
    rows = [(b, d) for b in range(case.elems) for d in ref.decodes[b]]
    if case.k == 1:
        ids, done, states = gr.greedy(case.logits if case.ss is None else np.stack([case.scaled(t) for t in range(case.num_steps)]),
                                      case.prompts, g, case.masks, case.max_len)
        rows += [(b, ids[b]) for b in range(case.elems)]
        for b in range(case.elems):                    # the greedy states are the replay of its ids
            n = int(np.argmax(done[:, b])) + 1 if done[:, b].any() else case.num_steps
            assert list(states[:n, b]) == gr.replay(g, ids[b])[:n]
    for b, row in rows:
        assert gr.accepts(g, row, case.plen(b)), (case.name, b, list(row))
        # the free picks never repeat a shift and never go back in time
        t_now, prev, section = 0, False, bool(g.with_ties)
        used = int(np.max(np.nonzero(row)[0])) + 1 if np.any(row) else 0
        for t, tok in enumerate(int(x) for x in row[:used]):
            shift = g.shift_first <= tok < g.shift_first + g.shift_count
            if t >= case.plen(b) and shift:
                assert not prev and tok - g.shift_first >= t_now and tok - g.shift_first <= g.max_steps and not section
            if t >= case.plen(b) and tok == g.tie_id:
                assert section
            t_now = (t_now + tok - g.shift_first if prev else tok - g.shift_first) if shift else t_now
            prev, section = shift, section and tok != g.tie_id
            if tok == EOS:
                break
        if case.masks is not None and case.masks[b] is not None:
            free = [int(x) for x in row[case.plen(b):used]]
            assert all(case.masks[b][x] for x in free)


def test_prompts_advance_the_state():
    g = gs.toy_grammar(1)
    assert gr.replay(g, gs.PROMPT_TIE)[-1] == 0                                   # behind the section, t = 0, no shift
    assert gr.replay(g, gs.PROMPT_SECTION)[-1] == gr.PREV_SHIFT | 4
    two = [gs.TIE, gs.SHIFT0 + 4, gs.SHIFT0 + 7]                                   # two forced shifts in a row add up
    assert gr.replay(g, two)[-1] == gr.PREV_SHIFT | 11
    logits = np.zeros((6, 1, 70), np.float32)
    logits[:, 0, gs.SHIFT0 + 2] = 5.0                                              # the model wants shift 2 at every step
    logits[:, 0, gs.PITCH0] = 1.0
    ids, _, states = gr.greedy(logits, [two], g)
    assert list(ids[0, :3]) == two and ids[0, 3] == gs.PITCH0                      # no third shift, and 2 < 11 anyway
    assert states[2, 0] == gr.PREV_SHIFT | 11 and states[3, 0] == 11
    assert ids[0, 4] == gs.PITCH0                                                  # shift 2 would run backwards: never again


CODECS = {"mt3": (vocabularies.VocabularyConfig(num_velocity_bins=1), 256, 204),
          "ismir2021": (vocabularies.VocabularyConfig(num_velocity_bins=127), 512, 409)}


@pytest.mark.parametrize("model", sorted(CODECS))
@pytest.mark.parametrize("spec", (note_sequences.NoteEncodingWithTiesSpec, note_sequences.NoteEncodingSpec),
                         ids=("ties", "notes"))
def test_codec_builder_agrees_with_the_python_codec(model, spec):
    cfg, frames, want_steps = CODECS[model]
    codec = vocabularies.build_codec(cfg)
    max_steps = int(np.floor(frames * 128 / 16000 * codec.steps_per_second))
    assert max_steps == want_steps
    vocab = vocabularies.num_embeddings(vocabularies.vocabulary_from_codec(codec))
    g = vocabularies.token_grammar(codec, vocab, spec, max_steps)
    for name, first, count in (("shift", g.shift_first, g.shift_count), ("pitch", g.pitch_first, g.pitch_count),
                               ("program", g.program_first, g.program_count), ("tie", g.tie_id, 1)):
        lo, hi = codec.event_type_range(name)
        assert (first, count) == (lo + 3, hi - lo + 1), name
    assert g.max_steps == max_steps and g.with_ties == int(spec is note_sequences.NoteEncodingWithTiesSpec)


def test_accepted_rows_lose_nothing_in_the_note_decoder():
    """rows built to hold exactly one fault of a kind the grammar forbids, and their repaired twins, through
    mt3_notes_decode with the real codec: the fault is counted (invalid / dropped), the twin -- accepted by `accepts` --
    gives dropped_events == 0 and no invalid event"""
    cfg, frames, max_steps = CODECS["mt3"]
    codec = vocabularies.build_codec(cfg)
    spec = note_sequences.NoteEncodingWithTiesSpec
    g = gr.from_struct(vocabularies.token_grammar(codec, 1536, spec, max_steps))
    E = vocabularies.event_codec.Event
    ev = lambda t, v: codec.encode_event(E(t, v)) + 3                              # noqa: E731
    on = [ev("program", 0), ev("velocity", 1), ev("pitch", 60)]
    off = [ev("program", 0), ev("velocity", 0), ev("pitch", 60)]
    good = [ev("tie", 0), ev("shift", 10)] + on + [ev("shift", 50)] + off + [EOS]

    def decode(row):
        toks = np.array(row[:row.index(EOS)], np.int32) - 3
        _, inv, drop = metrics_utils._run(codec, spec.spec_id, [toks], [0.0], [frames * 128 / 16000])
        return inv, drop

    assert gr.accepts(g, good) and decode(good) == (0, 0)
    back = [ev("tie", 0), ev("shift", 50)] + on + [ev("shift", 10)] + off + [EOS]          # time runs backwards
    assert not gr.accepts(g, back) and decode(back)[0] >= 1
    late = [ev("tie", 0), ev("shift", 10)] + on + [ev("shift", max_steps + 40)] + off + [EOS]   # past the segment's end
    assert not gr.accepts(g, late) and decode(late)[1] >= 1
    stray = [ev("tie", 0), ev("shift", 10)] + on + [ev("tie", 0), ev("shift", 50)] + off + [EOS]  # tie outside its section
    assert not gr.accepts(g, stray) and decode(stray)[0] >= 1
