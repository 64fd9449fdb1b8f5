"""Tied decoding on a box without a GPU: mt3_amd/ties.py (the numpy restatement of mt3n_replay + mt3n_tie_section) against
the note automaton of tests/note_grammar_ref.py, against vocabularies.tie_section_prompt, against the header's own inline
functions (mt3_note_grammar_tie_prompt), and -- the property the feature rests on -- against the HOST note decoder: on
chained segments whose tie sections come from ties.tie_prompt of the row before, the decoder counts nothing invalid or
dropped and the notes it holds after every segment are the replay's held set.

Where the host's state CAN differ from the replay (read off the note decoder, mt3_amd/csrc/symbolic.cpp, whose current program
and velocity outlive a segment; the generator excludes both by name, `restate`, and the last chain test keeps one alive):
  carried_program   the host's current program survives a segment boundary; the engine's rule starts every segment at
                    program 0.  A segment that names a pitch before any program id of its own (only possible behind an
                    empty tie section: a non-empty one opens with a program id) is read under different programs.
  carried_velocity  likewise the current velocity: the rule starts every segment at non-zero velocity, the host keeps a
                    velocity 0 from the segment before.
MT3's targets restate both before first use in every segment (remove_redundant_state_changes starts from no state per
segment), which is what `restate` does: each continuation opens with a program id and a velocity id."""
import ctypes as C

import numpy as np
import pytest

from mt3_amd import _lib, metrics_utils, note_sequences, ties, transcribe, vocabularies
from tests import note_grammar_ref as nr
from tests import note_grammar_script as ns

V = 1536
CODEC = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
TIES = note_sequences.NoteEncodingWithTiesSpec
NOTES = vocabularies.note_grammar(CODEC, V, TIES, 204)
N = nr.from_struct(NOTES)
GRAMMARS = {"toy": ns.toy_notes(), "128x128": ns.toy_notes(128, 128)}


def _struct(n):
    s = _lib.NoteGrammar()
    for f in nr.FIELDS:
        setattr(s.g if hasattr(s.g, f) else s, f, getattr(n, f))
    return s


def _random_row(n, rng, length, tie_at=None, top=None):
    """ids of every kind the rule reads (and a few it does not), biased to few programs and pitches so that pairs are set
    and cleared repeatedly"""
    top = top or n.drum_first + n.drum_count + 4
    kinds = [lambda: n.pitch_first + int(rng.choice([0, 1, 5, 31, 32, n.pitch_count - 1, rng.integers(n.pitch_count)])),
             lambda: n.program_first + int(rng.choice([0, 1, n.program_count - 1, rng.integers(n.program_count)])),
             lambda: n.velocity_first + int(rng.integers(n.velocity_count)),
             lambda: n.shift_first + int(rng.integers(n.shift_count)),
             lambda: int(rng.integers(2, top))]
    row = np.array([kinds[int(rng.choice(5, p=[0.45, 0.15, 0.25, 0.1, 0.05]))]() for _ in range(length)], np.int32)
    row[row == n.tie_id] = n.shift_first
    if tie_at is not None and tie_at < length:
        row[tie_at] = n.tie_id
    return row


def _replay(n, row):
    state = nr.initial(n)
    for tok in (int(t) for t in row):
        if tok <= 1:
            break
        state = nr.advance(n, state, tok)
    return state


@pytest.mark.parametrize("name", sorted(GRAMMARS))
def test_held_after_is_the_note_automatons_replay(name):
    n, rng = GRAMMARS[name], np.random.default_rng(7)
    rows = []
    for i in range(150):
        length = int(rng.integers(1, 90))
        rows.append(_random_row(n, rng, length, tie_at=None if i % 5 == 0 else int(rng.integers(0, length))))
    rows.append(np.array([1, n.pitch_first, n.tie_id], np.int32))                                   # an EOS first
    rows.append(np.array([n.program_first + 1, n.pitch_first + 3, 0, n.pitch_first + 4, n.tie_id], np.int32))   # a 0 mid-row
    rows.append(np.array([n.pitch_first + 2, n.velocity_first, n.pitch_first + 2], np.int32))       # no tie: all declared
    rows.append(np.array([n.tie_id, n.pitch_first + 2, n.velocity_first, n.pitch_first + 2, 1, 0, 0], np.int32))
    for row in rows:
        state = _replay(n, row)
        held = ties.held_after(n, row)
        assert held.dtype == np.uint32 and held.shape == (nr.table_words(n),)
        assert np.array_equal(held, nr.held_words(n, state)), list(row)
        assert set(ties.held_pairs(n, held)) == nr.held_pairs(n, state), list(row)
    assert nr.held_pairs(n, _replay(n, rows[-4])) == set()
    assert nr.held_pairs(n, _replay(n, rows[-3])) == {(1, 3)}
    assert nr.held_pairs(n, _replay(n, rows[-2])) == {(0, 2)}
    assert nr.held_pairs(n, _replay(n, rows[-1])) == set()


def _codec_pairs(held):
    """a held set of the real grammar as the (program, pitch) event values tie_section_prompt takes"""
    ev = lambda i: CODEC.decode_event_index(i - 3).value            # noqa: E731
    return [(ev(NOTES.g.program_first + r), ev(NOTES.g.pitch_first + p)) for r, p in ties.held_pairs(NOTES, held)]


@pytest.mark.parametrize("drop", (False, True))
def test_tie_prompt_is_the_vocabularys_tie_section(drop):
    rng = np.random.default_rng(11)
    rows = [_random_row(N, rng, int(rng.integers(1, 200)), tie_at=int(rng.integers(0, 6)), top=V) for _ in range(40)]
    rows.append(np.array([N.tie_id, 1], np.int32))                                                  # nothing held
    seen_overflow = seen_empty = False
    for row in rows:
        held = ties.held_after(NOTES, row)
        pairs = _codec_pairs(held)
        for cap in (0, 1, 3, len(pairs), len(pairs) + 1, 64):
            got, count = ties.tie_prompt(NOTES, row, cap, drop)
            want = vocabularies.tie_section_prompt(CODEC, pairs[:cap], remove_redundant_programs=drop)
            assert got.dtype == np.int32 and got.shape == (2 * cap + 1,) and count == len(pairs)
            assert ties.prompt_ids(got) == want and not got[len(want):].any(), (list(row), cap)
            seen_overflow |= count > cap
            seen_empty |= count == 0 and want == vocabularies.tie_section_prompt(CODEC, [])
    assert seen_overflow and seen_empty


@pytest.mark.parametrize("name", sorted(GRAMMARS) + ["mt3"])
def test_the_headers_inline_functions_agree(name):
    """mt3_note_grammar_tie_prompt (mt3n_replay + mt3n_tie_section compiled for the host) == ties.py"""
    lib = _lib.load()
    n = GRAMMARS.get(name, N)
    s, rng = _struct(n), np.random.default_rng(3)
    for i in range(60):
        length = int(rng.integers(1, 300))
        row = _random_row(n, rng, length, tie_at=int(rng.integers(0, min(length, 40))))
        if i % 7 == 0:
            row[int(rng.integers(0, length))] = int(rng.integers(0, 2))
        for cap, flags in ((0, 0), (2, 1), (5, 0), (64, 1)):
            out = np.full(2 * cap + 1, -7, np.int32)
            held = np.full(nr.table_words(n), 0xdeadbeef, np.uint32)
            count = lib.mt3_note_grammar_tie_prompt(C.byref(s), row.ctypes.data, length, cap, flags, out.ctypes.data,
                                                    held.ctypes.data)
            want, want_count = ties.tie_prompt(n, row, cap, bool(flags))
            assert count == want_count and np.array_equal(out, want) and np.array_equal(held, ties.held_after(n, row))


# ------------------------------------------------------------------------------------------- the host note decoder
def _continuation(rng, state, steps, restate=True):
    """random ids the note rule allows from `state` on (behind a tie section), EOS last.  restate: the continuation opens
    with a program id and a velocity id, as MT3's targets do (the module docstring's carried_program / carried_velocity)"""
    out = []
    programs = [N.program_first + v for v in (0, 1, 40)]
    pitches = [N.pitch_first + v for v in (0, 12, 31, 32, 33, 60, N.pitch_count - 1)]

    def emit(tok):
        nonlocal state
        assert nr.allowed(N, state, tok), tok
        out.append(tok)
        state = nr.advance(N, state, tok)

    if restate:
        emit(int(rng.choice(programs)))
        emit(N.velocity_first + int(rng.integers(2)))
    t = 0
    while len(out) < steps:
        kind = int(rng.choice(5, p=[0.45, 0.15, 0.2, 0.15, 0.05]))
        if kind == 3:
            t = int(rng.integers(t, min(t + 30, 204) + 1))
            tok = N.shift_first + t
        else:
            tok = int(rng.choice([pitches, programs, [N.velocity_first, N.velocity_first + 1], None,
                                  [N.drum_first + 36, N.drum_first + 40]][kind]))
        if nr.allowed(N, state, tok):
            emit(tok)
    emit(1)
    return out


def _chain(rng, segments, cap, drop, steps=60):
    """id rows of one file's consecutive segments, each opened by ties.tie_prompt of the row before"""
    rows, plens = [], []
    prompt = [N.tie_id]
    for _ in range(segments):
        state = nr.initial(N)
        for tok in prompt:
            state = nr.advance(N, state, tok)
        row = np.zeros(256, np.int32)
        body = prompt + _continuation(rng, state, steps)
        row[: len(body)] = body
        rows.append(row)
        plens.append(len(prompt))
        p, count = ties.tie_prompt(NOTES, row, cap, drop)
        assert count <= cap
        prompt = ties.prompt_ids(p)
    return rows, plens


def _host(rows):
    vocab = vocabularies.vocabulary_from_codec(CODEC)
    preds = []
    for j, row in enumerate(rows):
        tokens = vocab.decode_tf(row)
        tokens = tokens[: int(np.argmax(tokens == vocabularies.DECODED_EOS_ID))]
        start = j * 2.048
        preds.append({"est_tokens": tokens, "start_time": start - start % 0.01})
    return metrics_utils.event_predictions_to_ns_traced(preds, codec=CODEC, encoding_spec=TIES)


@pytest.mark.parametrize("drop", (True, False))
def test_chained_segments_keep_host_and_replay_in_step(drop):
    rng = np.random.default_rng(5 + drop)
    most = 0
    for _ in range(6):
        rows, plens = _chain(rng, 5, 64, drop)
        for row, plen in zip(rows, plens):
            assert nr.accepts(N, row, plen), nr.first_rejected(N, row, plen)
        for j in range(len(rows)):
            # the decoder's active set after segment j: the notes of segments 0 .. j that only the final flush ended
            res = _host(rows[: j + 1])
            assert res["est_invalid_events"] == 0 and res["est_dropped_events"] == 0
            ended_by = res["note_tokens"][:, 1, 0]
            active = {(n.program, n.pitch) for n, e in zip(res["est_ns"].notes, ended_by) if e < 0 and not n.is_drum}
            held = set(_codec_pairs(ties.held_after(NOTES, rows[j])))
            assert active == held, (j, sorted(active ^ held))
            most = max(most, len(held))
    assert most >= 3                                                  # the chains do carry notes over


def test_a_chain_that_does_not_restate_is_the_documented_exception():
    """carried_program, by construction: segment 0 ends on program 40 with nothing held; segment 1, behind its bare tie,
    starts a note without a program id.  The replay files it under program 0, the host under 40 -- the case `restate`
    excludes above, kept here so that the exclusion stays a statement about the code"""
    p40, pitch = N.program_first + 40, N.pitch_first + 12
    row0 = np.array([N.tie_id, p40, N.velocity_first + 1, N.shift_first + 10, N.drum_first + 36, 1], np.int32)
    row1 = np.array([N.tie_id, N.velocity_first + 1, pitch, 1], np.int32)
    assert nr.accepts(N, row0, 1) and nr.accepts(N, row1, 1)
    res = _host([row0, row1])
    ended_by = res["note_tokens"][:, 1, 0]
    active = {(n.program, n.pitch) for n, e in zip(res["est_ns"].notes, ended_by) if e < 0 and not n.is_drum}
    held = set(_codec_pairs(ties.held_after(NOTES, row1)))
    assert {p for p, _ in active} == {40} and {p for p, _ in held} == {0}


# ------------------------------------------------------------------------------------------------------ the C ABI
def test_the_symbols_are_exported_and_typed():
    lib = _lib.load()
    for name in ("mt3_op_tie_prompts", "mt3_note_grammar_tie_prompt"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4                                  # additive entry points
    assert _lib.TIE_DROP_REDUNDANT_PROGRAMS == 1


def test_tie_prompts_refuses_bad_arguments_before_any_device_work():
    lib = _lib.load()
    X = (C.c_int32 * 64)()
    p = C.cast(X, C.c_void_p)
    good = _struct(N)
    no_ties = _struct(N)
    no_ties.g.with_ties = 0
    wide = _struct(ns.toy_notes())
    wide.g.program_count = 129
    overlap = _struct(N)
    overlap.velocity_first = overlap.g.pitch_first
    call = lambda g, ids=p, rows=1, stride=8, cap=4, flags=1, out=p, cnt=p, held=None: \
        lib.mt3_op_tie_prompts(C.byref(g) if g is not None else None, ids, rows, stride, cap, flags, out, cnt, held, None)  # noqa: E731
    cases = [
        (dict(g=None), b"null descriptor"),
        (dict(g=no_ties), b"tie section"),
        (dict(g=wide), b"at most 128 programs and 128 pitches"),
        (dict(g=overlap), b"overlaps another range"),
        (dict(g=good, cap=-1), b"cap must be in [0, 2^30)"),
        (dict(g=good, cap=1 << 30), b"cap must be in [0, 2^30)"),
        (dict(g=good, flags=2), b"unknown flags"),
        (dict(g=good, rows=0), b"rows must be at least 1"),
        (dict(g=good, stride=0), b"ids_stride must be at least 1"),
        (dict(g=good, ids=None), b"null argument"),
        (dict(g=good, out=None), b"null argument"),
        (dict(g=good, cnt=None), b"null argument"),
    ]
    for kw, msg in cases:
        assert call(**kw) == _lib.MT3_ERR_INVALID, msg
        err = lib.mt3_last_error()
        assert err.startswith(b"mt3_op_tie_prompts: ") and msg in err, (err, msg)
    row = np.array([N.tie_id, 1], np.int32)
    out = np.zeros(3, np.int32)
    assert lib.mt3_note_grammar_tie_prompt(C.byref(good), row.ctypes.data, 0, 1, 0, out.ctypes.data, None) == -1
    assert lib.mt3_note_grammar_tie_prompt(C.byref(good), None, 2, 1, 0, out.ctypes.data, None) == -1
    assert lib.mt3_note_grammar_tie_prompt(C.byref(good), row.ctypes.data, 2, 1, 0, out.ctypes.data, None) == 0
    assert list(out) == [N.tie_id, 0, 0]


def test_cli_plan_parses_well_formed_tied(tmp_path):
    wav = tmp_path / "a.wav"
    wav.write_bytes(b"")
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--well-formed-tied", str(wav)])
    assert args.well_formed == "tied"
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--well-formed-notes", str(wav)])
    assert args.well_formed == "notes"
