"""The note rule (tests/note_grammar_ref.py, the automaton the kernels are tested against) tied to the REFERENCE's
semantics: the oracle's pure-Python note decoder (oracle/symbolic.py: note_sequences.decode_note_event and
run_length_encoding.decode_events).

A few hundred random token rows over the real `mt3` codec -- a tie section, then events -- are decoded one by one, each by a
fresh decoder whose active set is pre-seeded with the row's own tie-section pairs (what the previous segment would have left
sounding, were the tie section right: the part the engine cannot know).  A row the acceptor accepts must raise none of
  "note-off for inactive pitch/program", "pitch/program is already tied", "velocity cannot be zero for drum event";
a row with one planted violation of each kind must be rejected by the acceptor AT the planted token, and the decoder must
count an invalid event of that kind.  Also here, on the CPU: what the scripts of tests/note_grammar_script.py reach."""
import numpy as np
import pytest

from mt3_amd import note_sequences, vocabularies
from oracle import symbolic as S
from tests import note_grammar_ref as nr
from tests import note_grammar_script as ns

V = 1536
NOTE_OFF, TIED_TWICE, DRUM_ZERO = ("note-off for inactive pitch/program", "pitch/program is already tied",
                                   "velocity cannot be zero for drum event")


@pytest.fixture(scope="module")
def setup():
    codec = S.build_codec(S.VocabularyConfig(num_velocity_bins=1))
    product = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    n = nr.from_struct(vocabularies.note_grammar(product, V, note_sequences.NoteEncodingWithTiesSpec, 204))
    return codec, n


class _Recorder(S.NoteDecoder):
    """the oracle's decoder, keeping the message of every error decode_events swallows"""

    def __init__(self):
        super().__init__("ties")
        self.errors = []

    def consume(self, time, ev, codec):
        try:
            super().consume(time, ev, codec)
        except ValueError as e:
            self.errors.append(str(e))
            raise


def _decode(codec, n, row):
    """the errors and the invalid-event count of `row` (ids; EOS-trimmed here), decoded alone with its own tie-section
    pairs pre-seeded as sounding"""
    ids = [int(t) for t in row]
    ids = ids[:ids.index(1)] if 1 in ids else ids
    dec = _Recorder()
    program = 0
    for t in ids:                                       # the pairs the tie section declares
        if t == n.tie_id:
            break
        if n.program_first <= t < n.program_first + n.program_count:
            program = codec.decode_event_index(t - 3).value
        elif n.pitch_first <= t < n.pitch_first + n.pitch_count:
            dec.active[(codec.decode_event_index(t - 3).value, program)] = (0.0, 100)
    dec.begin_segment()
    invalid, _ = S.decode_events(dec, [t - 3 for t in ids], 0.0, None, codec)
    return dec.errors, invalid


def _random_row(rng, n, plant=None):
    """a tie section (some programs, some pitches, the tie), then events in grammar order -- increasing shifts, velocities,
    programs, onsets, note-offs of sounding notes, drums at velocity 1 -- that the acceptor accepts; plant: one violation of
    that kind at a random place after it makes sense.  Returns (row, index of the planted token or None)."""
    row, state, planted = [], nr.initial(n), None

    def emit(tok):
        nonlocal state
        row.append(tok)
        state = nr.advance(n, state, tok)

    def pairs():
        return sorted(nr.held_pairs(n, state))

    for _ in range(int(rng.integers(0, 5))):
        if rng.random() < 0.4:
            emit(n.program_first + int(rng.integers(0, n.program_count)))
        free = [p for p in range(n.pitch_count) if (nr.split(state)[1] & nr.PROGRAM, p) not in pairs()]
        emit(n.pitch_first + int(rng.choice(free)))
    if plant == TIED_TWICE and pairs():
        prog, p = pairs()[int(rng.integers(0, len(pairs())))]
        emit(n.program_first + prog)
        planted = len(row)
        emit(n.pitch_first + p)
    emit(n.tie_id)
    time, want_at = 0, int(rng.integers(2, 12))
    for step in range(int(rng.integers(14, 30))):
        gram, note, _ = nr.split(state)
        if plant in (NOTE_OFF, DRUM_ZERO) and planted is None and step >= want_at:
            if not note & nr.VELOCITY_ZERO:
                emit(n.velocity_first)
            note = nr.split(state)[1]
            planted = len(row)
            if plant == DRUM_ZERO:
                emit(n.drum_first + int(rng.integers(0, n.drum_count)))
            else:
                silent = [p for p in range(n.pitch_count) if (note & nr.PROGRAM, p) not in pairs()]
                emit(n.pitch_first + int(rng.choice(silent)))
            continue
        r = rng.random()
        if r < 0.2 and time < n.max_steps and not gram & (1 << 30):
            time = int(rng.integers(time, n.max_steps + 1))
            emit(n.shift_first + time)
        elif r < 0.35:
            emit(n.velocity_first + int(rng.integers(0, 2)))
        elif r < 0.5:
            emit(n.program_first + int(rng.integers(0, n.program_count)))
        elif note & nr.VELOCITY_ZERO:
            mine = [p for prog, p in pairs() if prog == note & nr.PROGRAM]
            if mine:
                emit(n.pitch_first + int(rng.choice(mine)))
            else:
                emit(n.velocity_first + 1)
        elif r < 0.85:
            emit(n.pitch_first + int(rng.integers(0, n.pitch_count)))      # an onset, of a sounding pitch too
        else:
            emit(n.drum_first + int(rng.integers(0, n.drum_count)))
    row.append(1)
    return row, planted


def test_accepted_rows_raise_none_of_the_three_errors(setup):
    codec, n = setup
    rng = np.random.default_rng(20260)
    offs = 0
    for i in range(300):
        row, _ = _random_row(rng, n)
        assert nr.accepts(n, row), (i, nr.first_rejected(n, row))
        errors, invalid = _decode(codec, n, row)
        assert not [e for e in errors if e in (NOTE_OFF, TIED_TWICE, DRUM_ZERO)], (i, errors)
        assert invalid == len(errors) == 0, (i, errors)
        state = nr.initial(n)
        for t in row[:-1]:
            offs += bool(nr.split(state)[1] & nr.VELOCITY_ZERO and n.pitch_first <= t < n.pitch_first + n.pitch_count and
                         not nr.split(state)[0] >> 31)
            state = nr.advance(n, state, t)
    assert offs >= 100                                   # the rows do end notes (one in three would do)


@pytest.mark.parametrize("kind", (NOTE_OFF, TIED_TWICE, DRUM_ZERO), ids=("note_off", "tied_twice", "drum_zero"))
def test_planted_violations_are_rejected_and_counted(setup, kind):
    codec, n = setup
    rng = np.random.default_rng(len(kind))
    seen = 0
    for i in range(150):
        row, at = _random_row(rng, n, plant=kind)
        if at is None:                                   # (a tie section that declared nothing cannot tie twice)
            assert kind == TIED_TWICE
            continue
        seen += 1
        rejected = nr.first_rejected(n, row)
        assert rejected is not None and rejected[0] == at, (i, at, rejected)
        errors, invalid = _decode(codec, n, row)
        assert errors.count(kind) >= 1 and invalid >= 1, (i, errors)
        assert errors[0] == kind                         # and it is the FIRST thing the decoder objects to
    assert seen >= 90


def test_the_scripts_reach_what_they_are_for():
    """the situations tests/test_gpu_note_grammar_rules.py runs on the GPU, found in the scripted cases' references"""
    found = set()
    for case in ns.token_cases():
        scaled = np.stack([case.scaled(t) for t in range(case.num_steps)])
        ids, _, _ = nr.greedy(scaled, case.prompts, case.n, case.masks, case.max_len)
        found |= ns.coverage(case, ids)
        plen = [len(p) if p else 0 for p in case.prompts]
        assert all(nr.accepts(case.n, ids[b], plen[b]) for b in range(case.elems)), case.name
    assert found >= {"noteoff", "double_tie", "drum", "switch"}, found
    hits = {c.name: ns.fork_with_other_table(c) for c in ns.beam_cases() if c.k > 1}
    assert sum(hits.values()) >= 10 and sum(1 for v in hits.values() if v) >= 4, hits
    # the grammar alone would have let the scripted rows break the note rule
    broken = 0
    for case in ns.token_cases():
        best = case.grammar_ref.decodes[:, -1]
        plen = [len(p) if p else 0 for p in case.prompts]
        broken += sum(not nr.accepts(case.n, best[b], plen[b]) for b in range(case.elems))
    assert broken >= len(ns.token_cases())
