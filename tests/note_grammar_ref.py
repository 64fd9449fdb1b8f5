"""CPU reference of NOTE-CONSISTENT decoding (mt3_engine_set_note_grammar; the rule: include/mt3_hip.h, mt3n_*): the
automaton in pure Python, and greedy / beam-1 / k-beam / sampled references built on tests/grammar_ref.py rather than
restated: inside `rule()` the three functions grammar_ref's references are written in (initial, advance, _rule_vector) are
the note rule's, over a state that holds the grammar's packed int, the `note` int and the table of sounding notes.

A state is ONE Python int: bits 0 .. 31 the grammar state (grammar_ref's), bits 32 .. 63 the `note` int (bits 0 .. 7 the
program value, bit 31 "velocity is zero"), and from bit 64 the table, bit (program * words + pitch // 32) * 32 + pitch % 32
as the device lays it out in uint32 words.  `split` gives the three, `held_words` the table as the device's words."""
import contextlib
import types

import numpy as np

from tests import grammar_ref as gr
from tests.beam_search_ref import EOS

VELOCITY_ZERO, PROGRAM = 1 << 31, 0xFF
FIELDS = gr.FIELDS + ("velocity_first", "velocity_count", "drum_first", "drum_count")
M32 = (1 << 32) - 1
_g_initial, _g_advance, _g_allowed, _g_rule_vector = gr.initial, gr.advance, gr.allowed, gr._rule_vector


def note_grammar(**kw):
    """a descriptor with the fields of mt3_note_grammar (its `g` member's fields flat beside the four ranges)"""
    assert set(kw) == set(FIELDS), sorted(set(kw) ^ set(FIELDS))
    return types.SimpleNamespace(**{f: int(kw[f]) for f in FIELDS})


def from_struct(s):
    return note_grammar(**{f: getattr(s.g, f) for f in gr.FIELDS},
                        **{f: getattr(s, f) for f in FIELDS[len(gr.FIELDS):]})


def row_words(n):
    return (n.pitch_count + 31) // 32


def table_words(n):
    return n.program_count * row_words(n)


def split(state):
    return state & M32, (state >> 32) & M32, state >> 64


def join(gram, note, held):
    return gram | (note << 32) | (held << 64)


def held_words(n, state):
    held = split(state)[2]
    return np.array([(held >> (32 * w)) & M32 for w in range(table_words(n))], np.uint32)


def held_pairs(n, state):
    """the sounding (program value, pitch value) pairs of a state"""
    held, W, out = split(state)[2], row_words(n), set()
    while held:
        low = held & -held
        bit = low.bit_length() - 1
        out.add((bit // (W * 32), bit % (W * 32)))
        held ^= low
    return out


def initial(n):
    return join(_g_initial(n), 0, 0)


def advance(n, state, tok):
    gram, note, held = split(state)
    bit0 = (note & PROGRAM) * row_words(n) * 32
    p = tok - n.pitch_first
    if 0 <= p < n.pitch_count:
        if gram & gr.TIE_SECTION or not note & VELOCITY_ZERO:
            held |= 1 << (bit0 + p)
        else:
            held &= ~(1 << (bit0 + p))
    elif 0 <= tok - n.program_first < n.program_count:
        note = (note & ~PROGRAM) | (tok - n.program_first)
    elif 0 <= tok - n.velocity_first < n.velocity_count:
        note = note | VELOCITY_ZERO if tok == n.velocity_first else note & ~VELOCITY_ZERO
    return join(_g_advance(n, gram, tok), note, held)


def allowed(n, state, i):
    gram, note, held = split(state)
    if not _g_allowed(n, gram, i):
        return False
    p = i - n.pitch_first
    if 0 <= p < n.pitch_count:
        bit = bool((held >> ((note & PROGRAM) * row_words(n) * 32 + p)) & 1)
        if gram & gr.TIE_SECTION:
            return not bit
        return bit if note & VELOCITY_ZERO else True
    if not gram & gr.TIE_SECTION and note & VELOCITY_ZERO and 0 <= i - n.drum_first < n.drum_count:
        return False
    return True


def allowed_vector(n, state, V):
    return np.array([allowed(n, state, i) for i in range(V)], bool)


def _rule_vector(n, state, mask, V):
    a = allowed_vector(n, state, V) if n is not None else np.ones(V, bool)
    return a & mask if mask is not None else a


@contextlib.contextmanager
def rule():
    """grammar_ref's references run the NOTE rule inside: its initial / advance / allowed / _rule_vector are this module's"""
    saved = gr.initial, gr.advance, gr.allowed, gr._rule_vector
    gr.initial, gr.advance, gr.allowed, gr._rule_vector = initial, advance, allowed, _rule_vector
    try:
        yield
    finally:
        gr.initial, gr.advance, gr.allowed, gr._rule_vector = saved


def accepts(n, row, plen=0):
    """grammar_ref.accepts under the note rule: every FREE token of `row` is allowed in the state the tokens before it
    leave"""
    with rule():
        return gr.accepts(n, row, plen)


def first_rejected(n, row, plen=0):
    """(position, state before it) of the first free token the rule disallows, or None"""
    state = initial(n)
    for t, tok in enumerate(int(x) for x in row):
        if tok == 0 and not np.any(np.asarray(row)[t:]):
            return None
        if t >= plen and not allowed(n, state, tok):
            return t, state
        if tok == EOS:
            return None
        state = advance(n, state, tok)
    return None


def replay(n, row):
    with rule():
        return gr.replay(n, row)


def greedy(logits, prompts, n, masks=None, max_len=0):
    """grammar_ref.greedy under the note rule: ids [rows][T], done [T][rows] and the states, a [T][rows] list of lists of
    Python ints (grammar_ref keeps them in an int64 array, which cannot hold a table)"""
    T, B, V = logits.shape
    ids, done, states = np.zeros((B, T), np.int32), np.zeros((T, B), np.int32), [[0] * B for _ in range(T)]
    for b in range(B):
        # one row at a time through grammar_ref.greedy's own loop is not possible (its state array is int64): the loop
        # below is that loop with the state kept as a Python int
        P = list(prompts[b]) if prompts is not None and prompts[b] is not None else []
        mask = masks[b] if masks is not None else None
        state, over = initial(n), False
        for t in range(T):
            if not over:
                if t < len(P):
                    tok = P[t]
                else:
                    x = np.where(_rule_vector(n, state, mask, V), logits[t, b].astype(np.float64), -np.inf)
                    tok = int(np.argmax(x))
                ids[b, t] = tok
                state = advance(n, state, tok)
                over = (t >= len(P) and tok == EOS) or bool(max_len and t + 1 >= max_len)
            done[t, b], states[t][b] = over, state
    return ids, done, states


def run_reference(case, n, masks=None, logits=None):
    """grammar_ref.run_reference (beam-1 and k-beam) under the note rule; r.states [steps][elems * k] are Python ints"""
    with rule():
        return gr.run_reference(case, n, masks, logits)


def sampled(scaled, streams, params, prompts, n, masks=None, max_len=0):
    """sampling_script.reference (the sampled greedy loop) under the note rule"""
    from tests import sampling_script as ss
    with rule():
        return ss.reference(scaled, streams, params, prompts, n, masks, max_len)
