"""CPU reference of WELL-FORMED decoding (mt3_engine_set_token_grammar; the rule: include/mt3_hip.h): the event-grammar
automaton in pure Python, and greedy / beam-1 / k-beam references with masks, prompts and the grammar, built on
tests/prompt_ref.py (which builds on tests/beam_search_ref.py) rather than restating them.

The state is the packed int of the header: bit 31 = inside the tie section, bit 30 = the previous token was a shift, bits
0 .. 29 = t, the time of the last shift.  Python ints here are the UNSIGNED value; `as_i32` gives what the device holds."""
import types

import numpy as np

from tests import prompt_ref as pr
from tests.beam_search_ref import EOS

TIE_SECTION, PREV_SHIFT, TIME = 1 << 31, 1 << 30, (1 << 30) - 1
FIELDS = ("shift_first", "shift_count", "max_steps", "tie_id", "program_first", "program_count", "pitch_first",
          "pitch_count", "with_ties")


def grammar(**kw):
    """a descriptor with the fields of mt3_token_grammar"""
    assert set(kw) == set(FIELDS), sorted(set(kw) ^ set(FIELDS))
    return types.SimpleNamespace(**{f: int(kw[f]) for f in FIELDS})


def from_struct(s):
    return grammar(**{f: getattr(s, f) for f in FIELDS})


def initial(g):
    return TIE_SECTION if g.with_ties else 0


def advance(g, state, tok):
    v = tok - g.shift_first
    if 0 <= v < g.shift_count:
        t = min((state & TIME) + v, 1 << 29) if state & PREV_SHIFT else v
        return (state & TIE_SECTION) | PREV_SHIFT | t
    if tok == g.tie_id:
        return state & TIME
    return state & ~PREV_SHIFT


def allowed(g, state, i):
    if i == EOS:
        return True
    if state & TIE_SECTION:
        return (i == g.tie_id or g.program_first <= i < g.program_first + g.program_count or
                g.pitch_first <= i < g.pitch_first + g.pitch_count)
    if i == g.tie_id:
        return False
    v = i - g.shift_first
    if 0 <= v < g.shift_count:
        return not (state & PREV_SHIFT) and (state & TIME) <= v <= g.max_steps
    return True


def allowed_vector(g, state, V):
    return np.array([allowed(g, state, i) for i in range(V)], bool)


def as_i32(state):
    return int(np.array([state], np.uint32).view(np.int32)[0])


def accepts(g, row, plen=0):
    """True iff every FREE token of `row` (ids up to and including the first EOS; the first `plen` are a prompt: they only
    advance the state) is allowed in the state the tokens before it leave; ids after EOS (or after the first padding 0 of a
    row that ended without one) must be 0."""
    state = initial(g)
    for t, tok in enumerate(int(x) for x in row):
        if tok == 0 and not np.any(np.asarray(row)[t:]):
            return True                                 # padding to the end: the row ended without EOS (max_len, or unfilled)
        if t >= plen and not allowed(g, state, tok):
            return False
        if tok == EOS:
            return not np.any(np.asarray(row)[t + 1:])
        state = advance(g, state, tok)
    return True


def replay(g, row):
    """the state after each token of `row`, frozen from the first EOS (whose own advance is the last one)"""
    out, state, over = [], initial(g), False
    for tok in (int(x) for x in row):
        if not over:
            state = advance(g, state, tok)
            over = tok == EOS
        out.append(state)
    return out


def _rule_vector(g, state, mask, V):
    a = allowed_vector(g, state, V) if g is not None else np.ones(V, bool)
    return a & mask if mask is not None else a


def greedy(logits, prompts, g=None, masks=None, max_len=0):
    """prompt_ref.greedy with the grammar and per-row masks (bool [V] or None): ids [rows][T], done [T][rows] and the
    packed states [T][rows] after every step (a finished row keeps its last).  g is None: no grammar (states 0)."""
    T, B, V = logits.shape
    ids, done, states = np.zeros((B, T), np.int32), np.zeros((T, B), np.int32), np.zeros((T, B), np.int64)
    for b in range(B):
        P = list(prompts[b]) if prompts is not None and prompts[b] is not None else []
        mask = masks[b] if masks is not None else None
        state, over = (initial(g) if g is not None else 0), False
        for t in range(T):
            if not over:
                if t < len(P):
                    tok = P[t]
                else:
                    x = np.where(_rule_vector(g, state, mask, V), logits[t, b].astype(np.float64), -np.inf)
                    tok = int(np.argmax(x))
                ids[b, t] = tok
                if g is not None:
                    state = advance(g, state, tok)
                over = (t >= len(P) and tok == EOS) or bool(max_len and t + 1 >= max_len)
            done[t, b], states[t, b] = over, state
    return ids, done, states


def run_reference(case, g=None, masks=None, logits=None):
    """prompt_ref.run_reference with each beam's own allowed vector (grammar state of its slot, element mask) applied to
    the logits before the log-softmax; r.states [steps][elems * k] holds the packed state of every slot after each step.
    g is None and masks is None: prompt_ref.run_reference itself."""
    if g is None and masks is None:
        return pr.run_reference(case, logits)
    k, n, V = case.k, case.elems * case.k, case.V
    state = [initial(g) if g is not None else 0] * n
    was_retired = np.zeros(case.elems, bool)
    states = []

    def rows_of(t):
        if logits is None:
            x = case.scaled(t).copy()
        else:
            x = np.asarray(logits[t], np.float64).copy()
            if case.ss is not None:
                x = x * ((case.ss[t].astype(np.float64).sum(-1) / case.dim + 1e-6) ** -0.5)[:, None]
        for s in range(n):
            x[s, ~_rule_vector(g, state[s], masks[s // k] if masks is not None else None, V)] = -np.inf
        return x

    class View:                                         # the case as prompt_ref.run_reference reads it, on the ruled rows
        pass

    view = View()
    view.k, view.num_steps, view.elems, view.max_len, view.ss, view.dim = k, case.num_steps, case.elems, case.max_len, None, 0
    view.prompts = getattr(case, "prompts", None)
    view.scaled = rows_of

    orig = pr.beam_search

    def beam_search(step, reorder, batch, kk, num_steps, prompts=None, on_step=None, **kw):
        def watch(t, live_lp, live_seq, index, retired, fin_score, fin_valid):
            new = list(state)
            for b in range(batch):
                if was_retired[b]:
                    continue
                for j in range(kk):
                    s = b * kk + j
                    if g is not None:
                        new[s] = advance(g, state[int(index[s])], int(live_seq[b, j, t]))
            state[:] = new
            was_retired[:] = retired
            states.append(list(state))
            on_step(t, live_lp, live_seq, index, retired, fin_score, fin_valid)
        return orig(step, reorder, batch, kk, num_steps, prompts=prompts, on_step=watch, **kw)

    pr.beam_search = beam_search
    try:
        r = pr.run_reference(view)
    finally:
        pr.beam_search = orig
    r.states = states[:len(r.retired)]
    return r
