"""Scripted cases for the NOTES instantiations of the token-rule kernels (mt3_op_token_steps_notes,
mt3_op_beam_search_notes): tests/grammar_script.py's cases, drawn step by step against its float64 mirror with the same
GAP and MAX_TRIES, built inside note_grammar_ref.rule() so that the mirror's state, the lifted ids and the reference are
those of the NOTE rule.

The toy vocabulary (whatever V >= 70): shifts 3 .. 12 (max_steps 8), pitches 13 .. 52 (40: a row spans two words, the second
ragged), velocities 53 (zero) and 54, tie 55, programs 56 .. 58, drums 59 .. 61, the rest extra ids (eight at V = 70: with ids 0 .. 2, the velocities and the
programs the worst state of the room check keeps 16 = 2k ids at k = 8).  As in grammar_script
every id the beam's state (or mask) disallows sits ABOVE the allowed ones.  On top of that a SCRIPT steers each element:
at a free step the ids of the step's kind are lifted by 12 (above the row's ladder, below the disallowed ids), so the
pick is the best ALLOWED id of that kind -- a tie section
that declares notes (and is offered the same pitches again), a velocity 0 followed by held and silent pitches, drums at
velocity 0, program switches between an onset and its offset.  `coverage` says which of the situations a run reached."""
import functools

import numpy as np

from tests import beam_script as bs
from tests import grammar_ref as gr
from tests import grammar_script as gs
from tests import note_grammar_ref as nr

SHIFT0, PITCH0, VEL0, TIE, PROGRAM0, DRUM0 = 3, 13, 53, 55, 56, 59
PITCHES, PROGRAMS = 40, 3


def toy_notes(programs=PROGRAMS, pitches=PITCHES):
    """the toy note grammar; (128, 128) lays the same kinds out over a vocabulary of at least 420 ids"""
    if (programs, pitches) == (PROGRAMS, PITCHES):
        return nr.note_grammar(shift_first=SHIFT0, shift_count=10, max_steps=8, tie_id=TIE, program_first=PROGRAM0,
                               program_count=PROGRAMS, pitch_first=PITCH0, pitch_count=PITCHES, with_ties=1,
                               velocity_first=VEL0, velocity_count=2, drum_first=DRUM0, drum_count=3)
    return nr.note_grammar(shift_first=3, shift_count=10, max_steps=8, pitch_first=13, pitch_count=pitches,
                           velocity_first=13 + pitches, velocity_count=2, tie_id=15 + pitches,
                           program_first=16 + pitches, program_count=programs, drum_first=16 + pitches + programs,
                           drum_count=4, with_ties=1)


def _kinds(n):
    p, q = n.pitch_first, n.program_first
    far = n.pitch_count - 3                               # a pitch of the row's last word
    return {
        "program1": [q + 1], "program0": [q], "program2": [q + n.program_count - 1],
        "declare": [p + 5, p + far, p + 7],               # tie-section declarations (and, offered again, double ties)
        "tie": [n.tie_id], "shift": list(range(n.shift_first, n.shift_first + 9)),
        "vel0": [n.velocity_first], "vel1": [n.velocity_first + 1],
        "offsets": [p + 5, p + far, p + 7, p + 9, p + 33 % n.pitch_count],      # held and silent pitches alike
        "onset": [p + 9, p + far - 1], "drums": list(range(n.drum_first, n.drum_first + n.drum_count)),
        "any": [],
    }


# per element: the kind of every FREE step (steps inside a prompt are skipped; past the script: "any")
SCRIPTS = (
    ("program1", "declare", "declare", "declare", "tie", "shift", "vel0", "offsets", "offsets", "drums", "program0", "vel1",
     "onset", "program2", "vel0", "offsets", "program0", "onset"),
    ("declare", "declare", "tie", "vel0", "offsets", "drums", "shift", "vel1", "onset", "program1", "vel0", "offsets",
     "program0", "onset", "offsets", "any", "any", "any"),
    ("tie", "vel0", "offsets", "drums", "vel1", "onset", "program2", "onset", "vel0", "program0", "onset", "offsets", "shift",
     "any", "any", "any", "any", "any"),
)
# prompts: a tie section that declares (program 1, pitch 5) and ends; one that forces a DISALLOWED token -- the same pair
# declared twice -- and a note-off of a silent pitch after it
PROMPT_SECTION = [PROGRAM0 + 1, PITCH0 + 5, TIE]
PROMPT_BREAKS = [PITCH0 + 7, PITCH0 + 7, TIE, VEL0]


class NoteCase(gs.GrammarCase):
    """A grammar_script.GrammarCase under the toy NOTE grammar, steered by SCRIPTS"""

    def __init__(self, name, k, V, elems, num_steps, prompts=None, masks=None, dims=(PROGRAMS, PITCHES), **kw):
        self.n = toy_notes(*dims)
        self._kind_ids = _kinds(self.n)
        self._ref_n = None
        orig_row, orig_grammar = bs._row, gs.toy_grammar

        def row(rng, V_, k_, style):
            if not isinstance(style, tuple):
                return orig_row(rng, V_, k_, style)
            z = orig_row(rng, V_, k_, style[0])
            z[self._kind_ids[style[1]]] += 12.0
            return z

        prompts = prompts or [None] * elems
        plen = [len(p) if p else 0 for p in prompts]
        base = kw.pop("plan", None) or (lambda b, t: "rand")

        def plan(b, t):
            f = t - plen[b]
            kind = SCRIPTS[b % len(SCRIPTS)][f] if 0 <= f < len(SCRIPTS[0]) else "any"
            return (base(b, t), kind)

        bs._row, gs.toy_grammar = row, (lambda with_ties=1: self.n)
        try:
            with nr.rule():
                super().__init__(name, k, V, elems, num_steps, prompts, masks, plan=plan, **kw)
        finally:
            bs._row, gs.toy_grammar = orig_row, orig_grammar

    @property
    def ref(self):
        """the reference WITH the note rule (and the masks) on these logits"""
        if self._ref_n is None:
            self._ref_n = nr.run_reference(self, self.n, self.masks)
        return self._ref_n

    @property
    def grammar_ref(self):
        """the reference with the event grammar ALONE on the same logits"""
        return gr.run_reference(self, self.n, self.masks)


def coverage(case, rows):
    """which situations the decoded `rows` (one per element) reached, from the logits the case scripted: at a free step the
    best id the event grammar ALONE would allow is what the note rule refused -- "noteoff" (a silent pitch at velocity 0),
    "double_tie", "drum" -- and "switch": a note-off whose onset lies before at least one program token"""
    n, found = case.n, set()
    for b, row in enumerate(rows):
        state, mask = nr.initial(n), case.masks[b] if case.masks is not None else None
        onset_at = {}
        for t, tok in enumerate(int(x) for x in row):
            if tok == 0:
                break
            gram, note, _ = nr.split(state)
            if t >= case.plen(b):
                x = np.array(case.scaled(t)[b * case.k], np.float64)
                x[~nr._g_rule_vector(n, gram, mask, case.V)] = -np.inf
                top = int(np.argmax(x))
                if top != tok and not nr.allowed(n, state, top):
                    if n.pitch_first <= top < n.pitch_first + n.pitch_count:
                        found.add("double_tie" if gram & gr.TIE_SECTION else "noteoff")
                    else:
                        found.add("drum")
            if n.pitch_first <= tok < n.pitch_first + n.pitch_count and not gram & gr.TIE_SECTION:
                key = (note & nr.PROGRAM, tok)
                if note & nr.VELOCITY_ZERO:
                    if key in onset_at and any(n.program_first <= int(r) < n.program_first + n.program_count
                                               for r in row[onset_at[key] + 1:t]):
                        found.add("switch")
                else:
                    onset_at[key] = t
            if tok == 1:
                break
            state = nr.advance(n, state, tok)
    return found


def fork_with_other_table(case):
    """steps of the k-beam reference at which some new slot j descends from a parent p != j whose table differs from the
    table slot j held before the step"""
    ref, k, hits = case.ref, case.k, 0
    for t in range(1, ref.steps_run):
        for s in range(case.elems * k):
            before, after = nr.split(ref.states[t - 1][s])[2], nr.split(ref.states[t][s])[2]
            others = [nr.split(ref.states[t - 1][(s // k) * k + j])[2] for j in range(k) if j != s % k]
            near = lambda a, b_: bin(a ^ b_).count("1") <= 1            # noqa: E731  (one token changes at most one bit)
            if not near(before, after) and any(near(o, after) for o in others):
                hits += 1
    return hits


def _prompts(kind):
    return {"none": [None, None, None], "section": [PROMPT_SECTION, None, PROMPT_SECTION],
            "breaks": [None, PROMPT_BREAKS, PROMPT_SECTION]}[kind]


def _mask(V, n):
    """a mask that intersects the rule: every other pitch, the odd shifts and one drum go; the scripted pitches stay"""
    keep = set(_kinds(n)["declare"] + _kinds(n)["offsets"] + _kinds(n)["onset"])
    forbid = [i for i in range(n.pitch_first, n.pitch_first + n.pitch_count, 2) if i not in keep]
    forbid += list(range(n.shift_first + 1, n.shift_first + 10, 2)) + [n.drum_first]
    return gs._mask(V, forbid)


@functools.lru_cache(maxsize=None)
def beam_cases():
    out = []
    for k in (1, 2, 8):
        out.append(NoteCase("n_v70_k%d" % k, k, 70, 3, 16, _prompts("none"), plan=lambda b, t: "no_eos" if t < 12 else "rand"))
        out.append(NoteCase("n_v70_breaks_k%d" % k, k, 70, 3, 14, _prompts("breaks"),
                            plan=lambda b, t: "no_eos" if t < 10 else "rand"))
        out.append(NoteCase("n_v70_scale_k%d" % k, k, 70, 3, 12, _prompts("section"), n_ss=32))
        out.append(NoteCase("n_v2048_k%d" % k, k, 2048, 3, 12, _prompts("section"),
                            plan=lambda b, t: "no_eos" if t < 9 else "rand"))
    m = _mask(70, toy_notes())
    out.append(NoteCase("n_v70_mask_k2", 2, 70, 3, 14, _prompts("section"), masks=[m, None, m],
                        plan=lambda b, t: "no_eos" if t < 10 else "rand"))
    out.append(NoteCase("n_v70_maxlen_k2", 2, 70, 3, 16, _prompts("none"), max_len=9,
                        plan=lambda b, t: "no_eos" if t >= 9 else "rand"))
    out.append(NoteCase("n_v512_128x128_k2", 2, 512, 3, 14, _prompts("none"), dims=(128, 128),
                        plan=lambda b, t: "no_eos" if t < 10 else "rand"))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def token_cases():
    out = []
    for V in (70, 2048, 2100):                         # 2100: the token kernel's element-loop path
        out.append(NoteCase("nt_v%d" % V, 1, V, 3, 16, _prompts("none"), plan=lambda b, t: "no_eos" if t < 12 else "rand"))
        out.append(NoteCase("nt_v%d_breaks" % V, 1, V, 3, 14, _prompts("breaks"),
                            plan=lambda b, t: "no_eos" if t < 10 else "rand"))
    out.append(NoteCase("nt_scale", 1, 70, 3, 12, _prompts("section"), n_ss=32))
    out.append(NoteCase("nt_scale_v2100", 1, 2100, 3, 12, _prompts("section"), n_ss=32))
    out.append(NoteCase("nt_maxlen", 1, 70, 3, 16, _prompts("section"), max_len=9,
                        plan=lambda b, t: "no_eos" if t >= 9 else "rand"))
    for V in (70, 2100):
        m = _mask(V, toy_notes())
        out.append(NoteCase("nt_mask_v%d" % V, 1, V, 3, 14, _prompts("section"), masks=[m, None, m],
                            plan=lambda b, t: "no_eos" if t < 10 else "rand"))
    out.append(NoteCase("nt_v512_128x128", 1, 512, 3, 16, _prompts("none"), dims=(128, 128),
                        plan=lambda b, t: "no_eos" if t < 12 else "rand"))
    return tuple(out)


class SampledCase:
    """sampling_script.Case's `tables` form (masks, prompts, max_len) with the toy NOTE grammar in the toy grammar's place:
    the first draw for which every pick of the sampled reference under the note rule meets sampling_script's margins"""

    def __init__(self, V, mode):
        from tests import sampling_script as ss
        self.n = toy_notes()
        orig = gs.toy_grammar
        gs.toy_grammar = lambda with_ties=1: self.n
        try:
            with nr.rule():
                self.case = ss.Case(V, mode, False, True)
        finally:
            gs.toy_grammar = orig
        self.name = "ns_" + self.case.name
