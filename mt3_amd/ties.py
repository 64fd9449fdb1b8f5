"""Tied decoding restated in numpy / pure Python: what a segment left sounding, as the tie section of the next.

The rule is stated in include/mt3_hip.h (mt3n_replay + mt3n_tie_section); the kernel mt3_op_tie_prompts
(mt3_amd/csrc/ties.hip) computes it one workgroup per row; this module is the third statement, the one the tests compare
the other two with -- as mt3_amd/sampling.py is for the sampling rule.

`grammar` is a note grammar descriptor: a `_lib.NoteGrammar` (`vocabularies.note_grammar`) or any object with the fields
of mt3_note_grammar flat (shift_first ... drum_count).  A held set is a uint32 array of mt3n_table_words words, bit
p % 32 of word program * row_words + p // 32 set = (program value, pitch value p) is sounding."""
from __future__ import annotations

import numpy as np

TIE_SECTION, PREV_SHIFT = 1 << 31, 1 << 30
DROP_REDUNDANT_PROGRAMS = 1


def _flat(grammar):
    g = getattr(grammar, "g", grammar)
    return (int(g.tie_id), int(g.program_first), int(g.program_count), int(g.pitch_first), int(g.pitch_count),
            int(grammar.velocity_first), int(grammar.velocity_count))


def row_words(grammar) -> int:
    return (_flat(grammar)[4] + 31) // 32


def table_words(grammar) -> int:
    return _flat(grammar)[2] * row_words(grammar)


def held_after(grammar, row) -> np.ndarray:
    """The serial replay of an engine id row (prompt included, 0-padded after EOS): from the tie-section state, program 0,
    velocity non-zero and nothing held, every id up to and without the first id <= 1 is applied -- a program id sets the
    program, a velocity id sets or clears "velocity is zero", `tie` ends the tie section, a pitch id sets its (program,
    pitch) inside the tie section or at non-zero velocity and clears it otherwise.  Returns the held set."""
    tie, prog0, n_prog, pitch0, n_pitch, vel0, n_vel = _flat(grammar)
    W = row_words(grammar)
    held = np.zeros(n_prog * W, np.uint32)
    in_tie, program, zero = True, 0, False
    for tok in (int(t) for t in np.asarray(row).reshape(-1)):
        if tok <= 1:
            break
        if 0 <= tok - pitch0 < n_pitch:
            p = tok - pitch0
            bit = np.uint32(1 << (p & 31))
            if in_tie or not zero:
                held[program * W + (p >> 5)] |= bit
            else:
                held[program * W + (p >> 5)] &= ~bit
        elif 0 <= tok - prog0 < n_prog:
            program = tok - prog0
        elif 0 <= tok - vel0 < n_vel:
            zero = tok == vel0
        elif tok == tie:
            in_tie = False
    return held


def held_pairs(grammar, held) -> list:
    """the (program value, pitch value) pairs of a held set, ascending"""
    W = row_words(grammar)
    bits = np.flatnonzero(np.unpackbits(np.asarray(held, np.uint32).astype("<u4").view(np.uint8), bitorder="little"))
    return [(int(i) // (32 * W), int(i) % (32 * W)) for i in bits]


def tie_section(grammar, held, cap: int, drop_redundant_programs: bool = True):
    """The tie section that declares a held set -> (int32 [2 * cap + 1] prompt row, 0-padded; pairs held): the pairs in
    ascending (program, pitch) order, a program id then a pitch id per pair -- with drop_redundant_programs a program id
    only where the program changes -- then `tie`.  More than `cap` pairs: the first `cap` are kept; the count is all."""
    tie, prog0, _, pitch0, _, _, _ = _flat(grammar)
    if cap < 0:
        raise ValueError("cap must not be negative, got %r" % (cap,))
    pairs = held_pairs(grammar, held)
    out, last = [], None
    for program, pitch in pairs[:cap]:
        if not (drop_redundant_programs and program == last):
            out.append(prog0 + program)
        out.append(pitch0 + pitch)
        last = program
    out.append(tie)
    row = np.zeros(2 * cap + 1, np.int32)
    row[: len(out)] = out
    return row, len(pairs)


def tie_prompt(grammar, row, cap: int = 64, drop_redundant_programs: bool = True):
    """`tie_section` of `held_after(grammar, row)`: the prompt row of the file's next segment and the pairs held"""
    return tie_section(grammar, held_after(grammar, row), cap, drop_redundant_programs)


def prompt_ids(prompt_row) -> list:
    """a 0-padded prompt row as the id list `Transformer.set_prompts` / `prompts=` take"""
    r = np.asarray(prompt_row).reshape(-1)
    return [int(v) for v in r[: int(np.count_nonzero(r))]]
