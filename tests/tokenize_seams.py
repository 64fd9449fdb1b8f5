"""Scripted jobs for the target tokenizer at the level of its ABI (include/mt3_hip.h, "target tokenizer"): event columns
and the two tables, written so that the thing under test sits on a tile edge of the kernel or on a scan carry
(tests/test_tokenize_seams_ref.py on the host, tests/test_gpu_tokenize_seams.py on the device).

A case is the six event columns, the file table, the row table, a rule, the strides to run it at, and its WITNESS: claims
(kind, row, subject, stated) that say where the case puts what it is about.  `observe` works the same thing out from the
tables alone, in plain Python; the host test asserts stated == observed for every claim, so that an edit of a builder cannot
quietly move a seam away.  Tile origins follow the kernel's own rule: event tiles of 256 start at the row's first event,
advance tiles of 256 at the tie begin of the file's previous row (0 before the first).

`restate_row` is the rule's items 1-5 once more, serially: a dict for the held table, lists for the ids.  It is written
from the header's text and calls nothing of the library."""
import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from mt3_amd import _lib, note_sequences, tokenize, vocabularies
from mt3_amd.note_sequences import Note, NoteSequence

TIES = note_sequences.NoteEncodingWithTiesSpec
TILE = 256
INT32_MAX = tokenize.INT32_MAX
X = (9, 64)                                    # the pair the advance cases are about; fillers never touch program 9


@dataclasses.dataclass
class Case:
    name: str
    events: np.ndarray                         # int32 [6, n]: step | pitch | program | velbin | is_drum | note
    files: np.ndarray                          # tokenize.FILE_DTYPE
    rows: np.ndarray                           # tokenize.ROW_DTYPE
    rule: _lib.TokenizeRule
    strides: tuple
    claims: list                               # the witness: (kind, row, subject, stated), see `observe`
    recipe: Optional[dict] = None              # sequences, frames, codec, granularity, segment_frames: the recipe can be asked

    def rule_bin(self, v):
        return min(max(int(v), 0), self.rule.velocity_count - 1)


# ------------------------------------------------------------------------------------------------ the rule, restated
def restate_row(rule, ev, step_lo, step_hi):
    """One row before the cut: (ids, note_of, is_onset, trace), EOS included.  trace[i] = (kind, event) says what
    position i is: 'tie program', 'tie pitch', 'tie', 'shift', 'program', 'velocity', 'pitch', 'drum', 'eos'."""
    step, pitch, program, velbin, is_drum, note = (ev[k].tolist() for k in range(6))
    ties = rule.spec == _lib.SPEC_TIES
    ids, note_of, is_onset, trace = [], [], [], []
    last = {"program": None, "velocity": None}                       # "none yet" matches nothing

    def put(token, kind, e=-1, of=-1, onset=0):
        ids.append(token), note_of.append(of), is_onset.append(onset), trace.append((kind, e))

    def put_program(p, kind, e=-1):                                  # items 3 and 4
        m = rule.program_map[p & 127]
        if m >= 0 and m != last["program"]:
            put(rule.program_first + m, kind, e)
        if m >= 0:
            last["program"] = m

    def bin_of(v):
        return min(max(v, 0), rule.velocity_count - 1)

    if ties:                                                         # item 1
        b = next((e for e in range(len(step)) if step[e] >= step_lo), None)
        if b is None:
            b = step.index(step[-1]) if step else 0
        held = {}
        for e in range(b):
            if is_drum[e]:
                continue
            if bin_of(velbin[e]):
                held[(program[e] & 127, pitch[e] & 127)] = True
            else:
                held.pop((program[e] & 127, pitch[e] & 127), None)
        for p, q in sorted(held):
            put_program(p, "tie program")
            put(rule.pitch_first + q, "tie pitch")
        put(rule.tie_id, "tie")
    prev = 0
    for e in range(len(step)):                                       # item 2
        if not step_lo <= step[e] < step_hi:
            continue
        d, v, drum = step[e] - step_lo, bin_of(velbin[e]), bool(ties and is_drum[e])
        if d > prev:
            for _ in range(d // rule.max_shift_steps):
                put(rule.shift_first + rule.max_shift_steps, "shift", e)
            if d % rule.max_shift_steps:
                put(rule.shift_first + d % rule.max_shift_steps, "shift", e)
        prev = d
        if ties and not drum:
            put_program(program[e], "program", e)
        if v != last["velocity"]:
            put(rule.velocity_first + v, "velocity", e)
        last["velocity"] = v
        put((rule.drum_first if drum else rule.pitch_first) + (pitch[e] & 127), "drum" if drum else "pitch", e, note[e],
            int(v != 0))
    put(1, "eos")                                                    # item 5, first half
    return ids, note_of, is_onset, trace


def restated(rule, ev, step_lo, step_hi, stride):
    """`restate_row`, cut to `stride` and padded: ids, note_of, is_onset, length, truncated"""
    ids, note_of, is_onset, _ = restate_row(rule, ev, step_lo, step_hi)
    n, pad = min(len(ids), stride), max(stride - len(ids), 0)
    return ids[:n] + [0] * pad, note_of[:n] + [-1] * pad, is_onset[:n] + [0] * pad, n, int(len(ids) > stride)


def host_row(rule, ev, step_lo, step_hi, stride):
    """the same through mt3_notes_tokenize"""
    ev = np.ascontiguousarray(ev)
    ids, note_of, is_onset = np.zeros(stride, np.int32), np.zeros(stride, np.int32), np.zeros(stride, np.uint8)
    length, cut = C.c_int32(), C.c_int32()
    ptr = [ev[k].ctypes.data for k in range(6)] if ev.shape[1] else [None] * 6
    _lib.check(_lib.load().mt3_notes_tokenize(C.byref(rule), *ptr, ev.shape[1], int(step_lo), int(step_hi), stride,
                                              ids.ctypes.data, note_of.ctypes.data, is_onset.ctypes.data, C.byref(length),
                                              C.byref(cut)))
    return ids, note_of, is_onset, length.value, cut.value


# ------------------------------------------------------------------------------------------- the tables, read in Python
def file_events(case, f):
    """the events of file f: a range that leaves [0, n_events] counts as empty"""
    e0, n, total = int(case.files[f]["event0"]), int(case.files[f]["n_events"]), case.events.shape[1]
    if e0 < 0 or n < 0 or e0 + n > total:
        e0, n = 0, 0
    return case.events[:, e0: e0 + n]


def rows_of(case, f):
    """the rows file f writes: those of its range that the row table gives to it, in order"""
    r0, n = int(case.files[f]["row0"]), int(case.files[f]["n_rows"])
    if r0 < 0 or n < 0 or r0 + n > len(case.rows):
        return []
    return [r for r in range(r0, r0 + n) if case.rows[r]["file"] == f]


def owner(case, row):
    """the file that writes `row`, or None"""
    f = int(case.rows[row]["file"])
    return f if 0 <= f < len(case.files) and row in rows_of(case, f) else None


SENTINEL = -77


def expected(case, stride, row_fn):
    """What a launch must leave in output arrays that held SENTINEL everywhere (is_onset: SENTINEL & 255): the rows
    through `row_fn` (`host_row` or `restated`), every row that no file writes untouched."""
    n = len(case.rows)
    out = dict(ids=np.full((n, stride), SENTINEL, np.int32), lengths=np.full(n, SENTINEL, np.int32),
               truncated=np.full(n, SENTINEL, np.int32), note_of=np.full((n, stride), SENTINEL, np.int32),
               is_onset=np.full((n, stride), SENTINEL & 255, np.uint8))
    for row in range(n):
        f = owner(case, row)
        if f is not None:
            seg = case.rows[row]
            out["ids"][row], out["note_of"][row], out["is_onset"][row], out["lengths"][row], out["truncated"][row] = \
                row_fn(case.rule, file_events(case, f), int(seg["step_lo"]), int(seg["step_hi"]), stride)
    return out


def _tie_begin(step, step_lo):
    b = int(np.searchsorted(step, step_lo, side="left"))
    if b < len(step) or not len(step):
        return b
    return int(np.searchsorted(step, step[-1], side="left"))


def _ranges(case, row):
    """(events of the row's file, advance origin, tie begin, first event, end of events) of a written row"""
    f = owner(case, row)
    assert f is not None, "row %d is written by no file" % row
    ev, mine = file_events(case, f), rows_of(case, f)
    before = mine[mine.index(row) - 1] if mine.index(row) else None
    origin = _tie_begin(ev[0], int(case.rows[before]["step_lo"])) if before is not None else 0
    lo, hi = int(case.rows[row]["step_lo"]), int(case.rows[row]["step_hi"])
    e_lo = int(np.searchsorted(ev[0], lo, side="left"))
    e_hi = max(e_lo, int(np.searchsorted(ev[0], hi, side="left"))) if hi > lo else e_lo
    return ev, origin, _tie_begin(ev[0], lo), e_lo, e_hi


def observe(case, kind, row, subject):
    """What the tables say about a claim.  Events are indices within the row's file.
      advance / events, event     (tile, lane) of the event in the row's advance / event tiles, None outside them
      writers, (program, pitch)   [(tile, lane, set)] of the pair's writers in the row's advance, drums left out
      held, (program, pitch)      whether the row's tie section declares the pair
      tie section, None           the tie section as [('program', m) | ('pitch', q)]
      program id / velocity id, event   whether the event writes one;   shift ids, event   the values it writes
      cut, stride                 what stands at position stride - 1 of the uncut row (the last id kept): (kind, event),
                                  ('pad', -1) past the EOS
      written, None               whether any file writes the row"""
    if kind == "written":
        return owner(case, row) is not None
    ev, origin, b, e_lo, e_hi = _ranges(case, row)
    if kind == "advance":
        return divmod(subject - origin, TILE) if origin <= subject < b else None
    if kind == "events":
        return divmod(subject - e_lo, TILE) if e_lo <= subject < e_hi else None
    if kind == "writers":
        return [divmod(e - origin, TILE) + (int(case.rule_bin(ev[3, e]) != 0),) for e in range(origin, b)
                if not ev[4, e] and (ev[2, e] & 127, ev[1, e] & 127) == subject]
    if kind == "held":
        return subject in _held(ev, b, case)
    seg, r = case.rows[row], case.rule
    ids, _, _, trace = restate_row(r, ev, int(seg["step_lo"]), int(seg["step_hi"]))
    n_tie = [k for k, _ in trace].index("tie")
    if kind == "tie section":
        return [("program", i - r.program_first) if k == "tie program" else ("pitch", i - r.pitch_first)
                for i, (k, _) in zip(ids[:n_tie], trace[:n_tie])]
    if kind in ("program id", "velocity id"):
        return (kind[:-3], subject) in trace
    if kind == "shift ids":
        return [i - r.shift_first for i, t in zip(ids, trace) if t == ("shift", subject)]
    if kind == "cut":
        return trace[subject - 1] if subject - 1 < len(trace) else ("pad", -1)
    raise ValueError(kind)


def _held(ev, b, case):
    table = {}
    for e in range(b):
        if not ev[4, e]:
            table[(int(ev[2, e]) & 127, int(ev[1, e]) & 127)] = case.rule_bin(ev[3, e]) != 0
    return {pair for pair, on in table.items() if on}


# ------------------------------------------------------------------------------------------------------- builders
_CODECS = {}


def codec_of(bins=1, max_shift_seconds=10):
    key = (bins, max_shift_seconds)
    if key not in _CODECS:
        _CODECS[key] = vocabularies.build_codec(vocabularies.VocabularyConfig(max_shift_seconds=max_shift_seconds,
                                                                              num_velocity_bins=bins))
    return _CODECS[key]


def rule_of(granularity="full", bins=1, max_shift_steps=None, program_map=None):
    r = tokenize.tokenize_rule(codec_of(bins), TIES, None, granularity)
    if max_shift_steps is not None:
        r.max_shift_steps = max_shift_steps
    for p, m in (program_map or {}).items():
        r.program_map[p] = m
    return r


def E(step, pitch, program=0, vel=1, drum=0):
    return (step, pitch, program, vel, drum)


def columns(events):
    """int32 [6, n] of (step, pitch, program, velbin, is_drum) tuples; note = 5000 + 3 * index"""
    ev = np.zeros((6, len(events)), np.int32)
    if events:
        ev[:5] = np.asarray(events, np.int64).T
    ev[5] = 5000 + 3 * np.arange(len(events))
    assert (np.diff(ev[0]) >= 0).all(), "steps ascend within a file"
    return ev


def one_file(name, events, segments, rule, strides, claims):
    files = np.zeros(1, tokenize.FILE_DTYPE)
    files[0] = (0, len(events), 0, len(segments), 0)
    rows = np.zeros(len(segments), tokenize.ROW_DTYPE)
    rows["step_lo"], rows["step_hi"] = [s[0] for s in segments], [s[1] for s in segments]
    return Case(name, columns(events), files, rows, rule, tuple(strides), claims)


def from_sequences(name, sequences, frames, strides, claims, granularity="full", segment_frames=256, max_shift_seconds=10):
    """a case the recipe can be asked about: the planner's own events and tables of NoteSequences under a stock codec"""
    codec = codec_of(1, max_shift_seconds)
    job = tokenize.plan(sequences, frames, codec, TIES, granularity, max(strides), segment_frames=segment_frames)
    return Case(name, job.packed.events, job.files, job.rows, job.rule, tuple(strides), claims,
                dict(sequences=sequences, frames=frames, codec=codec, granularity=granularity, segment_frames=segment_frames))


def bundle(name, cases):
    """the files of `cases` (one rule, one set of strides) as ONE job: a workgroup and a held table per file"""
    first = cases[0]
    assert all(bytes(c.rule) == bytes(first.rule) and c.strides == first.strides for c in cases)
    files, rows, claims, e0, r0 = [], [], [], 0, 0
    for c in cases:
        f, r = c.files.copy(), c.rows.copy()
        f["event0"] += e0
        f["row0"] += r0
        r["file"] += sum(len(x) for x in files)
        claims += [(k, row + r0, s, v) for k, row, s, v in c.claims]
        files.append(f), rows.append(r)
        e0, r0 = e0 + c.events.shape[1], r0 + len(c.rows)
    return Case(name, np.ascontiguousarray(np.concatenate([c.events for c in cases], axis=1)), np.concatenate(files),
                np.concatenate(rows), first.rule, first.strides, claims)


def split(case):
    """one job per file over the same outputs: file f alone as file 0 of its launch, every other row foreign"""
    jobs = []
    for f in range(len(case.files)):
        rows = case.rows.copy()
        rows["file"] = np.where(case.rows["file"] == f, 0, -1)
        jobs.append(dataclasses.replace(case, files=case.files[f: f + 1].copy(), rows=rows, claims=[]))
    return jobs


def _filler(i):
    """a write to a pair of programs 1 .. 3 at step i: mostly offsets, every fifth an onset"""
    return E(i, (7 * i) % 128, 1 + i % 3, 1 if i % 5 == 0 else 0)


def _advance(name, n, script, done, claims_of):
    """n fillers at steps 0 .. n - 1 with `script` {event: (pair, velbin, is_drum)} written over them, then two events
    at step n.  done = 0: one row at step n, its advance starting at event 0; otherwise a first row whose tie begin is
    event `done`, so that the second row's advance tiles start there."""
    events = [_filler(i) for i in range(n)] + [E(n, 30, 2), E(n + 1, 30, 2, 0)]
    for e, ((program, pitch), vel, drum) in script.items():
        events[e] = E(e, pitch, program, vel, drum)
    segments = [(n, INT32_MAX)] if not done else [(done, done + 3), (n, INT32_MAX)]
    return one_file(name, events, segments, rule_of(), (512,), claims_of(len(segments) - 1))


def advance_cases():
    out = []
    for done in (0, 37):
        a, b = done + 255, done + 256
        out.append(_advance("advance, split pair: onset in lane 255, offset in lane 0, done = %d" % done, done + 300,
                            {a: (X, 1, 0), b: (X, 0, 0)}, done,
                            lambda row, a=a, b=b: [("advance", row, a, (0, 255)), ("advance", row, b, (1, 0)),
                                                   ("writers", row, X, [(0, 255, 1), (1, 0, 0)]), ("held", row, X, False)]))
        out.append(_advance("advance, split pair: offset in lane 255, onset in lane 0, done = %d" % done, done + 300,
                            {done + 5: (X, 1, 0), a: (X, 0, 0), b: (X, 1, 0)}, done,
                            lambda row, a=a, b=b: [("advance", row, a, (0, 255)), ("advance", row, b, (1, 0)),
                                                   ("writers", row, X, [(0, 5, 1), (0, 255, 0), (1, 0, 1)]),
                                                   ("held", row, X, True)]))
    out.append(_advance("advance, stale key: set by lane 200, a tile without it, cleared by lane 3", 600,
                        {200: (X, 1, 0), 515: (X, 0, 0)}, 0,
                        lambda row: [("writers", row, X, [(0, 200, 1), (2, 3, 0)]), ("held", row, X, False)]))
    out.append(_advance("advance, stale key: cleared by lane 200, a tile without it, set by lane 3", 600,
                        {5: (X, 1, 0), 200: (X, 0, 0), 515: (X, 1, 0)}, 0,
                        lambda row: [("writers", row, X, [(0, 5, 1), (0, 200, 0), (2, 3, 1)]), ("held", row, X, True)]))
    out.append(_advance("advance, stale key: four writes in one tile, the last an onset", 300,
                        {10: (X, 1, 0), 50: (X, 0, 0), 90: (X, 0, 0), 130: (X, 1, 0)}, 0,
                        lambda row: [("writers", row, X, [(0, 10, 1), (0, 50, 0), (0, 90, 0), (0, 130, 1)]),
                                     ("held", row, X, True)]))
    y, z, w = (5, 64), (5, 70), (5, 65)                                # pairs 704, 710, 705: one word of the held table
    assert len({(p * 128 + q) >> 5 for p, q in (y, z, w)}) == 1
    out.append(_advance("advance, two winners in one word: one sets, one clears", 300,
                        {20: (z, 1, 0), 21: (w, 1, 0), 256 + 7: (y, 1, 0), 256 + 9: (z, 0, 0)}, 0,
                        lambda row: [("writers", row, y, [(1, 7, 1)]), ("writers", row, z, [(0, 20, 1), (1, 9, 0)]),
                                     ("held", row, y, True), ("held", row, z, False), ("held", row, w, True)]))
    x2 = (9, 65)
    out.append(_advance("advance, a drum on the last writer's numbers does not count", 300,
                        {100: (X, 1, 0), 150: (X, 0, 1), 20: (x2, 1, 0), 120: (x2, 0, 0), 180: (x2, 1, 1)}, 0,
                        lambda row: [("writers", row, X, [(0, 100, 1)]), ("writers", row, x2, [(0, 20, 1), (0, 120, 0)]),
                                     ("held", row, X, True), ("held", row, x2, False)]))
    return out


def split_pair_as_notes(reverse):
    """the split pair at done = 0 as a NoteSequence, one event per step: segments of 512 frames put the second row's tie
    begin at step 409, so its advance starts at event 0 and event 255 / 256 are lane 255 / lane 0"""
    at = lambda k: k / 100.0                                           # noqa: E731
    notes = [Note(at(2 * k), at(2 * k + 1), 20 + k % 100, 100, 1 + k % 3, False, 0) for k in range(127) if not (reverse and k == 5)]
    notes += [Note(at(254), 20.0, 30, 100, 4, False, 0)]
    notes += [Note(at(257 + 2 * k), at(258 + 2 * k), 20 + k, 100, 1, False, 0) for k in range(20)]
    if reverse:
        notes += [Note(at(10), at(255), X[1], 100, X[0], False, 0), Note(at(11), 20.0, 31, 100, 4, False, 0),
                  Note(at(256), 20.0, X[1], 100, X[0], False, 0)]
        writers = [(0, 10, 1), (0, 255, 0), (1, 0, 1)]
    else:
        notes += [Note(at(255), at(256), X[1], 100, X[0], False, 0)]
        writers = [(0, 255, 1), (1, 0, 0)]
    claims = [("advance", 1, 255, (0, 255)), ("advance", 1, 256, (1, 0)), ("writers", 1, X, writers), ("held", 1, X, reverse)]
    return from_sequences("advance, split pair as notes: %s" % ("offset, then onset" if reverse else "onset, then offset"),
                          [NoteSequence(notes=notes)], [1024], (1024,), claims, segment_frames=512)


def _held_then(name, held, after, rule, stride, claims):
    """onsets of the pairs `held`, two to a step from step 0, one row at step 100 whose events are `after` (tuples without step, one
    step apart from step 105 on)"""
    events = [E(i // 2, q, p) for i, (p, q) in enumerate(held)]
    events += [E(105 + i, *a) for i, a in enumerate(after)]
    return one_file(name, events, [(100, INT32_MAX)], rule, (stride,), claims), len(held)


def tie_cases():
    out = []
    section = [("program", 0), ("pitch", 60), ("pitch", 62), ("program", 8), ("pitch", 64)]
    out.append(_held_then("tie section, midi_class: rows 0 and 3 share a class, 9 opens its own",
                          [(0, 60), (3, 62), (9, 64)], [(70, 20)], rule_of("midi_class"), 64,
                          [("tie section", 0, None, section)])[0])
    notes = [Note(0.1, 9.0, 60, 100, 0, False, 0), Note(0.2, 9.0, 62, 100, 3, False, 0), Note(0.3, 9.0, 64, 100, 9, False, 0),
             Note(2.5, 2.6, 70, 100, 20, False, 0)]
    out.append(from_sequences("tie section, midi_class, as notes", [NoteSequence(notes=notes)], [512], (64,),
                              [("tie section", 1, None, section)], granularity="midi_class"))
    partial = {4: 4, 5: -1, 6: 4}
    out.append(_held_then("tie section, custom map: row 5 = -1 between rows 4 and 6, both mapped to 4",
                          [(4, 60), (5, 61), (6, 62)], [(70, 20)], rule_of(program_map=partial), 64,
                          [("tie section", 0, None, [("program", 4), ("pitch", 60), ("pitch", 61), ("pitch", 62)])])[0])
    held = [(0, 60), (33, 50), (40, 70)]
    case, n = _held_then("seam: the last held row's program is the first event's", held, [(65, 40), (66, 33)], rule_of(), 64,
                         [("program id", 0, 3, False), ("program id", 0, 4, True)])
    out.append(case)
    case, n = _held_then("seam: two drums before the first pitched event", held,
                         [(36, 0, 1, 1), (38, 0, 1, 1), (65, 40), (66, 33)], rule_of(), 64,
                         [("program id", 0, 5, False), ("program id", 0, 6, True)])
    out.append(case)
    drums = [(35 + i % 40, 0, i % 2, 1) for i in range(256)]
    case, n = _held_then("seam: event tile 0 all drums, the first mapped event is lane 0 of tile 1", held,
                         drums + [(65, 40), (66, 33)], rule_of(), 1024,
                         [("events", 0, 3 + 256, (1, 0)), ("events", 0, 3 + 255, (0, 255)),
                          ("program id", 0, 3 + 256, False), ("program id", 0, 3 + 257, True)])
    out.append(case)
    wide = [(7, q) for q in range(20, 100, 2)] + [(8, 33)]
    out.append(_held_then("tie section: a row of 40 pitches, more than one word", wide, [(70, 8)], rule_of(), 128,
                          [("tie section", 0, None, [("program", 7)] + [("pitch", q) for q in range(20, 100, 2)] +
                            [("program", 8), ("pitch", 33)]), ("program id", 0, len(wide), False)])[0])
    every = [(p, (5 * p) % 128) for p in range(128)]
    out.append(_held_then("tie section: 128 programs of one pitch, every lane below 128 writes", every, [(70, 127)],
                          rule_of(), 512,
                          [("tie section", 0, None, [x for p, q in every for x in (("program", p), ("pitch", q))]),
                           ("program id", 0, 128, False)])[0])
    return out


# per map: the program before the edge, one after it that must NOT write an id, one that must
CARRY_MAPS = {"full": (dict(), 17, 17, 18), "midi_class": (dict(granularity="midi_class"), 17, 18, 24),
              "partial": (dict(program_map={18: 17, **{p: -1 for p in range(40, 48)}}), 17, 18, 19)}


def carry_cases():
    """530 events in one row, three event tiles; the tile edge under test is event 256 (512 for the tile of drums)"""
    out = []
    for map_name, (kw, before, same, other) in CARRY_MAPS.items():
        for variant in ("same", "drums before the edge", "different", "a tile of drums"):
            ev = [E(i // 3, 30 + i % 60, (before, 60, 61)[(i // 7) % 3], i % 2, int(i % 11 == 0)) for i in range(530)]

            def put(i, program, drum=0):
                ev[i] = E(i // 3, 30 + i % 60, program, i % 2, drum)

            last, edge, writes = 255, 256, variant == "different"
            if variant == "drums before the edge":
                last = 249
                for i in range(250, 256):                            # the partial map: unmapped programs count as drums do
                    put(i, 41, 0) if map_name == "partial" and i >= 253 else put(i, 0, 1)
            if variant == "a tile of drums":
                edge = 512
                for i in range(256, 512):
                    put(i, same, 1)
            put(last, before)
            put(edge, other if writes else same)
            put(edge + 1, 60)
            claims = [("events", 0, 255, (0, 255)), ("events", 0, edge, (edge // 256, 0)), ("events", 0, 529, (2, 17)),
                      ("program id", 0, last, _writes_before(ev, last, before)),
                      ("program id", 0, edge, writes), ("program id", 0, edge + 1, True)]
            out.append(one_file("events, program carry, %s: %s" % (map_name, variant), ev, [(0, INT32_MAX)],
                                rule_of(**kw), (4096,), claims))
    return out


def _writes_before(ev, last, before):
    """whether event `last` (program `before`, mapped to itself by every map of CARRY_MAPS) writes its id: it does unless
    the pitched event before it, drums skipped, has the same program.  Background programs are 17, 60, 61: all mapped."""
    for e in range(last - 1, -1, -1):
        if not ev[e][4]:
            return ev[e][2] != before
    return True


def edge_cases():
    """300 events in one row, 127 velocity bins: the velocity id and the shift id of lane 0 of tile 1 depend on event 255"""
    out = []
    for equal in (True, False):
        for rises in (True, False):
            inc = [1 if i % 4 == 0 else 0 for i in range(300)]
            inc[254], inc[255], inc[256], inc[257] = 1, 0, int(rises), 1
            step = np.cumsum(inc) + 3
            vel = [(5 * i) % 128 for i in range(300)]
            vel[255], vel[256], vel[257] = 77, 77 if equal else 78, 20
            ev = [E(int(step[i]), 30 + i % 60, (i // 9) % 4, vel[i]) for i in range(300)]
            claims = [("events", 0, 255, (0, 255)), ("events", 0, 256, (1, 0)), ("velocity id", 0, 256, not equal),
                      ("shift ids", 0, 255, []), ("shift ids", 0, 256, [int(step[256])] if rises else []),
                      ("shift ids", 0, 257, [int(step[257])])]
            out.append(one_file("events, tile edge: velocity %s, step %s" % ("equal" if equal else "unequal",
                                                                             "rises at lane 0" if rises else "does not rise"),
                                ev, [(0, INT32_MAX)], rule_of(bins=127), (2048,), claims))
    return out


def shift_cases():
    steps = [6, 7, 8, 14, 15, 204]
    ev = [E(s, 60 + i, i % 2, 1 - i % 2) for i, s in enumerate(steps)]
    ev += [E(305, 50, 3), E(305, 52, 3), E(409, 50, 3, 0)]
    stated = [[6], [7], [7, 1], [7, 7], [7, 7, 1], [7] * 29 + [1], [7] * 14 + [2], [], [7] * 29 + [1]]
    out = [one_file("several shift ids: max_shift_steps = 7 on rows of 205 steps", ev, [(0, 205), (205, 410), (410, INT32_MAX)],
                    rule_of(max_shift_steps=7), (256,),
                    [("shift ids", 0 if e < 6 else 1, e, v) for e, v in enumerate(stated)])]
    # the same through the codec of max_shift_seconds = 1: ids of 100 steps, rows at steps 0, 204 and 409
    starts = [0.99, 1.00, 1.01, 2.00, 2.01]
    notes = [Note(t, 2.03, 60 + i, 100, i % 2, False, 0) for i, t in enumerate(starts)]
    notes += [Note(3.50, 5.0, 50, 100, 3, False, 0), Note(3.50, 5.0, 52, 100, 3, False, 0)]
    stated = [[99], [100], [100, 1], [100, 100], [100, 100, 1]]
    claims = [("shift ids", 0, e, v) for e, v in enumerate(stated)] + [("shift ids", 0, 5, [100, 100, 3]), ("shift ids", 0, 6, []),
                                                                      ("shift ids", 1, 10, [100, 46]), ("shift ids", 1, 11, [])]
    out.append(from_sequences("several shift ids: the codec of max_shift_seconds = 1", [NoteSequence(notes=notes)], [3 * 256],
                              (256,), claims, max_shift_seconds=1))
    return out


CUT_KINDS = ["tie program", "tie pitch", "tie pitch"] * 3 + ["tie"] + ["shift"] * 3 + ["program", "velocity", "pitch"] + \
    ["shift"] * 3 + ["pitch"]


def cut_case():
    """Row 1: a tie section of six pairs in three program rows, a first event of 3 shift ids + program + velocity + pitch,
    a second of 3 shift ids + pitch, then the offsets.  Run at every stride from 2 to 21, and around the row's own end:
    with `base` ids before the EOS, strides base - 1 and base are the truncated rows, base + 1 the last that keeps its EOS
    (in its last position), base + 2 the first with padding.  The second file is the first one's notes again: the same
    rows from another workgroup."""
    held = [Note(0.1, 9.0, q, 100, p, False, 0) for p, q in ((0, 60), (0, 62), (33, 50), (33, 52), (40, 70), (40, 72))]
    ns = NoteSequence(notes=held + [Note(4.06, 9.0, 65, 100, 8, False, 0), Note(4.07, 9.0, 66, 100, 8, False, 0)])
    probe = from_sequences("probe", [ns, ns], [512, 512], (4096,), [], max_shift_seconds=1)
    base = int(host_row(probe.rule, file_events(probe, 0), 204, INT32_MAX, 4096)[3]) - 1
    strides = tuple(range(2, 22)) + (base - 1, base, base + 1, base + 2)
    claims = [("cut", 1, s, (CUT_KINDS[s - 1], 6 if 11 <= s <= 16 else 7 if s >= 17 else -1)) for s in range(2, 21)]
    claims += [("cut", 1, base, ("pitch", 15)), ("cut", 1, base + 1, ("eos", -1)), ("cut", 1, base + 2, ("pad", -1))]
    claims += [("tie section", 3, None, [("program", 0), ("pitch", 60), ("pitch", 62), ("program", 33), ("pitch", 50),
                                         ("pitch", 52), ("program", 40), ("pitch", 70), ("pitch", 72)])]
    return from_sequences("the cut at every kind of position", [ns, ns], [512, 512], strides, claims, max_shift_seconds=1), base


def tables_case():
    """Tables the planner never builds.  Files: 0 and 1 with overlapping row ranges (each sees rows of the other), 2 with
    n_rows = 0 over rows 7 and 8, 3 an empty file of three rows, 4 with event0 = n_events + 5 (counts as empty).  File 0:
    two rows with one step_lo, a row with step_hi <= step_lo, a row past the last event; events with pitch 200, program
    -3, velbin -1 and 500.  Row 14 names file 0 but lies outside its range."""
    a = [E(0, 60, 0, 5), E(1, 200, 0, 90), E(2, 62, -3, 500), E(3, 60, 0, -1), E(5, 200, 0, 0), E(5, 64, 2, 127),
         E(6, 36, 0, 9, 1), E(7, 62, 125, 0), E(8, 66, 2, 128), E(9, 64, 2, 0), E(12, 70, 1, 3), E(12, 71, 1, 3)]
    b = [E(1, 50, 4, 1), E(2, 51, 4, 1), E(3, 50, 4, 0), E(4, 52, 5, 1), E(4, 53, 5, 1), E(6, 51, 4, 0), E(7, 52, 5, 0),
         E(9, 54, 5, 1)]
    events = np.ascontiguousarray(np.concatenate([columns(a), columns(b)], axis=1))
    n = events.shape[1]
    files = np.zeros(5, tokenize.FILE_DTYPE)
    files[0], files[1], files[2] = (0, len(a), 0, 7, 0), (len(a), len(b), 1, 4, 0), (0, len(a), 7, 0, 0)
    files[3], files[4] = (n, 0, 9, 3, 0), (n + 5, 4, 12, 2, 0)
    table = [(0, 0, 5), (1, 0, 4), (0, 5, 9), (0, 5, 9), (1, 4, INT32_MAX), (0, 9, 3), (0, 1000, INT32_MAX),
             (2, 0, 5), (2, 5, INT32_MAX), (3, 0, 204), (3, 204, 409), (3, 409, INT32_MAX), (4, 0, 204), (4, 204, INT32_MAX),
             (0, 0, INT32_MAX)]
    rows = np.zeros(len(table), tokenize.ROW_DTYPE)
    rows["file"], rows["step_lo"], rows["step_hi"] = zip(*table)
    claims = [("written", r, None, r not in (7, 8, 14)) for r in range(len(table))]
    claims += [("advance", 3, 4, None), ("events", 5, 9, None), ("events", 6, 10, None),           # b == done; no events
               ("held", 6, (1, 70), False), ("held", 6, (125, 62), False), ("held", 2, (0, 72), True)]
    return Case("tables the planner never builds", events, files, rows, rule_of(bins=127), (32,), claims)


_ALL = []


def all_cases():
    """every case, built once and left unchanged"""
    if not _ALL:
        advance = advance_cases()
        _ALL.extend(advance + [bundle("advance: every case above as one job of files", advance)] + tie_cases() +
                    [split_pair_as_notes(False), split_pair_as_notes(True)] + carry_cases() + edge_cases() + shift_cases() + [cut_case()[0], tables_case()])
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL
