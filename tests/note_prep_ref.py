"""Note preparation (include/mt3_hip.h, "note preparation") for the tests: hand-written cases with their
expected ends as literals, the closed form of the sustain rule in numpy (the per-note statement the kernel computes,
sharing no code with mt3_amd/note_prep.py), the host rules with every note's original position, and the jobs the device
tests run."""
import copy

import numpy as np

from mt3_amd import note_sequences as NS


def seq(notes, pedal=(), total_time=None, controls=()):
    """notes: (pitch, velocity, start, end[, instrument[, program[, is_drum]]]); pedal: (time, value[, instrument]) of
    controller 64; controls: (time, number, value[, instrument]) of any controller"""
    ns = NS.NoteSequence()
    for pitch, velocity, start, end, *rest in notes:
        instrument, program, drum = (list(rest) + [0, 0, False])[:3]
        ns.notes.append(NS.Note(start, end, pitch, velocity, program, drum, instrument))
    ns.total_time = max([n.end_time for n in ns.notes], default=0.0) if total_time is None else total_time
    for time, value, *rest in pedal:
        ns.control_changes.append(NS.ControlChange(time, 64, value, rest[0] if rest else 0))
    for time, number, value, *rest in controls:
        ns.control_changes.append(NS.ControlChange(time, number, value, rest[0] if rest else 0))
    return ns


# name -> (sequence, the expected end of every note in order, None: deleted; the expected total_time)
HAND = {
    # the two recalled from note_seq's sequences_lib_test [from memory: parity unpinned against note_seq]
    "note_seq_sustain": (seq([(11, 55, .22, .50), (40, 45, 2.50, 3.50), (55, 120, 4.0, 4.01)],
                             [(0, 127), (.75, 0), (2.0, 127), (3.0, 0), (3.75, 127), (4.5, 127), (4.8, 0), (4.9, 127),
                              (6.0, 0)]), [.75, 3.50, 4.8], 4.8),
    "note_seq_repeated_notes": (seq([(60, 100, .25, 1.50), (60, 100, 1.25, 1.50), (72, 100, 2.0, 3.50), (60, 100, 2.0, 3.0),
                                     (60, 100, 3.50, 4.50)], [(0, 127), (4.0, 0)]), [1.25, 2.0, 4.0, 3.50, 4.50], 4.50),
    # our own
    "together_under_the_pedal": (seq([(60, 100, 1.0, 1.5), (60, 90, 1.0, 1.2)], [(0, 127), (2.0, 0)]), [None, 2.0], 2.0),
    "never_released": (seq([(60, 100, 0.0, 1.0), (64, 100, 1.0, 3.0)], [(0.5, 127)], total_time=5.0), [3.0, 3.0], 3.0),
    "off_and_on_at_one_instant": (seq([(60, 100, .2, .5), (62, 100, 1.2, 1.5)], [(0, 127), (1.0, 127), (1.0, 0), (3.0, 0)]),
                                  [1.0, 1.5], 1.5),
    "another_instrument": (seq([(60, 100, 0.0, 1.0)], [(0, 127, 1), (4.0, 0, 1)]), [1.0], 1.0),
    "controller_1": (seq([(60, 100, 0.0, 1.0)], controls=[(0, 1, 127), (4.0, 1, 0)]), [1.0], 1.0),
    "values_63_and_64": (seq([(60, 100, .1, .4), (61, 100, 2.1, 2.4)], [(0, 63), (2.0, 64), (3.0, 63)]), [.4, 3.0], 3.0),
    "pedal_up_between_retriggers": (seq([(60, 100, .1, 2.8), (60, 100, 1.5, 1.7), (60, 100, 2.5, 2.6)],
                                        [(0, 127), (1.0, 0), (2.0, 127), (4.0, 0)]), [2.5, 1.7, 4.0], 4.0),
    "no_notes": (seq([], [(0, 127), (1.0, 0)]), [], 0.0),
    "two_instruments_opposite_pedals": (seq([(60, 100, 0.0, 1.0, 0), (60, 100, 0.0, 1.0, 1), (60, 100, 2.5, 3.0, 0),
                                             (60, 100, 2.5, 3.0, 1)],
                                            [(0, 127, 0), (0, 0, 1), (2.0, 0, 0), (2.0, 127, 1), (4.0, 127, 0), (4.0, 0, 1)]),
                                        [2.0, 1.0, 3.0, 4.0], 4.0),
}


def _tagged(ns):
    out = copy.deepcopy(ns)
    for i, n in enumerate(out.notes):
        n.pos = i                                    # an attribute deepcopy carries along: the note's original position
    return out


def host_rule(ns, mode):
    """the host yardstick on `ns` with every survivor's original position: (src int64, end f64, total_time)"""
    rule = NS.apply_sustain_control_changes if mode == "sustain" else NS.trim_overlapping_notes
    out = rule(_tagged(ns))
    return (np.array([n.pos for n in out.notes], np.int64), np.array([n.end_time for n in out.notes], np.float64),
            float(out.total_time))


def closed_form(ns):
    """Section 3 of the issue / DESIGN 6p in numpy: every note on its own -> (src int64, end f64, total_time)"""
    n = len(ns.notes)
    start = np.array([x.start_time for x in ns.notes], np.float64)
    end = np.array([x.end_time for x in ns.notes], np.float64)
    inst = np.array([x.instrument for x in ns.notes], np.int64)
    pitch = np.array([x.pitch for x in ns.notes], np.int64)
    cc = [c for c in ns.control_changes if c.control_number == 64]
    c_time = np.array([c.time for c in cc], np.float64)
    c_inst = np.array([c.instrument for c in cc], np.int64)
    c_off = np.array([c.control_value < 64 for c in cc], bool)
    t_last = float(np.concatenate([start, end, c_time]).max()) if n + len(cc) else 0.0
    new_end, keep = end.copy(), np.ones(n, bool)
    total, took_last = float(ns.total_time), False
    for g in np.unique(inst):
        by = np.lexsort((c_off[c_inst == g], c_time[c_inst == g]))             # (time, ON before OFF)
        p_time, p_off = c_time[c_inst == g][by], c_off[c_inst == g][by]
        off_times = p_time[p_off]

        def ped(t):
            k = np.searchsorted(p_time, t, "right")
            return (k > 0) & ~p_off[np.maximum(k - 1, 0)] if len(p_time) else np.zeros(np.shape(t), bool)

        def rel(t):
            k = np.searchsorted(off_times, t, "right")
            return np.where(k < len(off_times), np.append(off_times, np.inf)[k], np.inf)      # inf: none

        for p in np.unique(pitch[inst == g]):
            run = np.nonzero((inst == g) & (pitch == p))[0]
            run = run[np.lexsort((run, start[run]))]                           # (start, position)
            flagged = ped(start[run])
            after = np.where(flagged, np.arange(len(run)), len(run))
            nxt = np.minimum.accumulate(np.append(after, len(run))[::-1])[::-1][1:]      # first flagged later note
            has_j = nxt < len(run)
            s_j = np.where(has_j, start[run][np.minimum(nxt, len(run) - 1)], np.inf)
            s, e = start[run], end[run]
            down, r = ped(e), rel(e)
            cut = has_j & np.where(down, s_j < r, s_j <= e)
            hold = ~cut & down
            new_end[run] = np.where(cut, s_j, np.where(hold, np.where(np.isinf(r), t_last, r), e))
            keep[run] = ~(cut & (s_j == s))
            took_last |= bool((hold & np.isinf(r)).any())
            total = max([total] + r[hold & ~np.isinf(r)].tolist())
    return np.nonzero(keep)[0], new_end[keep], t_last if took_last else total


def random_sequence(rng, n_notes=None, n_pedal=None, span=12):
    """the family the closed form was derived on: 1-2 instruments, 1-3 pitches, integer times so that ties are dense, one
    in five with zero-length notes, controllers other than 64 mixed in"""
    instruments, pitches = int(rng.integers(1, 3)), int(rng.integers(1, 4))
    zero_length = rng.integers(5) == 0
    n_notes = int(rng.integers(0, 9)) if n_notes is None else n_notes
    n_pedal = int(rng.integers(0, 9)) if n_pedal is None else n_pedal
    notes = []
    for _ in range(n_notes):
        start = int(rng.integers(0, span))
        length = int(rng.integers(0 if zero_length else 1, 5))
        notes.append((60 + int(rng.integers(pitches)), int(rng.integers(1, 128)), float(start), float(start + length),
                      int(rng.integers(instruments)), int(rng.integers(2)), False))
    controls = [(float(rng.integers(0, span + 4)), 64 if rng.integers(4) else int(rng.choice([1, 66, 67])),
                 int(rng.choice([0, 63, 64, 127])), int(rng.integers(instruments))) for _ in range(n_pedal)]
    return seq(notes, controls=controls, total_time=float(rng.integers(0, span + 8)))


def run_of_600():
    """one (instrument, pitch) run of 600 notes, the pedal down only under notes near the run's end: the successor that
    cuts note 0 (held until 595.0, under the pedal then) is note 591, two tile boundaries away"""
    notes = [(60, 100, float(i), 595.0 if i == 0 else i + 0.5) for i in range(600)]
    return seq(notes, [(0.25, 127), (0.75, 0), (590.75, 127), (598.25, 0), (599.4, 127)])


def long_pedal():
    """a pedal table of 700 entries with a run of 300 consecutive ON values before its OFF, under 257 notes"""
    pedal = [(i * 0.01, 64 + i % 60) for i in range(300)] + [(3.0, 0)]
    pedal += [(3.5 + i * 0.01, 127 if i % 7 else 0) for i in range(399)]
    rng = np.random.default_rng(5)
    notes = [(int(rng.integers(50, 60)), 80, float(t), float(t + rng.uniform(0.01, 0.5))) for t in rng.uniform(0, 8, 257)]
    return seq(notes, pedal)


def all_deleted():
    """zero-length notes starting together under the pedal: trim deletes every one of them, sustain all but the last of each
    pitch (the last note of a run has no successor, so sustain alone cannot delete a whole file)"""
    return seq([(60 + i % 3, 100, 1.0, 1.0) for i in range(9)], [(0, 127), (5.0, 0)])


def piano_like(rng, n_notes, n_pedal, seconds):
    """a piano-like file: random notes over `seconds`, a continuous-valued pedal going down and up every few seconds"""
    start = np.sort(rng.uniform(0, seconds, n_notes))
    notes = [(int(p), int(v), float(s), float(s + d)) for p, v, s, d in
             zip(rng.integers(21, 109, n_notes), rng.integers(1, 128, n_notes), start, rng.uniform(0.05, 1.0, n_notes))]
    t = np.sort(rng.uniform(0, seconds, n_pedal))
    value = np.clip(64 + 80 * np.sin(t * 1.7) + rng.integers(-8, 9, n_pedal), 0, 127).astype(int)
    return seq(notes, [(float(a), int(b)) for a, b in zip(t, value)])


def ragged_job():
    """one job with every shape the kernel treats differently"""
    rng = np.random.default_rng(11)
    job = [seq([]), seq([(60, 100, 0.5, 1.0)]), seq([(60, 100, 0.5, 1.0)], [(0.75, 127)])]
    job += [piano_like(rng, n, 40, 20.0) for n in (255, 256, 257, 4 * 256 + 3)]
    job += [run_of_600(), long_pedal(), all_deleted(), HAND["two_instruments_opposite_pedals"][0]]
    job += [random_sequence(rng, 300, 60, span=40) for _ in range(2)]
    return job
