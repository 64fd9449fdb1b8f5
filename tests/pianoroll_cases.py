"""Hand-computed piano rolls and frame counts, shared by tests/test_pianoroll_ref.py (which pins the numpy restatement
with them) and tests/test_gpu_pianoroll.py (which sends them through the device)."""
import numpy as np

from mt3_amd.note_sequences import Note, NoteSequence


def ns_of(*notes):
    return NoteSequence(notes=[Note(*n) for n in notes])


def roll_of(width, *runs):
    """float64 [128, width] with `velocity` in roll[pitch, first:last] for every (pitch, first, last, velocity)"""
    roll = np.zeros((128, width), np.float64)
    for pitch, first, last, velocity in runs:
        roll[pitch, first:last] = velocity
    return roll


# (name, sequence, fps, is_drum, the roll worked out by hand)        Note(start, end, pitch, velocity, program, is_drum)
ROLL_CASES = [
    # 1.02 - 1.0 < 0.05: the note ends at 1.05; frames int(100.0) = 100 up to int(105.0...) = 105, which is also the width
    ("short note becomes 0.05 s", ns_of((1.0, 1.02, 60, 80)), 100.0, False, roll_of(105, (60, 100, 105, 80))),
    # 0.29 * 100 = 28.999999999999996 in float64: frame 28, not 29
    ("truncation of 0.29 * 100", ns_of((0.29, 0.5, 60, 80)), 100.0, False, roll_of(50, (60, 28, 50, 80))),
    ("two programs on one pitch sum", ns_of((0.0, 1.0, 60, 50, 0), (0.5, 1.0, 60, 70, 40)), 10.0, False,
     roll_of(10, (60, 0, 5, 50), (60, 5, 10, 120))),
    # the drum note lasts until 2.0 s: 200 frames wide, but it renders as zeros
    ("drum note widens the roll and stays silent", ns_of((0.0, 0.5, 60, 100), (1.0, 2.0, 36, 90, 0, True)), 100.0, False,
     roll_of(200, (60, 0, 50, 100))),
    # is_drum: every note 0.05 s long, the drum flag ignored: 0 .. 0.05 and 1.0 .. 1.05
    ("is_drum renders every note at 0.05 s", ns_of((0.0, 0.5, 60, 100), (1.0, 2.0, 36, 90, 0, True)), 100.0, True,
     roll_of(105, (60, 0, 5, 100), (36, 100, 105, 90))),
    # int(1.01) == int(1.52) == 1: an empty slice; the width is int(1.52) = 1
    ("coinciding indices add nothing", ns_of((0.101, 0.152, 60, 80)), 10.0, False, roll_of(1)),
    ("an empty sequence", ns_of(), 62.5, False, roll_of(0)),
]


def _cells(width, ref=(), est=()):
    r, e = np.zeros((128, width[0]), np.float64), np.zeros((128, width[1]), np.float64)
    for (p, c), v in ref:
        r[p, c] = v
    for (p, c), v in est:
        e[p, c] = v
    return r, e


# (name, ref roll, est roll, threshold, (TP, FP, FN), (precision, recall, f1) by hand)
COUNT_CASES = [
    # ref is 3 wide, est 5: est's cell in column 4 faces padding (FP); ref's cell (60, 2) faces an est cell (TP)
    ("unequal widths", *_cells((3, 5), ref=[((60, 2), 100)], est=[((60, 2), 1), ((61, 4), 1)]), 30, (1, 1, 0),
     (0.5, 1.0, 2 * 0.5 * 1.0 / 1.5)),
    # velocity exactly 30 is off (strict >), 31 is on; est cells of 1 are on
    ("threshold is strict", *_cells((4, 4), ref=[((10, 0), 30), ((10, 1), 31)], est=[((10, 0), 1), ((10, 1), 1)]), 30,
     (1, 1, 0), (0.5, 1.0, 2 * 0.5 * 1.0 / 1.5)),
    ("all-zero est", *_cells((4, 2), ref=[((10, 0), 90), ((11, 3), 90)]), 30, (0, 0, 2), (0.0, 0.0, 0.0)),
    ("both of width 0", *_cells((0, 0)), 30, (0, 0, 0), (0.0, 0.0, 0.0)),
    # TP 3, FP 1, FN 2: P = 3/4, R = 3/5, F1 = 2 * 0.75 * 0.6 / 1.35 = 2/3
    ("worked example 3/1/2", *_cells((8, 8), ref=[((5, c), 64) for c in (0, 1, 2, 3, 4)],
                                     est=[((5, c), 64) for c in (2, 3, 4)] + [((6, 0), 20)]), 30, (3, 1, 2),
     (0.75, 0.6, 2 * 0.75 * 0.6 / (0.75 + 0.6))),
]


def random_sequence(rng, n_notes, seconds, fps, drums=True):
    """notes with programs and drums, start times on frame boundaries (k / fps), a hair beside them (+-1e-12) and anywhere"""
    notes = []
    for _ in range(n_notes):
        kind = rng.integers(0, 4)
        k = int(rng.integers(0, max(1, int(seconds * fps))))
        start = (k / fps, max(0.0, k / fps - 1e-12), k / fps + 1e-12, float(rng.uniform(0, seconds)))[kind]
        length = (float(rng.uniform(0.0, 0.04)), int(rng.integers(1, 40)) / fps, float(rng.uniform(0.05, 2.0)))[rng.integers(0, 3)]
        notes.append(Note(start, start + length, int(rng.integers(0, 128)), int(rng.integers(1, 128)),
                          int(rng.integers(0, 128)), bool(drums and rng.integers(0, 5) == 0)))
    return NoteSequence(notes=notes)
