"""The hand-made files of the target tokenizer's tests (tests/test_tokenize_ref.py on the host, tests/test_gpu_tokenize.py
on the device): (name, NoteSequence, n_frames) triples.  A segment is 256 frames = 2.048 s, so segment s starts at step
204.8 s: step_lo = 0, 204, 409, 614, ... (the first step whose time is past the segment's first frame, less one)."""
import numpy as np

from mt3_amd import synthetic
from mt3_amd.note_sequences import Note, NoteSequence

SEG = 256


def _ns(*notes):
    return NoteSequence(notes=[Note(float(a), float(b), int(p), int(v), int(prog), bool(drum), 0)
                               for a, b, p, v, prog, drum in notes])


def hand_made():
    # 700 short notes in segment 0: 1400 events whose velocity alternates and whose program changes every other event
    storm = [(0.2 + 0.002 * i, 0.201 + 0.002 * i, 20 + i % 100, 100, i % 2, False) for i in range(700)]
    return [
        ("empty file of 3 segments", _ns(), 3 * SEG),
        ("one segment", _ns((0.1, 0.5, 60, 100, 0, False), (0.3, 0.9, 64, 80, 0, False)), 200),
        ("one note across 3 segment starts", _ns((1.0, 7.0, 60, 100, 0, False)), 4 * SEG),
        ("struck again while sounding, released once", _ns((0.5, 5.0, 60, 100, 0, False), (1.0, 2.5, 60, 100, 0, False)), 3 * SEG),
        ("offset and onset of one pair at the same time", _ns((0.5, 3.0, 60, 100, 0, False), (3.0, 5.0, 60, 100, 0, False)), 3 * SEG),
        ("two times on one step", _ns((0.501, 1.0, 60, 100, 0, False), (0.504, 1.0, 62, 100, 0, False)), SEG),
        ("event exactly on step_lo", _ns((2.04, 2.5, 60, 100, 0, False), (2.05, 4.09, 62, 100, 0, False)), 3 * SEG),
        ("half to even", _ns((0.125, 0.3, 60, 100, 0, False), (0.375, 0.5, 62, 100, 0, False)), SEG),
        ("notes after the last frame", _ns((1.0, 2.0, 60, 100, 0, False), (5.0, 6.0, 62, 100, 0, False), (9.5, 30.0, 64, 100, 0, False)),
         2 * SEG),
        ("offset, then two silent segments", _ns((0.5, 1.0, 60, 100, 0, False), (0.7, 1.5, 64, 100, 0, False)), 3 * SEG),
        ("drum and pitched note on one pitch number", _ns((0.5, 3.0, 40, 100, 0, False), (0.5, 0.6, 40, 100, 0, True),
                                                          (2.5, 2.6, 40, 90, 0, True), (2.6, 2.7, 38, 0, 0, True)), 2 * SEG),
        ("three programs held, seam on the last program", _ns(
            (0.5, 3.0, 60, 100, 0, False), (0.6, 3.0, 50, 100, 33, False), (0.7, 3.0, 70, 100, 40, False), (0.8, 3.0, 72, 100, 40, False),
            (2.1, 2.5, 65, 100, 40, False)), 2 * SEG),
        ("three programs held, seam on another program", _ns(
            (0.5, 3.0, 60, 100, 0, False), (0.6, 3.0, 50, 100, 33, False), (0.7, 3.0, 70, 100, 41, False),
            (2.1, 2.5, 65, 100, 33, False), (2.2, 2.6, 66, 100, 34, False)), 2 * SEG),
        ("chord storm", _ns(*storm), 2 * SEG),
        ("zero velocity note", _ns((0.2, 0.4, 60, 0, 0, False), (0.3, 0.5, 61, 1, 0, False), (0.35, 0.6, 62, 127, 3, False)), SEG),
    ]


def spread(ns, seed):
    """`ns` with programs spread over {0, 33, 40} and 20 % drums"""
    rng = np.random.default_rng(seed)
    out = NoteSequence(total_time=ns.total_time)
    for n in ns.notes:
        out.notes.append(Note(n.start_time, n.end_time, n.pitch, int(rng.integers(1, 128)), int(rng.choice([0, 33, 40])),
                              bool(rng.random() < 0.2), 0))
    return out


def random_files(seconds=20.0, seeds=range(8)):
    frames = int(seconds * 125) + 1
    return [("random_music %d" % s, synthetic.random_music(seconds, seed=s), frames) for s in seeds]


def spread_files(seconds=20.0, seeds=range(8)):
    frames = int(seconds * 125) + 1
    return [("spread %d" % s, spread(synthetic.random_music(seconds, seed=s), 100 + s), frames) for s in seeds]


def shifted(ns, shift):
    """every note time + shift, clamped at 0: what `shifts=` means"""
    return NoteSequence(notes=[Note(max(n.start_time + shift, 0.0), max(n.end_time + shift, 0.0), n.pitch, n.velocity, n.program,
                                    n.is_drum, n.instrument) for n in ns.notes], total_time=ns.total_time)
