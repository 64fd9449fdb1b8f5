"""Synthetic progressions and the edge job of the harmony tests (a helper, not a test): numpy only, deterministic."""
import numpy as np

from mt3_amd import _lib, note_sequences

FPS = 100
BEAT_TILE, NOTE_TILE = _lib.HARMONY_BEAT_TILE, _lib.HARMONY_NOTE_TILE


def note(start, end, pitch, drum=False):
    """a note from FRAMES: start / 100 and end / 100 round back to the frames exactly"""
    return note_sequences.Note(start_time=int(start) / float(FPS), end_time=int(end) / float(FPS), pitch=int(pitch),
                               velocity=90, program=0, is_drum=bool(drum))


def sequence(notes):
    return note_sequences.NoteSequence(notes=list(notes), total_time=max((n.end_time for n in notes), default=0.0))


# ---- progressions

def progression(tonic, minor, bar, form, jitter=0, seed=0, period=50, first=40, repeats=2, lead_in=0):
    """I-IV-V-I (or i-iv-V-i) on `tonic`, one chord per bar of `bar` beats, `repeats` times, the beats `period` frames
    apart from frame `first` on; `lead_in` beats of the last chord's bar come before the first downbeat (the phase).
    form "block": the triad struck on every beat for one beat, the root an octave below struck on the downbeat for the
    bar; "arpeggio": one chord tone per beat (root, third, fifth, third) over the same bass.  jitter: every onset moves
    by a whole number of frames drawn from -jitter .. jitter (seeded); the ends stay.
    -> (NoteSequence, beat frames int32, truth): truth = dict(key, chords int8 [B], beats_per_bar, downbeat)"""
    rng = np.random.RandomState(seed)
    degrees = [(0, minor), (5, minor), (7, 0), (0, minor)] * repeats       # (root above the tonic, minor triad)
    bars = [degrees[-1]] * (1 if lead_in else 0) + degrees
    skip = bar - lead_in if lead_in else 0                                 # the beats of the lead-in bar that are not played
    n_beats = len(bars) * bar - skip
    beats = first + period * np.arange(n_beats)
    notes, chords = [], np.zeros(n_beats, np.int8)

    def move():
        return int(rng.randint(-jitter, jitter + 1)) if jitter else 0

    for k, (degree, is_minor) in enumerate(bars):
        root = (tonic + degree) % 12
        third = 48 + root + (3 if is_minor else 4)
        tones = [48 + root, third, 48 + root + 7, third]
        for j in range(bar):
            i = k * bar + j - skip
            if i < 0:
                continue
            chords[i] = 1 + 2 * root + is_minor
            t, t1 = int(beats[i]), int(beats[i]) + period
            if j == 0:
                notes.append(note(max(t + move(), 0), t + (bar - j) * period, 36 + root))
            if form == "block":
                notes += [note(max(t + move(), 0), t1, p) for p in tones[:3]]
            else:
                notes.append(note(max(t + move(), 0), t1, tones[j % 4]))
    order = rng.permutation(len(notes))
    truth = dict(key=2 * tonic + minor, chords=chords, beats_per_bar=bar, downbeat=lead_in % bar)
    return sequence([notes[i] for i in order]), beats.astype(np.int32), truth


def progressions(jitter=0):
    """every (name, NoteSequence, beat frames, truth): four major and four minor keys, 4/4 and 3/4, both forms, two of
    them with a lead-in (a downbeat phase other than 0)"""
    out = []
    for t, (tonic, minor) in enumerate(((0, 0), (3, 0), (6, 0), (9, 0), (9, 1), (0, 1), (6, 1), (2, 1))):
        for bar in (4, 3):
            for form in ("block", "arpeggio"):
                lead_in = (t % 3) if bar == 3 else (t % 4)
                name = "%d%s %d/4 %s lead-in %d" % (tonic, "m" if minor else "", bar, form, lead_in)
                out.append((name,) + progression(tonic, minor, bar, form, jitter, seed=len(out), lead_in=lead_in))
    return out


# ---- the edge job

def grid(n_beats, period=40, first=30):
    return (first + period * np.arange(n_beats)).astype(np.int32)


def random_file(seed, n_notes, beats, drums=0.15):
    """`n_notes` notes with starts drawn over the beats' span and a little beyond, lengths of 1 .. 3 beat periods, pitches
    drawn around a few chords so that the path has something to follow; some drums; the notes in drawn order"""
    rng = np.random.RandomState(seed)
    beats = np.asarray(beats, np.int64)
    lo, hi = (int(beats[0]) - 20, int(beats[-1]) + 60) if len(beats) else (0, 400)
    span = int(np.diff(beats).mean()) if len(beats) > 1 else 40
    notes = []
    for _ in range(n_notes):
        s = max(int(rng.randint(lo, hi)), 0)
        if len(beats) and rng.rand() < 0.5:                                 # half of the notes start near a beat
            s = max(int(beats[rng.randint(len(beats))]) + int(rng.randint(-4, 5)), 0)
        root = (0, 5, 7, 9)[(s // (4 * span)) % 4]
        pitch = 36 + root + int(rng.choice([0, 4, 7, 12, 16, 19, 24])) + (int(rng.randint(-2, 3)) if rng.rand() < 0.2 else 0)
        notes.append(note(s, s + int(rng.randint(1, 3 * span + 1)), pitch, rng.rand() < drums))
    return sequence(notes)


def edge_job():
    """-> [(name, NoteSequence, beat frames int32)]: one job that crosses every seam of the rule and of the kernel"""
    job = []

    def add(name, notes, beats):
        job.append((name, notes if hasattr(notes, "notes") else sequence(notes), np.asarray(beats, np.int32)))

    triad = lambda b: [note(b[0] if len(b) else 30, (b[-1] if len(b) else 30) + 40, p) for p in (48, 52, 55)]   # noqa: E731
    for B in range(6):                                                      # below and at 2 m for m = 2 (and 3 at B = 6 below)
        add("%d beats" % B, triad(grid(B)) + [note(int(f), int(f) + 5, 38, True) for f in grid(B)[::2]], grid(B))
    for B in (6, 7, 8, BEAT_TILE - 1, BEAT_TILE, BEAT_TILE + 1, 3 * BEAT_TILE + 1):
        add("random, %d beats" % B, random_file(B, 90, grid(B)), grid(B))
    for n in (NOTE_TILE - 1, NOTE_TILE, NOTE_TILE + 1, 2 * NOTE_TILE + 61):
        add("random, %d notes" % n, random_file(n, n, grid(40)), grid(40))
    long = grid(2 * BEAT_TILE + 6)
    add("one note over every interval", [note(0, int(long[-1]) + 200, 57)], long)
    add("notes before the first beat and after the last interval",
        [note(0, 25, 60), note(5, 30, 64), note(30 + 40 * 8, 30 + 40 * 8 + 50, 67), note(600, 700, 48), note(30, 70, 50)], grid(8))
    add("notes that end on a beat frame", [note(30, 70, 60), note(50, 110, 64), note(70, 71, 67), note(29, 30, 48),
                                           note(110, 150, 55)], grid(8))
    add("drums only", [note(int(f) + d, int(f) + d + 6, 36 + d, True) for f in grid(9) for d in (0, 1)], grid(9))
    add("one pitch", [note(int(f), int(f) + 40, 60) for f in grid(9)], grid(9))
    add("no notes", [], grid(9))
    add("no notes and no beats", [], grid(0))
    add("notes and no beats", triad(grid(0)), grid(0))
    add("two notes of one pitch overlapping", [note(30, 150, 60), note(70, 190, 60), note(30, 190, 67)], grid(6))
    add("pitches 0 and 127", [note(30, 200, 0), note(35, 200, 127), note(110, 230, 127), note(150, 152, 0)], grid(7))
    unequal = np.cumsum([20, 13, 400, 14, 399, 57, 13, 13, 200, 31, 400, 13, 90])
    add("unequal intervals", random_file(5, 120, unequal), unequal)
    # E of A major (A C# E) in interval 0 is 3 * 3 - 10 = -1: (-1 * 256) // 10 = -26, truncation would give -25
    add("a negative E that is no multiple of tot", [note(30, 37, 60), note(40, 43, 61), note(70, 110, 60)], grid(4))
    # C alone: C major and C minor tie on every beat (the lower state); every class as long as every other: twelve keys tie
    add("two chords tie", [note(30, 30 + 40 * 6, 48)], grid(6))
    add("twelve keys tie", [note(30 + 10 * c, 40 + 10 * c, 60 + c) for c in range(12)], grid(5))
    # drums on the beats 0, 1, 4, 5: the phases 0 and 1 of m = 4 tie (the lower phase); on 0, 2, 4, 6 AND nothing else
    # m = 2 beats m = 4; every beat alike: no score above 0, no meter
    add("two phases tie", [note(int(f), int(f) + 3, 36, True) for f in grid(8)[[0, 1, 4, 5]]], grid(8))
    add("m = 2 over m = 4", [note(int(f), int(f) + 3, 36, True) for f in grid(8)[::2]], grid(8))
    add("every beat alike", [note(int(f), int(f) + 3, 36, True) for f in grid(8)], grid(8))
    add("onsets at the window's edge", [note(int(f) + d, int(f) + d + 9, 40 + d) for f in grid(10)[::3] for d in (-4, -3, 3, 4)]
        + [note(30, 400, 40 + 3)], grid(10))
    close = np.array([10, 11, 12, 14, 17, 18, 30, 31, 45], np.int32)       # beats closer than the onset window
    add("beats a frame apart", random_file(9, 40, close), close)
    add("a late file", random_file(3, 60, grid(12, 50, (1 << 20) - 800)), grid(12, 50, (1 << 20) - 800))
    for name, ns, beats, _ in progressions(2)[:6]:
        add("progression " + name, ns, beats)
    return job
