"""Synthetic metrical input for the beat tracker's tests (a helper, not a test): numpy only, deterministic."""
import numpy as np

from mt3_amd import note_sequences

FPS = 100


def sequence(frames, length=0.1):
    """one note per onset frame, in the order given: start = frame / 100 exactly (so the packer's rounding gives `frame`
    back), pitches and programs varied, every fourth note a drum"""
    notes = [note_sequences.Note(start_time=int(f) / float(FPS), end_time=int(f) / float(FPS) + length, pitch=36 + i % 48,
                                 velocity=100, program=(i % 3) * 8, is_drum=i % 4 == 3) for i, f in enumerate(frames)]
    return note_sequences.NoteSequence(notes=notes, total_time=max((n.end_time for n in notes), default=0.0))


def metrical(bpm, beats, jitter_frames=0, drop=0.0, extra=0.0, seed=0, first=37):
    """-> (NoteSequence, grid): `beats` beats at `bpm` from frame `first` on, grid[i] = first + round(i * 6000 / bpm) (int64
    frames).  Each beat carries one onset, moved by a whole number of frames drawn from -jitter_frames .. jitter_frames;
    round(drop * beats) beats, the first and last never, carry none; round(extra * beats) further onsets lie on frames
    drawn uniformly between the first and last beat that are on no grid frame.  The notes are shuffled."""
    rng = np.random.RandomState(seed)
    grid = first + np.rint(np.arange(beats) * (60.0 * FPS / bpm)).astype(np.int64)
    keep = np.ones(beats, bool)
    if beats > 2:
        keep[1 + rng.permutation(beats - 2)[:int(round(drop * beats))]] = False
    onsets = grid[keep] + rng.randint(-jitter_frames, jitter_frames + 1, int(keep.sum()))
    off_grid = np.setdiff1d(np.arange(grid[0], grid[-1] + 1), grid)
    more = off_grid[rng.permutation(len(off_grid))[:int(round(extra * beats))]]
    frames = np.concatenate([onsets, more])
    return sequence(frames[rng.permutation(len(frames))]), grid


def f_measure(found, grid, tolerance=7):
    """the beat F-measure: a found beat and a grid beat match when they are within `tolerance` frames (the customary 70 ms),
    each at most once, in order of time"""
    found, grid = [int(f) for f in found], [int(g) for g in grid]
    i = j = hits = 0
    while i < len(found) and j < len(grid):
        if abs(found[i] - grid[j]) <= tolerance:
            hits, i, j = hits + 1, i + 1, j + 1
        elif found[i] < grid[j]:
            i += 1
        else:
            j += 1
    if not hits:
        return 0.0
    precision, recall = hits / len(found), hits / len(grid)
    return 2 * precision * recall / (precision + recall)
