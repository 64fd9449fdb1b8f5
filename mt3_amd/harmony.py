"""Key, chords and bars: the harmony and the meter of a transcription from its own notes and beats.

  analyze(sequences, beats, ...)             key, chord per beat, bar length and downbeats of every file of a job on the
                                             device (mt3_op_analyze_harmony): one upload, one op call, one copy back
  analyze_reference(sequences, beats, ...)   THE RULE in numpy: the yardstick of the kernel, bit for bit
  key_profiles()                             the Krumhansl-Kessler profiles as the int32 table the rule multiplies with
  chord_name(state, key)                     "N", "C", "Am", "Eb", ... spelled for the key

`midi_io.note_sequence_to_midi_bytes(ns, beats=b.times, harmony=h)` writes the key signature, the time signature and a
marker per chord change into the tempo map's track.

THE RULE is integer arithmetic throughout (`//` floors, argmax takes the lowest index), so any order of the sums and
integer atomics give the same bits.  Per file, fps = 100; the notes have start, end, pitch, is_drum; the beat frames
b[0 .. B-1] are int32, strictly ascending, below 2^20 (`beats.track(...)[f].frames`, or any such array).

 1. NOTE FRAMES (host, float64)  s = floor(start * fps + 0.5), e = max(floor(end * fps + 0.5), s + 1); e <= 2^20.
 2. BEAT INTERVALS  B < 2: no chords, no meter (beats_per_bar 0); the key is still found.  Else interval i is
    [b[i], b[i+1]) for i < B - 1 and the last one is as long as the one before it: [b[B-1], 2 b[B-1] - b[B-2]).  len[i] is
    its length.  What a note has before b[0] or after the last interval's end is clipped away.
 3. BEAT ROLL  R[i][p] = the frames non-drum notes of pitch p share with interval i, summed over the notes (two notes of
    one pitch count twice), int32.  H[i][c] = sum of R[i][p] over p % 12 == c; tot[i] = sum of H[i].  low[i] = the lowest p
    with 4 R[i][p] >= len[i], or -1; bass[i] = low[i] % 12, or -1.
 4. KEY (one per file, whatever the beats)  D[c] = the total of e - s over the non-drum notes of class c (int64);
    key_score[k] = sum over c of K[k][c] * D[c] with K = `key_profiles()`; the key is the LOWEST k of maximal score,
    k = 2 * tonic + mode (0 major, 1 minor); -1 without non-drum notes.  K[k] is the key's Krumhansl-Kessler profile
    with its mean taken off, scaled to unit norm and to 4096: for a fixed D the Pearson correlation of D with the
    profile is key_score[k] / (4096 * norm(D - mean(D))) up to K's rounding, and the divisor does not depend on k -- so
    the scores order the 24 keys as the correlations do.
 5. CHORDS  25 states: 0 = N (no chord), 1 + 2 r + q = the triad on root r, major (q = 0: tones r, r + 4, r + 7) or minor
    (q = 1: r, r + 3, r + 7).  E[i][k] = sum over c of w_k(c) * H[i][c] + (H[i][r] if bass[i] == r else 0), w = +2 on a
    chord tone, -1 elsewhere; E[i][0] = 0.  Q[i][k] = (E[i][k] * 256) // max(tot[i], 1): -256 .. 768.
        V[0][k] = Q[0][k];   V[i][k] = Q[i][k] + max(V[i-1][k], M - change_penalty)
    M = the largest V[i-1][.], at its lowest index j; staying wins on equal values; back[i][k] = k or j.  The path ends at
    the LOWEST k of maximal V[B-1] and is read back: chords int8 [B], chord_score = V[B-1][end].  |V| <= 768 B + 2^20 <
    2^30 with B <= 2^20, so int32 holds it.
 6. METER  change[i] = 1 when i > 0 and chords[i] != chords[i-1];  on[i] = min(the notes, drums too, with
    |s - b[i]| <= 3, 255);  struck[i] = 1 when a non-drum note with |s - b[i]| <= 3 has pitch low[i];
    a[i] = onset_weight * on[i] + change_weight * change[i] + bass_weight * struck[i].  For m in (2, 3, 4) with B >= 2 m
    and phase f in 0 .. m - 1: num = the sum of a[i] over i % m == f, cnt = the number of such i,
        score(m, f) = (num << 16) // cnt - ((sum of a - num) << 16) // (B - cnt)
    The meter is the (m, f) of maximal score, the lowest m, then the lowest f on ties; no admissible m, or no score > 0:
    beats_per_bar 0, downbeat -1, no downbeats.  Else the downbeats are the beats i % m == f.

change_penalty, the three weights, the +2 / -1 / bass template and the 4 R >= len threshold are DESIGN CHOICES, not
measurements (DESIGN.md section 6t holds the procedure and the ranges).  Limits: one key per file (no modulations);
triads only (a seventh chord is heard as its triad); one meter per file, bars of 2, 3 or 4 quarter notes (6/8 comes out
as 3 or 2); chords change only on beats; drums carry no harmony; programs are ignored.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List

import numpy as np

from . import _lib, note_arrays
from .beats import Beats, _check_sequences

FPS = _lib.BEATS_FPS
MAX_FRAMES = _lib.BEATS_MAX_FRAMES
STATES = _lib.HARMONY_STATES                             # 25
KEYS = _lib.HARMONY_KEYS                                 # 24
BEAT_TILE, NOTE_TILE = _lib.HARMONY_BEAT_TILE, _lib.HARMONY_NOTE_TILE
ONSET_WINDOW = _lib.HARMONY_ONSET_WINDOW                 # 3 frames to either side of a beat
MAX_CHANGE_PENALTY, MAX_WEIGHT = _lib.HARMONY_MAX_CHANGE_PENALTY, _lib.HARMONY_MAX_WEIGHT
WORKSPACE_BYTES_PER_BEAT = _lib.HARMONY_WORKSPACE_BYTES_PER_BEAT
# the middle of the range (512 .. 1202) over which the numpy rule recovers every label of all 64 progressions of
# tests/harmony_cases.py, clean and jittered; the weights: every value tried recovers every meter there, so they are set
# by reasoning
DEFAULT_CHANGE_PENALTY = 857
DEFAULT_ONSET_WEIGHT, DEFAULT_CHANGE_WEIGHT, DEFAULT_BASS_WEIGHT = 1, 4, 2
FILE_DTYPE = np.dtype([("first", "<i8"), ("beat0", "<i8"), ("n_notes", "<i4"), ("n_beats", "<i4")])

# Krumhansl & Kessler (1982): the probe-tone ratings of the twelve classes above a major and a minor tonic
KK_MAJOR = (6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88)
KK_MINOR = (6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17)
SHARP_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")
FLAT_NAMES = ("C", "Db", "D", "Eb", "E", "F", "Gb", "G", "Ab", "A", "Bb", "B")
# the MIDI key-signature value of key 2 * tonic + mode: a major key's own (-5 .. 6), a minor key its relative major's
_MAJOR_SHARPS = (0, -5, 2, -3, 4, -1, 6, 1, -4, 3, -2, 5)
SHARPS = tuple(_MAJOR_SHARPS[(t + 3 * q) % 12] for t in range(12) for q in (0, 1))


@dataclasses.dataclass
class Harmony:
    """One file's harmony and meter.  key: -1, or 2 * tonic + mode; key_name: "Eb major", "" without a key; sharps: the MIDI
    key-signature value, -7 .. 7 (0 without a key); key_scores: int64 [24]; chords: int8 [B], a state per beat;
    chord_score: V at the path's end; beats_per_bar: 0, 2, 3 or 4; downbeat: the phase, -1 without a meter; downbeats:
    float64 times; segments: the runs of equal chords as (start_time, end_time, name)."""
    key: int
    key_name: str
    sharps: int
    key_scores: np.ndarray
    chords: np.ndarray
    chord_score: int
    beats_per_bar: int
    downbeat: int
    downbeats: np.ndarray
    segments: list


@dataclasses.dataclass
class Packed:
    """the host side of one mt3_op_analyze_harmony call"""
    column: np.ndarray                  # uint8: start | end | key (pitch + 256 * is_drum), int32 each, file after file
    n_notes: int
    beats: np.ndarray                   # int32: the beat frames, file after file
    files: np.ndarray                   # FILE_DTYPE [n_files]

    def notes(self, f: int):
        a, n = int(self.files["first"][f]), int(self.files["n_notes"][f])
        cols = self.column.view("<i4").reshape(3, -1) if self.n_notes else np.zeros((3, 0), np.int32)
        return cols[0, a: a + n], cols[1, a: a + n], cols[2, a: a + n]

    def beat_frames(self, f: int) -> np.ndarray:
        a = int(self.files["beat0"][f])
        return self.beats[a: a + int(self.files["n_beats"][f])]


@functools.lru_cache(maxsize=1)
def key_profiles() -> np.ndarray:
    """K, int32 [24, 12]: row 2 t + q is the Krumhansl-Kessler profile of mode q, mean taken off, unit norm, times 4096,
    rotated to tonic t; built here and nowhere else"""
    table = np.zeros((KEYS, 12), np.int32)
    for q, profile in enumerate((KK_MAJOR, KK_MINOR)):
        p = np.asarray(profile, np.float64)
        p = p - p.mean()
        p = p / np.sqrt((p * p).sum())
        for t in range(12):
            table[2 * t + q] = np.rint(4096.0 * p[(np.arange(12) - t) % 12]).astype(np.int32)
    table.setflags(write=False)
    return table


def chord_tones(state: int):
    """the three pitch classes of a chord state 1 .. 24, the root first"""
    r, q = (state - 1) // 2, (state - 1) % 2
    return r, (r + 4 - q) % 12, (r + 7) % 12


def chord_name(state: int, key: int = -1) -> str:
    """"N" for state 0, else the root's name, flats in a key whose signature has flats, and "m" for a minor triad"""
    state = int(state)
    if not 0 <= state < STATES:
        raise ValueError("a chord state is 0 .. %d, got %r" % (STATES - 1, state))
    if state == 0:
        return "N"
    names = FLAT_NAMES if 0 <= key < KEYS and SHARPS[key] < 0 else SHARP_NAMES
    return names[(state - 1) // 2] + ("m" if (state - 1) % 2 else "")


def key_name(key: int) -> str:
    if not 0 <= key < KEYS:
        return ""
    return (FLAT_NAMES if SHARPS[key] < 0 else SHARP_NAMES)[key // 2] + (" minor" if key % 2 else " major")


def _check_parameters(change_penalty, onset_weight, change_weight, bass_weight):
    def whole(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    if not whole(change_penalty) or not 0 <= change_penalty <= MAX_CHANGE_PENALTY:
        raise ValueError("change_penalty must be an int 0 .. %d, got %r" % (MAX_CHANGE_PENALTY, change_penalty))
    for name, v in (("onset_weight", onset_weight), ("change_weight", change_weight), ("bass_weight", bass_weight)):
        if not whole(v) or not 0 <= v <= MAX_WEIGHT:
            raise ValueError("%s must be an int 0 .. %d, got %r" % (name, MAX_WEIGHT, v))
    return int(change_penalty), int(onset_weight), int(change_weight), int(bass_weight)


def pack(sequences, beats) -> Packed:
    """every check of `analyze` on its notes and beats, and step 1 of the rule: the note frames of every file as three
    int32 columns, the beat frames as one"""
    sequences = _check_sequences(sequences, "analyze")
    try:
        beats = list(beats)
    except TypeError:
        raise ValueError("analyze takes one entry of beats per sequence") from None
    if len(beats) != len(sequences):
        raise ValueError("beats has %d entries for %d sequences" % (len(beats), len(sequences)))
    starts, ends, keys, frames, files = [], [], [], [], np.zeros(len(sequences), FILE_DTYPE)
    for f, (seq, b) in enumerate(zip(sequences, beats)):
        start, end, pitch, _, drum = note_arrays.fields(seq)
        note_arrays.check_times(start, end, not_negative=True, prefix="file %d: " % f)
        note_arrays.check_range("file %d: pitches must be 0 .. 127" % f, pitch)
        s = np.floor(start * float(FPS) + 0.5).astype(np.int64)
        e = np.maximum(np.floor(end * float(FPS) + 0.5).astype(np.int64), s + 1)
        if len(e) and int(e.max()) > MAX_FRAMES:
            raise ValueError("file %d: a note ends at frame %d; a file has at most %d frames (%.1f hours)"
                             % (f, int(e.max()), MAX_FRAMES, MAX_FRAMES / FPS / 3600.0))
        fr = np.ascontiguousarray(b.frames if isinstance(b, Beats) else b).reshape(-1)
        if len(fr) and (fr.dtype.kind not in "iu" or fr[0] < 0 or fr[-1] >= MAX_FRAMES or
                        (np.diff(fr.astype(np.int64)) <= 0).any()):
            raise ValueError("file %d: beat frames must be strictly ascending whole numbers, 0 .. %d" % (f, MAX_FRAMES - 1))
        fr = fr.astype(np.int64)
        longest = int(np.diff(fr).max()) if len(fr) >= 2 else 0
        if len(s) * longest >= 1 << 31:
            raise ValueError("file %d: %d notes times its longest beat interval (%d frames) must stay below 2^31"
                             % (f, len(s), longest))
        starts.append(s), ends.append(e), keys.append(pitch + 256 * (drum != 0)), frames.append(fr.astype(np.int32))
        files[f] = (0, 0, len(s), len(fr))
    files["first"] = note_arrays.offsets(files["n_notes"])[:-1]
    files["beat0"] = note_arrays.offsets(files["n_beats"])[:-1]
    return Packed(note_arrays.pack([starts, ends, keys], ("<i4", "<i4", "<i4")), int(files["n_notes"].sum()),
                  np.concatenate(frames).astype("<i4") if frames else np.zeros(0, "<i4"), files)


# ---- THE RULE, step by step, for one file

def intervals(b: np.ndarray) -> np.ndarray:
    """step 2: the B + 1 edges of the B intervals of B >= 2 beat frames, int64"""
    b = np.asarray(b, np.int64)
    return np.concatenate([b, [2 * b[-1] - b[-2]]])


def beat_roll(s, e, key, b):
    """step 3 -> (R int32 [B, 128], H int64 [B, 12], tot int64 [B], low int64 [B], len int64 [B])"""
    edges = intervals(b)
    B = len(edges) - 1
    R = np.zeros((B, 128), np.int64)
    pitched = np.flatnonzero(np.asarray(key) < 256)
    for at in range(0, len(pitched), 1024):                                # (a block of notes at a time: memory)
        n = pitched[at: at + 1024]
        s_n, e_n = np.asarray(s, np.int64)[n, None], np.asarray(e, np.int64)[n, None]
        shared = np.clip(e_n, edges[None, :-1], edges[None, 1:]) - np.clip(s_n, edges[None, :-1], edges[None, 1:])
        np.add.at(R, (slice(None), np.asarray(key, np.int64)[n]), shared.T)
    assert R.max(initial=0) < 1 << 31
    length = np.diff(edges)
    H = np.concatenate([R, np.zeros((B, 4), np.int64)], 1).reshape(B, 11, 12).sum(1)
    loud = 4 * R >= length[:, None]
    low = np.where(loud.any(1), np.argmax(loud, 1), -1)
    return R.astype(np.int32), H, H.sum(1), low, length


def durations(s, e, key) -> np.ndarray:
    """step 4: D, int64 [12]"""
    pitched = np.asarray(key) < 256
    D = np.zeros(12, np.int64)
    np.add.at(D, np.asarray(key, np.int64)[pitched] % 12, (np.asarray(e, np.int64) - np.asarray(s, np.int64))[pitched])
    return D


def key_scores(D: np.ndarray) -> np.ndarray:
    return key_profiles().astype(np.int64) @ np.asarray(D, np.int64)


@functools.lru_cache(maxsize=1)
def _templates() -> np.ndarray:
    """w, int64 [25, 12]: +2 on a chord tone, -1 elsewhere, zeros for N"""
    w = np.zeros((STATES, 12), np.int64)
    for k in range(1, STATES):
        w[k] = -1
        w[k, list(chord_tones(k))] = 2
    return w


def emissions(H, tot, low):
    """step 5's scores -> (E int64 [B, 25], Q int64 [B, 25])"""
    H, tot, low = np.asarray(H, np.int64), np.asarray(tot, np.int64), np.asarray(low, np.int64)
    E = H @ _templates().T
    bass = np.where(low >= 0, low % 12, -1)
    for q in (0, 1):
        E[:, 1 + q::2] += np.where(bass[:, None] == np.arange(12)[None, :], H, 0)
    return E, (E * 256) // np.maximum(tot, 1)[:, None]


def chord_path(Q, change_penalty: int):
    """step 5's path -> (chords int8 [B], chord_score)"""
    Q = np.asarray(Q, np.int64)
    B = len(Q)
    V, back, states = Q[0].copy(), np.zeros((B, STATES), np.int64), np.arange(STATES)
    for i in range(1, B):
        j = int(np.argmax(V))
        move = V[j] - change_penalty
        stay = V >= move                                                   # staying wins on equal values
        back[i] = np.where(stay, states, j)
        V = Q[i] + np.where(stay, V, move)
    k = int(np.argmax(V))
    score, chords = int(V[k]), np.zeros(B, np.int8)
    for i in range(B - 1, -1, -1):
        chords[i] = k
        k = int(back[i, k])
    return chords, score


def accents(s, key, b, low, chords, onset_weight: int, change_weight: int, bass_weight: int) -> np.ndarray:
    """step 6's a, int64 [B]"""
    s, key, b = np.asarray(s, np.int64), np.asarray(key, np.int64), np.asarray(b, np.int64)
    near = np.abs(s[None, :] - b[:, None]) <= ONSET_WINDOW                 # [B, notes]
    on = np.minimum(near.sum(1), 255)
    struck = (near & (key[None, :] == np.asarray(low, np.int64)[:, None])).any(1)      # a drum's key is >= 256, low < 128
    change = np.concatenate([[0], (np.diff(np.asarray(chords, np.int64)) != 0).astype(np.int64)])
    return onset_weight * on + change_weight * change + bass_weight * struck.astype(np.int64)


def meter_scores(a) -> dict:
    """step 6's score(m, f) of every admissible (m, f), in the order of the tie rule"""
    a = np.asarray(a, np.int64)
    B, total, out = len(a), int(a.sum()), {}
    for m in (2, 3, 4):
        if B < 2 * m:
            continue
        for f in range(m):
            num, cnt = int(a[f::m].sum()), len(a[f::m])
            out[(m, f)] = (num << 16) // cnt - ((total - num) << 16) // (B - cnt)
    return out


def meter(a):
    """-> (beats_per_bar, downbeat): the first (m, f) of maximal score > 0, else (0, -1)"""
    best, found = 0, (0, -1)
    for mf, score in meter_scores(a).items():
        if score > best:
            best, found = score, mf
    return found


def analyze_file(s, e, key, b, change_penalty, onset_weight, change_weight, bass_weight):
    """steps 2 .. 6 for one file -> (key, key_scores int64 [24], chords int8 [B], chord_score, beats_per_bar, downbeat)"""
    D = durations(s, e, key)
    scores = key_scores(D)
    found = int(np.argmax(scores)) if D.any() else -1
    if len(b) < 2:
        return found, scores, np.zeros(0, np.int8), 0, 0, -1
    _, H, tot, low, _ = beat_roll(s, e, key, b)
    chords, chord_score = chord_path(emissions(H, tot, low)[1], change_penalty)
    bar, phase = meter(accents(s, key, b, low, chords, onset_weight, change_weight, bass_weight))
    return found, scores, chords, chord_score, bar, phase


def _harmony(key, scores, chords, chord_score, bar, phase, b) -> Harmony:
    key, bar, phase = int(key), int(bar), int(phase)
    chords = np.ascontiguousarray(chords, np.int8)
    segments = []
    if len(chords):
        edges = intervals(b).astype(np.float64) / float(FPS)
        cuts = np.concatenate([[0], np.flatnonzero(np.diff(chords)) + 1, [len(chords)]])
        segments = [(float(edges[i]), float(edges[j]), chord_name(chords[i], key)) for i, j in zip(cuts[:-1], cuts[1:])]
    downbeats = np.asarray(b, np.int32)[phase::bar].astype(np.float64) / float(FPS) if bar else np.zeros(0, np.float64)
    return Harmony(key, key_name(key), SHARPS[key] if key >= 0 else 0, np.ascontiguousarray(scores, np.int64), chords,
                   int(chord_score), bar, phase if bar else -1, downbeats, segments)


def analyze_reference(sequences, beats, change_penalty: int = DEFAULT_CHANGE_PENALTY,
                      onset_weight: int = DEFAULT_ONSET_WEIGHT, change_weight: int = DEFAULT_CHANGE_WEIGHT,
                      bass_weight: int = DEFAULT_BASS_WEIGHT) -> List[Harmony]:
    """`analyze` in numpy alone: the same arguments, checks and results, bit for bit"""
    parameters = _check_parameters(change_penalty, onset_weight, change_weight, bass_weight)
    packed = pack(sequences, beats)
    return [_harmony(*analyze_file(*packed.notes(f), packed.beat_frames(f), *parameters), packed.beat_frames(f))
            for f in range(len(packed.files))]


def run(packed: Packed, change_penalty: int, onset_weight: int, change_weight: int, bass_weight: int):
    """one upload, one mt3_op_analyze_harmony call, one copy back -> (key_scores i64 [files, 24], info i32 [files, 4]: key,
    chord_score, beats_per_bar, downbeat; chords i8 [total beats]: a file's from its `beat0` on)"""
    import torch
    n_files, n, n_beats = len(packed.files), packed.n_notes, len(packed.beats)
    profiles = key_profiles().reshape(-1)
    # the one upload: files | start | end | key | beat frames | profiles (every part a multiple of 4 bytes, files of 8)
    parts = [packed.files.view(np.uint8).reshape(-1), packed.column, packed.beats.view(np.uint8), profiles.view(np.uint8)]
    data = note_arrays.to_device(np.concatenate(parts))
    files_at = data.data_ptr()
    start_at = files_at + FILE_DTYPE.itemsize * n_files
    beats_at = start_at + 12 * n
    profiles_at = beats_at + 4 * n_beats
    info_at, chords_at = 8 * KEYS * n_files, 8 * KEYS * n_files + 16 * n_files
    out = torch.empty(chords_at + n_beats, device="cuda", dtype=torch.uint8)
    workspace = torch.empty(max(WORKSPACE_BYTES_PER_BEAT * n_beats, 1), device="cuda", dtype=torch.uint8)
    keys_host = packed.column.view("<i4")[2 * n:] if n else None
    stream = torch.cuda.current_stream()
    _lib.check(_lib.load().mt3_op_analyze_harmony(
        start_at if n else None, start_at + 4 * n if n else None, start_at + 8 * n if n else None,
        keys_host.ctypes.data if n else None, n, beats_at if n_beats else None,
        packed.beats.ctypes.data if n_beats else None, n_beats, packed.files.ctypes.data, files_at, n_files, profiles_at,
        len(profiles), change_penalty, onset_weight, change_weight, bass_weight, workspace.data_ptr(),
        workspace.numel(), out.data_ptr(), out.data_ptr() + info_at, out.data_ptr() + chords_at, stream.cuda_stream))
    workspace.record_stream(stream)
    host = out.cpu().numpy()                                               # the one copy back
    return (host[:info_at].view("<i8").reshape(n_files, KEYS), host[info_at: chords_at].view("<i4").reshape(n_files, 4),
            host[chords_at:].view(np.int8))


def analyze(sequences, beats, change_penalty: int = DEFAULT_CHANGE_PENALTY, onset_weight: int = DEFAULT_ONSET_WEIGHT,
            change_weight: int = DEFAULT_CHANGE_WEIGHT, bass_weight: int = DEFAULT_BASS_WEIGHT) -> List[Harmony]:
    """The key, the chord of every beat, the bar length and the downbeats of every file of a job, on the device.
    sequences: one NoteSequence (or metrics_utils.NOTE_DTYPE record array) per file, the order of a file's notes does not
    matter; beats: per file a `beats.Beats` or its beat frames.  change_penalty (0 .. 2^20): what the chord path pays for
    a change, in units of Q (256 = the whole interval on the chord); onset_weight, change_weight, bass_weight (0 .. 255):
    what a note onset, a chord change and a struck bass note on a beat add to its accent.  -> one `Harmony` per file.
    One upload, one op call, one copy back; there is no host fallback (`analyze_reference` is the yardstick, not a
    substitute).  ValueError, before anything is uploaded: not a list of sequences; beats that do not match them; a time
    that is not finite or is negative; a pitch outside 0 .. 127; a note that ends after frame 2^20; beat frames that are
    not strictly ascending in 0 .. 2^20 - 1; a parameter out of range.  An empty job gives an empty list."""
    parameters = _check_parameters(change_penalty, onset_weight, change_weight, bass_weight)
    packed = pack(sequences, beats)
    if not len(packed.files):
        return []
    scores, info, chords = run(packed, *parameters)
    return [_harmony(info[f, 0], scores[f], chords[int(b0): int(b0) + int(nb)] if nb >= 2 else np.zeros(0, np.int8),
                     info[f, 1], info[f, 2], info[f, 3], packed.beat_frames(f))
            for f, (b0, nb) in enumerate(zip(packed.files["beat0"], packed.files["n_beats"]))]
