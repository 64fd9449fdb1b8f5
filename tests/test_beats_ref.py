"""The beat tracker's rule (mt3_amd/beats.py, track_reference / snap_reference) against what it must do, on the CPU: a
scalar transcription of the five steps, the exact metrical cases, the jittered ones behind the default tightness, the edges
of every index and tie rule, snapping, and the MIDI tempo map.

One expectation differs from the issue's wording and is derived here instead: the envelope E reaches one frame to either
side of an onset, so two onsets d frames apart have products at lags d - 2 .. d + 2.  Two notes 24 frames apart therefore
DO reach LAG_MIN = 25 (A[25] = E[a] E[a + 25] + ... > 0) and are tracked with period 25; the greatest distance that gives no
beats is 22 (22 + 2 < 25).  Both distances, and 25, are tested against that arithmetic."""
import hashlib
import math

import numpy as np
import pytest

from mt3_amd import beats, midi_io
from mt3_amd import note_sequences as N
from tests import beats_cases as bc

JITTER_BPM = (92, 100, 108, 116, 124, 132, 140, 148)       # seeds 0 .. 7; inside 90 .. 150: the prior leaves no octave choice
# the F-measures of the numpy rule at the default tightness, seeds 0 .. 7: every beat found
RECORDED_F = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
# one beat of the 48 lost or one added moves F by 0.011 .. 0.021; the bar allows one, for a libm whose exp / log round
# an entry of the two tables the other way
F_MARGIN = 0.03


def scalar_rule(frames, prior_bpm=120.0, tightness=beats.DEFAULT_TIGHTNESS, width=1.0):
    """the five steps, one Python integer at a time, tables included -> (period, beat frames, score)"""
    if not len(frames):
        return 0, [], 0
    F = max(frames) + 1
    n = [0] * (F + 2)
    for f in frames:
        n[f + 1] = min(n[f + 1] + 1, 255)
    E = [n[t] + 2 * n[t + 1] + n[t + 2] for t in range(F)]
    peak = max(E)
    S = [(e << 16) // peak for e in E]
    l0 = 60.0 * 100 / prior_bpm
    best, p = 0, 0
    for l in range(25, 201):
        A = sum(E[t] * E[t + l] for t in range(F - l))
        W = int(np.rint(65536.0 * np.exp(-0.5 * (np.log2(l / l0) / width) ** 2)))
        if A * W > best:
            best, p = A * W, l
    if p == 0:
        return 0, [], 0
    lo, hi = (p + 1) // 2, 2 * p
    pen = {l: int(np.rint(tightness * 65536.0 * np.log(np.float64(l) / p) ** 2)) for l in range(lo, hi + 1)}
    C, back = [0] * F, [0] * F
    for t in range(F):
        top, arg = None, 0
        for l in range(lo, hi + 1):
            if t - l >= 0 and (top is None or C[t - l] - pen[l] > top):
                top, arg = C[t - l] - pen[l], l
        if top is not None and top > 0:
            C[t], back[t] = S[t] + top, arg
        else:
            C[t] = S[t]
    t = max(F - p, 0)
    for u in range(t, F):
        if C[u] > C[t]:
            t = u
    score, path = C[t], [t]
    while back[t]:
        t -= back[t]
        path.append(t)
    return p, path[::-1], score


def frames_of(ns):
    return [int(math.floor(n.start_time * 100 + 0.5)) for n in ns.notes]


def agree(ns, **kw):
    got = beats.track_reference([ns], **kw)[0]
    p, path, score = scalar_rule(frames_of(ns), **kw)
    assert (got.period, got.frames.tolist(), got.score) == (p, path, score)
    assert got.frames.dtype == np.int32 and np.array_equal(got.times, got.frames / 100.0)
    assert got.qpm == (6000.0 / p if p else 0.0)
    return got


# ---- exact cases

@pytest.mark.parametrize("bpm,period", [(150, 40), (120, 50), (100, 60)])
def test_onsets_on_every_beat_are_tracked_exactly(bpm, period):
    ns, grid = bc.metrical(bpm, 32)
    got = agree(ns)
    assert got.period == period
    # pen[p] = 0 and every other step pays: from the second beat on the path walks the grid, and skips none of it
    found = got.frames.tolist()
    assert len(found) >= 31 and set(found[1:]) <= set(grid.tolist())
    inside = [g for g in grid.tolist() if found[0] <= g <= found[-1]]
    assert [f for f in found if f in set(grid.tolist())] == inside
    assert found[-1] == grid[-1] and got.qpm == bpm


# ---- jittered cases: the default tightness

@pytest.mark.parametrize("seed", range(8))
def test_jittered_files_stay_tracked_at_the_default_tightness(seed):
    ns, grid = bc.metrical(JITTER_BPM[seed], 48, jitter_frames=1, drop=0.2, extra=0.2, seed=seed)
    got = beats.track_reference([ns])[0]
    f = bc.f_measure(got.frames, grid)
    print("seed %d: %d bpm, period %d, %d beats, F-measure %.4f" % (seed, JITTER_BPM[seed], got.period, len(got.frames), f))
    assert abs(got.period - 6000.0 / JITTER_BPM[seed]) <= 2          # two onsets moved by a frame each: no octave error
    assert f >= min(RECORDED_F) - F_MARGIN


def test_the_default_tightness_is_the_middle_of_the_tracked_range():
    cases = [bc.metrical(b, 48, 1, 0.2, 0.2, seed) for seed, b in enumerate(JITTER_BPM)]

    def all_found(tightness):
        out = beats.track_reference([ns for ns, _ in cases], tightness=tightness)
        return all(bc.f_measure(o.frames, grid) == 1.0 for o, (_, grid) in zip(out, cases))

    assert beats.DEFAULT_TIGHTNESS == (20 + 184) / 2
    assert all(all_found(t) for t in (20.0, 60.0, 102.0, 184.0))         # the range written down in DESIGN.md 6r ...
    assert not all_found(19.0) and not all_found(192.0)                   # ... and its two ends


# ---- edges

def test_empty_and_single_onsets_have_no_beats():
    for frames in ([], [0], [731], [40] * 7):                             # no notes; one; all notes in one frame
        got = agree(bc.sequence(frames))
        assert (got.period, len(got.frames), got.score, got.qpm) == (0, 0, 0, 0.0)


def test_two_notes_around_lag_min():
    assert agree(bc.sequence([10, 32])).period == 0                       # 22 apart: lags up to 24 only
    near = agree(bc.sequence([10, 34]))                                    # 24 apart: E[9] E[34] + E[10] E[35] = 4 at lag 25
    assert near.period == 25 and near.frames.tolist()[-1] in (34, 35)
    at = agree(bc.sequence([10, 35]))                                      # 25 apart: 1 * 1 + 2 * 2 + 1 * 1 at lag 25
    assert at.period == 25 and at.frames.tolist() == [10, 35]
    assert agree(bc.sequence([0, 24])).period == 0                        # the file's first frame: no E[-1] to reach lag 25


def test_the_clamp_at_255_onsets():
    ns, grid = bc.metrical(120, 12)
    crowd = bc.sequence(frames_of(ns) + [int(grid[5])] * 299)             # 300 onsets in one frame
    got = agree(crowd)
    E = beats.envelope(np.array(frames_of(crowd)), int(grid[-1]) + 1)
    assert E.max() == 2 * 255 and E[grid[5] - 1] == 255 and got.period == 50


@pytest.mark.parametrize("p", [25, 40])
@pytest.mark.parametrize("which", ["lo", "lo+1", "hi", "hi+1", "p"])
def test_file_lengths_at_the_window_s_ends(which, p):
    lo, hi = (p + 1) // 2, 2 * p
    F = {"lo": lo, "lo+1": lo + 1, "hi": hi, "hi+1": hi + 1, "p": p}[which]
    got = agree(bc.sequence(sorted(set(range(0, F, p)) | {F - 1})))        # onsets p apart, and one in the last frame
    if which == "hi+1":                                                    # 0, p, 2 p: the file's last frame is t - hi = 0's reach
        assert got.period == p and got.frames.tolist() == [0, p, 2 * p]
    if F <= p:                                                             # no two onsets a whole period apart
        assert got.period == 0 or got.period < p


def test_constant_envelope_takes_the_lowest_lag_and_the_lowest_frame():
    got = agree(bc.sequence(list(range(400))))                             # an onset in every frame
    # A[l] = 16 (400 - l) - 14 falls with l: the prior picks the period, every S but the two ends is the peak
    assert got.period == int(np.argmax([(16 * (400 - l) - 14) * w for l, w in zip(range(25, 201), beats.prior_table())])) + 25
    flat = agree(bc.sequence(list(range(400))), tightness=0.0)             # no step pays: every C of a block ties
    assert flat.frames[0] == 1                                             # frame 0 has E = 3, frame 1 is the first of the peak's
    assert np.all(np.diff(flat.frames) == (flat.period + 1) // 2)          # the lowest lag on equal values


def test_the_order_of_the_notes_and_record_arrays():
    ns, _ = bc.metrical(108, 24, 1, 0.2, 0.2, seed=5)
    a = beats.track_reference([ns])[0]
    b = beats.track_reference([N.NoteSequence(notes=sorted(ns.notes, key=lambda n: -n.start_time))])[0]
    assert a.frames.tolist() == b.frames.tolist() and a.score == b.score


def test_track_refuses_bad_input():
    with pytest.raises(ValueError, match="at least|fewer than"):
        beats.track_reference([bc.sequence([1 << 20])])
    with pytest.raises(ValueError, match="tightness"):
        beats.track_reference([], tightness=-1.0)
    with pytest.raises(ValueError, match="prior_bpm"):
        beats.track_reference([], prior_bpm=0.0)


# ---- snapping

def _ns(pairs):
    return N.NoteSequence(notes=[N.Note(a, b, 60 + i, 90, 3, i % 2 == 1, 2) for i, (a, b) in enumerate(pairs)],
                          total_time=max(b for _, b in pairs), control_changes=[N.ControlChange(0.5, 64, 127, 2)])


def _times(ns):
    return [(n.start_time, n.end_time) for n in ns.notes]


BEAT_FRAMES = np.array([50, 100, 164, 228], np.int32)                      # 0.5, 1.0, 1.64, 2.28 s


def test_notes_on_the_grid_do_not_move():
    b = BEAT_FRAMES / 100.0
    grid = [b[i] + (k / 4.0) * (b[i + 1] - b[i]) for i in range(3) for k in range(4)] + [b[3]]
    ns = _ns([(g, h) for g, h in zip(grid, grid[1:])])
    out = beats.snap_reference([ns], [BEAT_FRAMES], 4)[0]
    assert _times(out) == _times(ns)
    assert [(n.pitch, n.velocity, n.program, n.is_drum, n.instrument) for n in out.notes] == \
        [(n.pitch, n.velocity, n.program, n.is_drum, n.instrument) for n in ns.notes]
    assert out.control_changes == ns.control_changes and out is not ns and out.notes[0] is not ns.notes[0]


def test_half_way_goes_to_the_lower_point_and_short_notes_keep_one_step():
    # steps of 0.125 s in the first interval: 0.5625 is exactly half way between 0.5 and 0.625
    ns = _ns([(0.5625, 0.9), (0.5626, 0.9), (0.70, 0.71), (0.99, 1.0)])
    out = _times(beats.snap_reference([ns], [BEAT_FRAMES], 4)[0])
    assert out[0] == (0.5, 0.875) and out[1] == (0.625, 0.875)
    assert out[2] == (0.75, 0.875)                                          # both ends at 0.75: one step is kept
    assert out[3] == (1.0, 0.5 + (5 / 4.0) * 0.5)                           # the start's interval goes on: its fifth step
    assert _times(ns)[0] == (0.5625, 0.9)                                   # the input is untouched


def test_before_the_first_and_after_the_last_beat_the_grid_continues():
    ns = _ns([(0.0, 0.13), (0.26, 0.5), (2.5, 3.0)])
    out = _times(beats.snap_reference([ns], [BEAT_FRAMES], 2)[0])
    d0, d2 = 0.5, 2.28 - 1.64
    assert out[0] == (0.5 + (-2 / 2.0) * d0, 0.5 + (-1 / 2.0) * d0)
    assert out[1] == (0.5 + (-1 / 2.0) * d0, 0.5)
    assert out[2] == (1.64 + (3 / 2.0) * d2, 1.64 + (4 / 2.0) * d2)


def test_fewer_than_two_beats_leave_the_notes_and_bad_arguments_are_refused():
    ns = _ns([(0.33, 0.71)])
    for few in ([], [50]):
        assert _times(beats.snap_reference([ns], [np.array(few, np.int32)], 4)[0]) == _times(ns)
    for bad in (0, 49, 2.0, True):
        with pytest.raises(ValueError, match="subdivisions"):
            beats.snap_reference([ns], [BEAT_FRAMES], bad)
    with pytest.raises(ValueError, match="ascending"):
        beats.snap_reference([ns], [np.array([50, 50])], 4)
    with pytest.raises(ValueError, match="entries"):
        beats.snap_reference([ns], [], 4)


# ---- MIDI

def fixed_sequence():
    return N.NoteSequence(
        notes=[N.Note(0.0, 0.5, 60, 100, 0, False, 0), N.Note(0.25, 1.0, 64, 90, 0, False, 0),
               N.Note(1.013, 1.5, 38, 127, 0, True, 9), N.Note(2.0, 2.004, 72, 1, 40, False, 1),
               N.Note(3.3333, 4.75, 55, 64, 40, False, 1)], total_time=4.75,
        control_changes=[N.ControlChange(0.1, 64, 127, 0), N.ControlChange(0.9, 64, 0, 0)])


# SHA-256 of the bytes the writer gave for fixed_sequence() BEFORE it learned about beats (qpm 120, and qpm 90)
PARENT_SHA = "1ed3da6a7e84f7e91ee28f90f653d11353b3f3502cb68a4319bcc1af143cbf83"
PARENT_SHA_90 = "59d7dda4b81ec6221e8a9aa355ccc499878638673ca04d8fa5e46f73ea0a4684"
# what the reader gave for those bytes before it learned about tempo maps
PARENT_READ = [(0.0, 0.5), (0.25, 1.0), (1.0136363636363637, 1.5), (2.0, 2.0045454545454544), (3.334090909090909, 4.75)]


def test_without_beats_the_writer_gives_the_bytes_it_always_gave():
    ns = fixed_sequence()
    assert hashlib.sha256(midi_io.note_sequence_to_midi_bytes(ns)).hexdigest() == PARENT_SHA
    assert hashlib.sha256(midi_io.note_sequence_to_midi_bytes(ns, beats=None)).hexdigest() == PARENT_SHA
    assert hashlib.sha256(midi_io.note_sequence_to_midi_bytes(ns, qpm=90.0)).hexdigest() == PARENT_SHA_90


def test_a_single_tempo_file_reads_as_before():
    back = midi_io.midi_bytes_to_note_sequence(midi_io.note_sequence_to_midi_bytes(fixed_sequence()))
    assert _times(back) == PARENT_READ and back.total_time == 4.75
    assert [(c.time, c.control_value) for c in back.control_changes] == [(0.1, 127), (0.9, 0)]
    slow = midi_io.midi_bytes_to_note_sequence(midi_io.note_sequence_to_midi_bytes(fixed_sequence(), qpm=90.0))
    # one tempo at tick 0: tick * tempo / 1e6 / resolution, the parent's very expression
    assert [a for a, _ in _times(slow)] == [int(round(t * 220 * 90.0 / 60.0)) * 666667 / 1e6 / 220
                                            for t, _ in _times(fixed_sequence())]


@pytest.mark.parametrize("frames", [[37, 87, 139, 188, 240, 291, 340, 392, 445], [0, 50, 100, 151], [120, 160, 201]])
def test_a_tempo_map_round_trips(frames):
    b = [f / 100.0 for f in frames]
    ns = fixed_sequence()
    data = midi_io.note_sequence_to_midi_bytes(ns, beats=b)
    m, t0 = midi_io.preroll(b)
    assert t0 <= 0 < t0 + (b[1] - b[0]) and m == math.ceil(b[0] / (b[1] - b[0]) - 1e-9)
    # intervals of whole frames are whole microseconds: the tempo field holds them exactly, and only a tick's rounding
    # is left -- half a tick at the tempo of the interval the time lies in
    def half_tick(t):
        i = min(max(int(np.searchsorted(b, t, side="right")) - 1, 0), len(b) - 2)
        return 0.5 * (b[i + 1] - b[i]) / 220 + 1e-9
    back = midi_io.midi_bytes_to_note_sequence(data)
    assert len(back.notes) == len(ns.notes)
    for (s0, e0), (s1, e1) in zip(_times(ns), _times(back)):
        assert abs(s1 + t0 - s0) <= half_tick(s0)
        assert abs(e1 + t0 - e0) <= half_tick(e0) or e0 - s0 < 2 * half_tick(s0)      # (a note is at least one tick long)
    read = midi_io.midi_bytes_to_beats(data)
    assert len(read) >= m + len(b) - 1
    for i, t in enumerate(b[:len(read) - m]):
        assert abs(read[m + i] + t0 - t) <= 1e-6 * (m + i + 1)
    # every beat is a quarter note: set-tempo events on whole beats, one per beat but the last
    assert data.count(b"\xff\x51\x03") == len(b) - 1 + (1 if m else 0)


def test_tempo_rounding_stays_within_a_microsecond_per_beat():
    # intervals that are no whole microseconds: the 24-bit tempo field rounds each to the nearest, 0.5 us at the most, so
    # beat i is off by at most 0.5 us * i; the issue's bound of 1 us per beat holds with room
    b = np.cumsum(0.4 + 0.1 * np.sin(np.arange(40)) / math.pi).tolist()
    data = midi_io.note_sequence_to_midi_bytes(fixed_sequence(), beats=b)
    m, t0 = midi_io.preroll(b)
    read = midi_io.midi_bytes_to_beats(data)
    assert len(read) >= m + 10
    for i, t in enumerate(b[:len(read) - m]):
        assert abs(read[m + i] + t0 - t) <= 0.5e-6 * (m + i + 1) + 1e-9
        assert abs(read[m + i] + t0 - t) <= 1e-6 * (m + i + 1)


def test_the_writer_refuses_beats_it_cannot_write():
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0], [0.0, float("nan")], [0.0, 20.0]):
        with pytest.raises(ValueError, match="beat"):
            midi_io.note_sequence_to_midi_bytes(fixed_sequence(), beats=bad)
