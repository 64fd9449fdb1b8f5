"""The numpy statement of the harmony rule (mt3_amd/harmony.py) on hand-computed literals, the key table, the progressions
of tests/harmony_cases.py with the counts DESIGN.md section 6t records (zero), the MIDI round trip of the signatures and
markers, and every ValueError of `analyze` and `analyze_reference`."""
import numpy as np
import pytest

from mt3_amd import harmony, midi_io
from mt3_amd import note_sequences as N
from tests import harmony_cases as hc


def columns(notes):
    """(s, e, key) of (start frame, end frame, pitch[, drum]) tuples"""
    s, e, k = (np.array([n[i] for n in notes], np.int64) for i in range(3))
    return s, e, k + 256 * np.array([len(n) > 3 and n[3] for n in notes], np.int64)


def test_a_c_major_triad_over_four_beats():
    b = np.array([30, 70, 110, 150], np.int32)
    s, e, key = columns([(30, 190, 48), (30, 190, 52), (30, 190, 55)])
    assert harmony.intervals(b).tolist() == [30, 70, 110, 150, 190]
    R, H, tot, low, length = harmony.beat_roll(s, e, key, b)
    assert R.dtype == np.int32 and R.sum() == 480 and (R[:, [48, 52, 55]] == 40).all()
    assert H.tolist() == [[40, 0, 0, 0, 40, 0, 0, 40, 0, 0, 0, 0]] * 4 and tot.tolist() == [120] * 4
    assert low.tolist() == [48] * 4 and length.tolist() == [40] * 4
    E, Q = harmony.emissions(H, tot, low)
    # C: 2 * 120 + the bass's 40; Cm: C and G and the bass; Em, Am: two tones; G, F: one tone; D: none
    assert [int(E[0, k]) for k in (0, 1, 2, 10, 20, 15, 11, 5)] == [0, 280, 160, 120, 120, 0, 0, -120]
    assert [int(Q[0, k]) for k in (0, 1, 2, 10, 20, 15, 11, 5)] == [0, 597, 341, 256, 256, 0, 0, -256]
    assert (Q == Q[0]).all() and Q.min() == -256
    chords, score = harmony.chord_path(Q, harmony.DEFAULT_CHANGE_PENALTY)
    assert chords.tolist() == [1, 1, 1, 1] and chords.dtype == np.int8 and score == 4 * 597
    a = harmony.accents(s, key, b, low, chords, 1, 4, 2)
    assert a.tolist() == [5, 0, 0, 0]                                      # three onsets and the struck bass on beat 0
    assert harmony.meter_scores(a) == {(2, 0): (5 << 16) // 2, (2, 1): -((5 << 16) // 2)}      # B = 4 admits m = 2 alone
    assert harmony.meter(a) == (2, 0)
    D = harmony.durations(s, e, key)
    assert D.tolist() == [160, 0, 0, 0, 160, 0, 0, 160, 0, 0, 0, 0]
    assert harmony.key_scores(D)[0] == 160 * (2684 + 840 + 1598) and int(np.argmax(harmony.key_scores(D))) == 0


def test_a_single_note_and_the_tie_of_its_two_triads():
    b = np.array([30, 70, 110], np.int32)
    s, e, key = columns([(50, 90, 61)])
    R, H, tot, low, _ = harmony.beat_roll(s, e, key, b)
    assert R[:, 61].tolist() == [20, 20, 0] and R.sum() == 40 and tot.tolist() == [20, 20, 0]
    assert low.tolist() == [61, 61, -1]                                    # 4 * 20 >= 40
    _, Q = harmony.emissions(H, tot, low)
    want = np.full(25, -256)
    want[[0, 3, 4, 13, 14, 19, 22]] = [0, 768, 768, 512, 512, 512, 512]    # C#, C#m (root and bass); F#, F#m, A, Bbm (a tone)
    assert Q[0].tolist() == want.tolist() and Q[1].tolist() == want.tolist() and not Q[2].any()
    assert harmony.chord_path(Q, harmony.DEFAULT_CHANGE_PENALTY)[0].tolist() == [3, 3, 3]     # the lower of the tied states
    # free changes: every state reaches the silent beat with 1536, and the lowest of them is N
    chords, score = harmony.chord_path(Q, 0)
    assert chords.tolist() == [3, 3, 0] and score == 1536
    scores = harmony.key_scores(harmony.durations(s, e, key))
    assert scores[2] == 2684 * 40 and scores[3] == 2683 * 40 and int(np.argmax(scores)) == 2


def test_silence_is_no_chord_no_key_and_no_meter():
    h = harmony.analyze_reference([N.NoteSequence()], [hc.grid(6)])[0]
    assert (h.key, h.key_name, h.sharps, h.chord_score, h.beats_per_bar, h.downbeat) == (-1, "", 0, 0, 0, -1)
    assert h.chords.tolist() == [0] * 6 and not h.key_scores.any() and len(h.downbeats) == 0
    assert h.segments == [(0.3, 2.7, "N")]


def test_the_floor_of_a_negative_score():
    b = hc.grid(4)
    s, e, key = columns([(30, 37, 60), (40, 43, 61), (70, 110, 60)])
    _, H, tot, low, _ = harmony.beat_roll(s, e, key, b)
    E, Q = harmony.emissions(H, tot, low)
    assert tot[0] == 10 and E[0, 19] == 3 * 3 - 10 and Q[0, 19] == -26     # A major holds the C# alone: -256 / 10 floors
    assert E[0, 11] == 3 * 7 - 10 and Q[0, 11] == 281                       # F major holds the C alone: 2816 / 10


def test_the_tie_orders_of_the_meter():
    scores = harmony.meter_scores([1, 1, 0, 0, 1, 1, 0, 0])
    assert scores[(4, 0)] == scores[(4, 1)] == 65536 - 131072 // 6 == 43691 and scores[(4, 2)] == -(262144 // 6)
    assert scores[(2, 0)] == 0 and scores[(3, 1)] == 131072 // 3 - 131072 // 5
    assert list(scores) == [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3)]
    assert harmony.meter([1, 1, 0, 0, 1, 1, 0, 0]) == (4, 0)               # the lower phase
    assert harmony.meter([1, 0, 1, 0, 1, 0, 1, 0]) == (2, 0)               # m = 2 and m = 4 both reach 65536: the lower m
    assert harmony.meter([1] * 8) == (0, -1) and harmony.meter([0] * 8) == (0, -1)
    assert harmony.meter([3, 0, 0]) == (0, -1) and harmony.meter_scores([3, 0, 0]) == {}       # B < 4: nothing admissible
    assert set(m for m, _ in harmony.meter_scores([1] * 5)) == {2} and set(m for m, _ in harmony.meter_scores([1] * 6)) == {2, 3}


def test_the_key_profiles():
    K = harmony.key_profiles()
    assert K.dtype == np.int32 and K.shape == (24, 12) and not K.flags.writeable
    assert K[0].tolist() == [2684, -1172, -2, -1079, 840, 569, -901, 1598, -1023, 166, -1116, -564]
    assert K[1].tolist() == [2683, -1054, -194, 1711, -1136, -183, -1197, 1066, 277, -1043, -378, -552]
    for t in range(12):
        for q in (0, 1):
            assert K[2 * t + q].tolist() == np.roll(K[q], t).tolist()
    # the same order as the Pearson correlation, on a duration profile with a clear answer
    D = np.array([9, 0, 4, 0, 6, 5, 0, 8, 0, 3, 0, 2], np.int64)
    r = [np.corrcoef(D, np.roll(p, t))[0, 1] for t in range(12) for p in (harmony.KK_MAJOR, harmony.KK_MINOR)]
    # score / (4096 * norm(D - mean D)) is the correlation, up to the rounding of K: at most half a unit per class
    norm = 4096.0 * np.sqrt(((D - D.mean()) ** 2).sum())
    assert np.abs(harmony.key_scores(D) / norm - np.array(r)).max() <= 0.5 * D.sum() / norm
    assert int(np.argmax(harmony.key_scores(D))) == int(np.argmax(r)) == 0


def test_sharps_and_names_of_all_24_keys():
    major = {0: 0, 7: 1, 2: 2, 9: 3, 4: 4, 11: 5, 6: 6, 5: -1, 10: -2, 3: -3, 8: -4, 1: -5}    # the circle of fifths
    assert len(harmony.SHARPS) == 24 and all(-7 <= v <= 7 for v in harmony.SHARPS)
    for t in range(12):
        assert harmony.SHARPS[2 * t] == major[t] and harmony.SHARPS[2 * t + 1] == major[(t + 3) % 12]
    assert [harmony.key_name(k) for k in (0, 6, 7, 19, 21, 12)] == ["C major", "Eb major", "D# minor", "A minor", "Bb minor",
                                                                     "F# major"]
    assert harmony.chord_name(0) == "N" and harmony.chord_name(7, 6) == "Eb" and harmony.chord_name(7, 0) == "D#"
    assert harmony.chord_name(20) == "Am" and harmony.chord_name(22, 21) == "Bbm"
    with pytest.raises(ValueError, match="a chord state is 0 .. 24"):
        harmony.chord_name(25)


@pytest.mark.parametrize("jitter", [0, 2])
def test_every_label_of_every_progression_is_recovered(jitter):
    """with the defaults the rule makes no error on the 32 clean and the 32 jittered progressions
    (block triads and arpeggios): key, chord of every beat, bar length and downbeat phase."""
    cases = hc.progressions(jitter)
    assert len(cases) == 32 and {c[3]["beats_per_bar"] for c in cases} == {3, 4} and {c[3]["downbeat"] for c in cases} == {0, 1, 2, 3}
    found = harmony.analyze_reference([c[1] for c in cases], [c[2] for c in cases])
    for (name, _, beats, truth), h in zip(cases, found):
        assert h.key == truth["key"], name
        assert h.chords.tolist() == truth["chords"].tolist(), name
        assert (h.beats_per_bar, h.downbeat) == (truth["beats_per_bar"], truth["downbeat"]), name
        assert h.downbeats.tolist() == (beats[truth["downbeat"]::truth["beats_per_bar"]] / 100.0).tolist(), name


def test_the_ends_of_the_recorded_range_of_the_change_penalty():
    """512 .. 1202 recovers everything; one step outside either end does not"""
    cases = hc.progressions(0) + hc.progressions(2)

    def wrong(penalty):
        found = harmony.analyze_reference([c[1] for c in cases], [c[2] for c in cases], penalty)
        return sum(int((h.chords != c[3]["chords"]).sum()) for c, h in zip(cases, found))

    assert wrong(512) == 0 and wrong(1202) == 0 and wrong(511) > 0 and wrong(1203) > 0
    assert harmony.DEFAULT_CHANGE_PENALTY == (512 + 1202) // 2


def test_the_midi_round_trip():
    name, ns, b, truth = hc.progressions(0)[16 + 2]                         # A minor, 3/4, one beat of lead-in
    assert truth["downbeat"] == 1 and truth["beats_per_bar"] == 3
    h = harmony.analyze_reference([ns], [b])[0]
    times = b / 100.0
    plain = midi_io.note_sequence_to_midi_bytes(ns, beats=times)
    assert midi_io.note_sequence_to_midi_bytes(ns, beats=times, harmony=None) == plain
    assert midi_io.note_sequence_to_midi_bytes(ns) == midi_io.note_sequence_to_midi_bytes(ns, 120.0, None, None)
    data = midi_io.note_sequence_to_midi_bytes(ns, beats=times, harmony=h)
    assert midi_io.preroll(times) == (1, times[0] - 0.5) and midi_io.preroll(times, None) == midi_io.preroll(times)
    m, t0 = midi_io.preroll(times, h)
    assert m == 2 and (m + h.downbeat) % h.beats_per_bar == 0               # one more beat: tick 0 is a downbeat
    read = midi_io.midi_bytes_to_signatures(data)
    assert read["key_signatures"] == [(0.0, 0, 1)] and read["time_signatures"] == [(0.0, 3, 4)]
    assert [text for _, text in read["markers"]] == [name for _, _, name in h.segments] == ["Am", "Dm", "E", "Am", "Dm", "E", "Am"]
    assert np.allclose([t + t0 for t, _ in read["markers"]], [start for start, _, _ in h.segments], rtol=0, atol=1e-9)
    beats_read = midi_io.midi_bytes_to_beats(data)
    assert np.allclose(np.array(beats_read[m: m + len(times)]) + t0, times[:len(beats_read) - m], rtol=0, atol=1e-9)
    back, source = midi_io.midi_bytes_to_note_sequence(data), midi_io.midi_bytes_to_note_sequence(plain)
    assert [(n.pitch, n.velocity, n.program, n.is_drum) for n in back.notes] == \
           [(n.pitch, n.velocity, n.program, n.is_drum) for n in source.notes]
    assert np.allclose([n.start_time + t0 for n in back.notes], [n.start_time + midi_io.preroll(times)[1] for n in source.notes],
                       rtol=0, atol=1e-6)
    assert midi_io.midi_bytes_to_signatures(plain) == {"key_signatures": [], "time_signatures": [], "markers": []}
    # no key, no meter, N: only the N.C. marker is written
    silent = harmony.analyze_reference([N.NoteSequence()], [b])[0]
    quiet = midi_io.midi_bytes_to_signatures(midi_io.note_sequence_to_midi_bytes(N.NoteSequence(), beats=times, harmony=silent))
    assert quiet["key_signatures"] == [] and quiet["time_signatures"] == [] and [t for _, t in quiet["markers"]] == ["N.C."]
    flat = harmony.analyze_reference([hc.progressions(0)[4][1]], [hc.progressions(0)[4][2]])[0]      # Eb major: three flats
    ks = midi_io.midi_bytes_to_signatures(midi_io.note_sequence_to_midi_bytes(
        hc.progressions(0)[4][1], beats=hc.progressions(0)[4][2] / 100.0, harmony=flat))["key_signatures"]
    assert ks == [(0.0, -3, 0)] and flat.segments[0][2] == "Eb"
    with pytest.raises(ValueError, match="harmony= needs the beats"):
        midi_io.note_sequence_to_midi_bytes(ns, harmony=h)
    with pytest.raises(ValueError, match="harmony has 25 chords for 24 beats"):
        midi_io.note_sequence_to_midi_bytes(ns, beats=times[:-1], harmony=h)


def _one(start=0.0, end=None, pitch=60):
    return N.NoteSequence(notes=[N.Note(start, start + 0.1 if end is None else end, pitch, 90)])


@pytest.mark.parametrize("call", [harmony.analyze, harmony.analyze_reference])
def test_every_value_error_before_anything_is_uploaded(call):
    two = [np.array([10, 60]), np.array([10, 60])]
    for bad in (_one(), "notes", [_one(), 3], None):
        with pytest.raises(ValueError, match="analyze takes a list of NoteSequences"):
            call(bad, two)
    with pytest.raises(ValueError, match="beats has 1 entries for 2 sequences"):
        call([_one(), _one()], two[:1])
    with pytest.raises(ValueError, match="analyze takes one entry of beats per sequence"):
        call([_one(), _one()], 7)
    for bad in (float("nan"), float("inf"), -0.01):
        with pytest.raises(ValueError, match="file 1: note times must be finite and not negative"):
            call([_one(), _one(bad, 1.0)], two)
    for pitch in (-1, 128):
        with pytest.raises(ValueError, match="file 1: pitches must be 0 .. 127, got %d" % pitch):
            call([_one(), _one(pitch=pitch)], two)
    with pytest.raises(ValueError, match="file 0: a note ends at frame 1048577; a file has at most 1048576 frames"):
        call([_one(10485.0, 10485.77), _one()], two)
    for bad in ([10, 10], [60, 10], [-1, 5], [10, 1 << 20], np.array([0.5, 1.5])):
        with pytest.raises(ValueError, match="file 1: beat frames must be strictly ascending whole numbers, 0 .. 1048575"):
            call([_one(), _one()], [two[0], np.asarray(bad)])
    many = N.NoteSequence(notes=[N.Note(0.0, 0.1, 60, 90)] * 4096)
    with pytest.raises(ValueError, match="file 0: 4096 notes times its longest beat interval \\(524288 frames\\) must stay"):
        call([many], [np.array([0, 1 << 19])])
    for kw, text in ((dict(change_penalty=-1), "change_penalty must be an int 0 .. 1048576, got -1"),
                     (dict(change_penalty=(1 << 20) + 1), "change_penalty must be an int 0 .. 1048576"),
                     (dict(change_penalty=3.0), "change_penalty must be an int"),
                     (dict(change_penalty=True), "change_penalty must be an int"),
                     (dict(onset_weight=256), "onset_weight must be an int 0 .. 255, got 256"),
                     (dict(change_weight=-1), "change_weight must be an int 0 .. 255, got -1"),
                     (dict(bass_weight=1.5), "bass_weight must be an int 0 .. 255, got 1.5")):
        with pytest.raises(ValueError, match=text):
            call([_one(), _one()], two, **kw)


def test_records_and_beats_objects_are_accepted_and_the_order_of_the_notes_does_not_matter():
    from mt3_amd import beats as beat_tracking, metrics_utils
    name, ns, b, truth = hc.progressions(2)[5]
    want = harmony.analyze_reference([ns], [b])[0]
    rec = np.zeros(len(ns.notes), metrics_utils.NOTE_DTYPE)
    for i, n in enumerate(ns.notes[::-1]):
        rec[i]["start_time"], rec[i]["end_time"], rec[i]["pitch"], rec[i]["velocity"] = n.start_time, n.end_time, n.pitch, 90
        rec[i]["is_drum"] = n.is_drum
    wrapped = beat_tracking.Beats(b / 100.0, b, 50, 120.0, 0)
    got = harmony.analyze_reference([rec], [wrapped])[0]
    assert got.chords.tolist() == want.chords.tolist() and got.key == want.key and got.segments == want.segments
    assert np.array_equal(got.key_scores, want.key_scores) and (got.beats_per_bar, got.downbeat) == (want.beats_per_bar, want.downbeat)
