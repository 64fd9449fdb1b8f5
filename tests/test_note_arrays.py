"""mt3_amd/note_arrays.py: the one extraction of a NoteSequence's columns, the shared checks, offset tables and the byte
layout of an upload.  No GPU."""
import numpy as np
import pytest

from mt3_amd import metrics_utils, note_arrays
from mt3_amd.note_sequences import Note, NoteSequence

NOTES = [(0.5, 1.25, 60, 100, 3, False), (0.0, 0.5, 38, 90, 0, True), (2.0, 2.0, 127, 0, 127, False)]


def _both(notes):
    ns = NoteSequence(notes=[Note(start_time=s, end_time=e, pitch=p, velocity=v, program=g, is_drum=d) for s, e, p, v, g, d in notes])
    rec = np.zeros(len(notes), metrics_utils.NOTE_DTYPE)
    for i, (s, e, p, v, g, d) in enumerate(notes):
        rec[i] = (s, e, p, v, g, d, 0, 0)
    return ns, rec


@pytest.mark.parametrize("notes", [NOTES, []], ids=["three", "empty"])
def test_fields_of_a_sequence_and_of_its_record_array_are_equal(notes):
    ns, rec = _both(notes)
    for program in (False, True):
        a, b = note_arrays.fields(ns, program), note_arrays.fields(rec, program)
        assert len(a) == len(b) == (6 if program else 5)
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.dtype == y.dtype == (np.float64 if k < 2 else np.int64) and x.shape == y.shape == (len(notes),)
            assert x.tolist() == y.tolist()
    start, end, pitch, velocity, drum, program = note_arrays.fields(ns, program=True)
    assert (start.tolist(), end.tolist()) == ([n[0] for n in notes], [n[1] for n in notes])
    assert (pitch.tolist(), velocity.tolist()) == ([n[2] for n in notes], [n[3] for n in notes])
    assert (program.tolist(), drum.tolist()) == ([n[4] for n in notes], [int(n[5]) for n in notes])


def test_offsets():
    assert note_arrays.offsets([]).tolist() == [0] and note_arrays.offsets([]).dtype == np.int64
    assert note_arrays.offsets([0, 3, 0]).tolist() == [0, 0, 3, 3]
    big = note_arrays.offsets(np.array([2 ** 31 - 1, 2 ** 31 - 1], np.int32))        # summed in int64 whatever comes in
    assert big.tolist() == [0, 2 ** 31 - 1, 2 ** 32 - 2] and big.dtype == np.int64


@pytest.mark.parametrize("n", [0, 1, 5])
def test_column_offsets_of_the_render_layout(n):
    assert note_arrays.column_offsets([8, 8, 8, 4, 4, 4], n) == [0, 8 * n, 16 * n, 24 * n, 28 * n, 32 * n]


def test_a_column_that_would_start_off_its_alignment_is_refused():
    for n in (1, 5):
        with pytest.raises(ValueError, match="wider columns first"):
            note_arrays.column_offsets([4, 8], n)
        with pytest.raises(ValueError, match="wider columns first"):
            note_arrays.pack([[np.zeros(n)], [np.zeros(n)]], ("<i4", "<f8"))
    assert note_arrays.column_offsets([4, 8], 2) == [0, 8]          # an even count happens to keep the f64 column aligned


def test_pack_lays_the_columns_back_to_back():
    packed = note_arrays.pack([[np.array([1.5]), np.array([-2.0])], [np.array([7, -1])]], ("<f8", "<i4"))
    assert packed.dtype == np.uint8 and packed.size == 24
    assert packed[:16].view("<f8").tolist() == [1.5, -2.0] and packed[16:].view("<i4").tolist() == [7, -1]
    assert note_arrays.pack([[], []], ("<f8", "<i4")).size == 0
    assert note_arrays.upload(packed[:0], 0, ("<f8", "<i4")) == (None, [None, None])        # no items: nothing is uploaded


def test_the_time_check():
    good = np.array([0.0, 1.5])
    note_arrays.check_times(good, good[:0])
    note_arrays.check_times(np.array([-1.0, 2.0]))                  # a negative time is refused only where asked
    for bad in (np.array([0.0, np.nan]), np.array([np.inf, 1.0]), np.array([-np.inf])):
        with pytest.raises(ValueError, match="^note times must be finite$"):
            note_arrays.check_times(good, bad)
        with pytest.raises(ValueError, match="^sequence 3: note times must be finite and not negative$"):
            note_arrays.check_times(bad, good, not_negative=True, prefix="sequence 3: ")
    with pytest.raises(ValueError, match="finite and not negative"):
        note_arrays.check_times(good, np.array([1.0, -0.5]), not_negative=True)


def test_the_range_check():
    good = np.array([0, 64, 127])
    note_arrays.check_range("pitches", good, good[:0])
    for bad in (-1, 128):
        with pytest.raises(ValueError, match="^sequence 2: pitches are 0 .. 127, got %d$" % bad):
            note_arrays.check_range("sequence 2: pitches are 0 .. 127", np.array([5, bad, 300]))
    with pytest.raises(ValueError, match="^velocities are 0 .. 127, got 128$"):
        note_arrays.check_range("velocities are 0 .. 127", good, np.array([128]))
    with pytest.raises(ValueError, match=r"^pitches, programs and velocities must be in 0 \.\. 127$"):
        note_arrays.check_range("pitches, programs and velocities must be in 0 .. 127", good, good, np.array([128]), got=False)
