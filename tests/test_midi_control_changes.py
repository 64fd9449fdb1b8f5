"""Controller events through mt3_amd/midi_io.py: written with the notes and read back, a file without them byte for byte
what the writer gave before it knew them, running status across controller and note events, SysEx skipped."""
import struct

from mt3_amd import midi_io
from mt3_amd import note_sequences as NS

# note_sequence_to_midi_bytes of `_plain()` before control changes existed
PLAIN = bytes.fromhex(
    "4d546864000000060001000400dc4d54726b0000000b00ff510307a12000ff2f004d54726b0000001000c00000903c64815c803c0000ff2f00"
    "4d54726b0000001100c121815c914050815c81400000ff2f004d54726b0000001000c9006e99265a824a89260000ff2f00")


def _plain():
    return NS.NoteSequence(notes=[NS.Note(0.0, 0.5, 60, 100), NS.Note(0.25, 1.0, 38, 90, 0, True, 9),
                                  NS.Note(0.5, 1.0, 64, 80, 33, False, 1)], total_time=1.0)


def test_a_file_without_controllers_is_written_as_before():
    assert midi_io.note_sequence_to_midi_bytes(_plain()) == PLAIN


def test_round_trip_of_notes_and_controllers():
    tick = 60.0 / 120.0 / 220                                # seconds per tick: times on the grid come back exactly
    ns = NS.NoteSequence(notes=[NS.Note(0.0, 110 * tick, 60, 100), NS.Note(55 * tick, 220 * tick, 38, 90, 0, True, 9)],
                         total_time=220 * tick)
    ns.control_changes = [NS.ControlChange(0.0, 64, 127, 0), NS.ControlChange(110 * tick, 64, 0, 0),
                          NS.ControlChange(55 * tick, 64, 70, 0), NS.ControlChange(30 * tick, 1, 5, 0),
                          NS.ControlChange(40 * tick, 64, 100, 9)]
    back = midi_io.midi_bytes_to_note_sequence(midi_io.note_sequence_to_midi_bytes(ns))
    assert back.notes == ns.notes and back.total_time == ns.total_time
    assert back.control_changes == sorted(ns.control_changes, key=lambda c: c.time)
    # the pedal's event at a tick comes before the notes of that tick: note_seq's order of events
    data = midi_io.note_sequence_to_midi_bytes(ns)
    assert data.index(bytes([0xB0, 64, 127])) < data.index(bytes([0x90, 60, 100]))
    assert NS.apply_sustain_control_changes(back).notes[0].end_time == 110 * tick        # held to the release, exactly


def test_a_pedal_without_notes_gets_a_track_of_its_own():
    ns = NS.NoteSequence(control_changes=[NS.ControlChange(0.5, 64, 127, 0), NS.ControlChange(1.0, 64, 0, 0)])
    back = midi_io.midi_bytes_to_note_sequence(midi_io.note_sequence_to_midi_bytes(ns))
    assert back.notes == [] and back.control_changes == ns.control_changes


def _file(body: bytes, resolution=220) -> bytes:
    body += b"\x00\xff\x2f\x00"
    return b"MThd" + struct.pack(">IHHH", 6, 0, 1, resolution) + b"MTrk" + struct.pack(">I", len(body)) + body


def test_running_status_across_controller_and_note_events():
    # tempo 500000 (the default): a tick is 1 / 440 s.  B0 64 127, then 64 0 under running status; 90 60 100, then
    # 60 0 (a note-off as velocity 0) under running status; B0 again after the notes
    body = (b"\x00\xb0\x40\x7f" + b"\x6e\x40\x00" + b"\x00\x90\x3c\x64" + b"\x6e\x3c\x00" + b"\x00\xb0\x40\x40"
            + b"\x00\x01\x07")
    ns = midi_io.midi_bytes_to_note_sequence(_file(body))
    assert ns.notes == [NS.Note(0.25, 0.5, 60, 100, 0, False, 0)]
    assert ns.control_changes == [NS.ControlChange(0.0, 64, 127, 0), NS.ControlChange(0.25, 64, 0, 0),
                                  NS.ControlChange(0.5, 64, 64, 0), NS.ControlChange(0.5, 1, 7, 0)]


def test_a_sysex_in_the_stream_is_skipped():
    sysex = b"\x00\xf0\x05\x7e\x7f\x09\x01\xf7"                   # GM system on: F0, length 5, payload ending in F7
    long = b"\x00\xf0\x81\x02" + bytes([0x90] * 129) + b"\xf7"    # a two-byte length (130), data that looks like status
    escape = b"\x00\xf7\x02\x90\x3c"                              # F7 escape form
    body = sysex + b"\x00\xb9\x40\x7f" + long + b"\x00\x90\x3c\x64" + escape + b"\x6e\x80\x3c\x00"
    ns = midi_io.midi_bytes_to_note_sequence(_file(body))
    assert ns.notes == [NS.Note(0.0, 0.25, 60, 100, 0, False, 0)]
    assert ns.control_changes == [NS.ControlChange(0.0, 64, 127, 9)]
