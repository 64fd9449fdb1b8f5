"""Note containers and encoding specs (mirror of the decode half of mt3/note_sequences.py).

`NoteSequence` stands in for the `note_seq.NoteSequence` proto (fields the path
uses: notes[*].{start_time,end_time,pitch,velocity,program,is_drum,instrument},
total_time, ticks_per_quarter=220 -- note_sequences.py:281,307-310).  The note
state machine itself (note_sequences.py:262-408) lives in libmt3hip.so
(csrc/symbolic.cpp) and is selected by the spec objects below.
"""
from __future__ import annotations

import copy
import dataclasses
from typing import List

from . import _lib

DEFAULT_VELOCITY = 100
DEFAULT_NOTE_DURATION = 0.01
MIN_NOTE_DURATION = 0.01


@dataclasses.dataclass
class Note:
    start_time: float = 0.0
    end_time: float = 0.0
    pitch: int = 0
    velocity: int = 0
    program: int = 0
    is_drum: bool = False
    instrument: int = 0


@dataclasses.dataclass
class ControlChange:
    """One MIDI controller event (note_seq's NoteSequence.ControlChange, the fields the sustain rule reads)."""
    time: float = 0.0
    control_number: int = 0
    control_value: int = 0
    instrument: int = 0


@dataclasses.dataclass
class NoteSequence:
    notes: List[Note] = dataclasses.field(default_factory=list)
    total_time: float = 0.0
    ticks_per_quarter: int = 220
    control_changes: List[ControlChange] = dataclasses.field(default_factory=list)      # the last field: see DESIGN 6p


@dataclasses.dataclass
class TrackSpec:
    """One track to score on its own (note_sequences.py:35-39): the notes of one (program, is_drum), named."""
    name: str
    program: int = 0
    is_drum: bool = False


def extract_track(ns: NoteSequence, program: int, is_drum: bool) -> NoteSequence:
    """The notes of `ns` with exactly that program and drum flag, in their order (the notes are shared, not copied);
    total_time is their latest end, 0.0 without notes (note_sequences.py:42-49)."""
    notes = [n for n in ns.notes if n.program == program and bool(n.is_drum) == bool(is_drum)]
    return NoteSequence(notes=notes, total_time=max((n.end_time for n in notes), default=0.0), ticks_per_quarter=220)


def trim_overlapping_notes(ns: NoteSequence) -> NoteSequence:
    """Trim overlapping notes of one (pitch, program, is_drum), dropping zero-length notes (note_sequences.py:52-69).  A new
    sequence; `ns` is not touched."""
    ns_trimmed = copy.deepcopy(ns)
    channels = set((note.pitch, note.program, note.is_drum) for note in ns_trimmed.notes)
    for pitch, program, is_drum in channels:
        notes = [note for note in ns_trimmed.notes
                 if note.pitch == pitch and note.program == program and note.is_drum == is_drum]
        sorted_notes = sorted(notes, key=lambda note: note.start_time)
        for i in range(1, len(sorted_notes)):
            if sorted_notes[i - 1].end_time > sorted_notes[i].start_time:
                sorted_notes[i - 1].end_time = sorted_notes[i].start_time
    ns_trimmed.notes = [note for note in ns_trimmed.notes if note.start_time < note.end_time]
    return ns_trimmed


def validate_note_sequence(ns: NoteSequence) -> None:
    """Raise ValueError if `ns` contains invalid notes (note_sequences.py:87-94)."""
    for note in ns.notes:
        if note.start_time >= note.end_time:
            raise ValueError("note has start time >= end time: %f >= %f" % (note.start_time, note.end_time))
        if note.velocity == 0:
            raise ValueError("note has zero velocity")


SUSTAIN_CONTROL_NUMBER = 64
_SUS_ON, _SUS_OFF, _NOTE_ON, _NOTE_OFF = range(4)


def apply_sustain_control_changes(ns: NoteSequence, sustain_control_number: int = SUSTAIN_CONTROL_NUMBER) -> NoteSequence:
    """The notes of `ns` as they sound under its sustain pedal (controller 64, down from value 64 on): a note whose key goes
    up while its instrument's pedal is down lasts until the pedal goes up, or until the same pitch is struck again under the
    pedal.  note_seq.apply_sustain_control_changes, event by event [from memory: parity unpinned against note_seq].  A new
    sequence, its control changes kept; `ns` is not touched.  The yardstick of mt3_op_prepare_notes: DESIGN 6p."""
    out = copy.deepcopy(ns)
    events = [(n.start_time, _NOTE_ON, n) for n in out.notes] + [(n.end_time, _NOTE_OFF, n) for n in out.notes]
    events += [(cc.time, _SUS_ON if cc.control_value >= 64 else _SUS_OFF, cc) for cc in out.control_changes
               if cc.control_number == sustain_control_number]
    events.sort(key=lambda e: (e[0], e[1]))                  # stable: the order above breaks ties
    active, sus, removed, time = {}, {}, set(), 0
    for time, kind, value in events:
        inst = value.instrument
        notes = active.setdefault(inst, [])
        if kind == _SUS_ON:
            sus[inst] = True
        elif kind == _SUS_OFF:
            sus[inst] = False
            still = []
            for note in notes:
                if note.end_time < time:
                    note.end_time = time
                    out.total_time = max(out.total_time, time)
                else:
                    still.append(note)
            active[inst] = still
        elif kind == _NOTE_ON:
            if sus.get(inst, False):
                still = []
                for note in notes:
                    if note.pitch == value.pitch:
                        note.end_time = time
                        if note.start_time == note.end_time:
                            removed.add(id(note))
                    else:
                        still.append(note)
                active[inst] = notes = still
            notes.append(value)
        elif not sus.get(inst, False):                       # _NOTE_OFF
            active[inst] = [note for note in notes if note is not value]
    for notes in active.values():
        for note in notes:
            note.end_time = time
            out.total_time = time
    out.notes = [note for note in out.notes if id(note) not in removed]
    return out


def sustain_reference(ns: NoteSequence) -> NoteSequence:
    """What the reference tokenizes and stores for evaluation (preprocessors.py:154-160): the sustained notes, the control
    changes cleared."""
    out = apply_sustain_control_changes(ns)
    out.control_changes = []
    return out


@dataclasses.dataclass(frozen=True)
class NoteEncodingSpecType:
    """Which decoder the C library runs (note_sequences.py:411-446)."""
    name: str
    spec_id: int


NoteOnsetEncodingSpec = NoteEncodingSpecType("NoteOnsetEncodingSpec", _lib.SPEC_ONSETS)
NoteEncodingSpec = NoteEncodingSpecType("NoteEncodingSpec", _lib.SPEC_NOTES)
NoteEncodingWithTiesSpec = NoteEncodingSpecType("NoteEncodingWithTiesSpec", _lib.SPEC_TIES)


# ---------------------------------------------------------------------------------------------
# Encode side (mirror of note_sequences.py:141-259): NoteSequence -> timed
# event data -> codec events.  Host integer work; used to synthesise valid token streams.
import itertools  # noqa: E402
from typing import Optional, Sequence, Tuple  # noqa: E402

from . import event_codec  # noqa: E402
from . import vocabularies  # noqa: E402


@dataclasses.dataclass
class NoteEventData:
    pitch: int
    velocity: Optional[int] = None
    program: Optional[int] = None
    is_drum: Optional[bool] = None
    instrument: Optional[int] = None


@dataclasses.dataclass
class NoteEncodingState:
    """velocity bin of every (pitch, program) seen so far (0 = off)."""
    active_pitches: dict = dataclasses.field(default_factory=dict)


def note_sequence_to_onsets(ns: NoteSequence):
    notes = sorted(ns.notes, key=lambda n: n.pitch)          # pitch = tie-break of the later stable sort
    return [n.start_time for n in notes], [NoteEventData(pitch=n.pitch) for n in notes]


def note_sequence_to_onsets_and_offsets(ns: NoteSequence):
    """offsets listed before onsets so that, at equal times, offsets sort first."""
    notes = sorted(ns.notes, key=lambda n: n.pitch)
    times = [n.end_time for n in notes] + [n.start_time for n in notes]
    values = ([NoteEventData(pitch=n.pitch, velocity=0) for n in notes] +
              [NoteEventData(pitch=n.pitch, velocity=n.velocity) for n in notes])
    return times, values


def note_sequence_to_onsets_and_offsets_and_programs(ns: NoteSequence):
    notes = sorted(ns.notes, key=lambda n: (n.is_drum, n.program, n.pitch))
    pitched = [n for n in notes if not n.is_drum]            # drums have no offsets
    times = [n.end_time for n in pitched] + [n.start_time for n in notes]
    values = ([NoteEventData(pitch=n.pitch, velocity=0, program=n.program, is_drum=False) for n in pitched] +
              [NoteEventData(pitch=n.pitch, velocity=n.velocity, program=n.program, is_drum=n.is_drum)
               for n in notes])
    return times, values


def note_event_data_to_events(state: Optional[NoteEncodingState], value: NoteEventData,
                              codec: event_codec.Codec) -> Sequence[event_codec.Event]:
    E = event_codec.Event
    if value.velocity is None:
        return [E("pitch", value.pitch)]
    vbin = vocabularies.velocity_to_bin(value.velocity, vocabularies.num_velocity_bins_from_codec(codec))
    if value.program is None:
        if state is not None:
            state.active_pitches[(value.pitch, 0)] = vbin
        return [E("velocity", vbin), E("pitch", value.pitch)]
    if value.is_drum:
        return [E("velocity", vbin), E("drum", value.pitch)]
    if state is not None:
        state.active_pitches[(value.pitch, int(value.program))] = vbin
    return [E("program", value.program), E("velocity", vbin), E("pitch", value.pitch)]


def note_encoding_state_to_events(state: NoteEncodingState) -> Sequence[event_codec.Event]:
    """program/pitch pairs of the sounding notes (sorted by program, then pitch) + the `tie` marker."""
    E = event_codec.Event
    out = []
    for pitch, program in sorted(state.active_pitches, key=lambda k: (k[1], k[0])):
        if state.active_pitches[(pitch, program)]:
            out += [E("program", program), E("pitch", pitch)]
    out.append(E("tie", 0))
    return out


# what the three specs use on the encode side (note_sequences.py:416-446)
ENCODING_FNS = {
    "NoteOnsetEncodingSpec": (lambda: None, note_event_data_to_events, None),
    "NoteEncodingSpec": (lambda: None, note_event_data_to_events, None),
    "NoteEncodingWithTiesSpec": (NoteEncodingState, note_event_data_to_events, note_encoding_state_to_events),
}
