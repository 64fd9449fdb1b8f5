"""NoteSequence -> Standard MIDI File (the notebook ends with
`note_seq.sequence_proto_to_midi_file(est_ns, path)`).

note_seq / pretty_midi are not available here, so this is a from-scratch SMF type-1 writer (and a
reader, for round-trip tests) following their conventions: resolution = `ticks_per_quarter` (220),
one tempo of 120 qpm at tick 0, tick = round(time * resolution * qpm / 60), one track per
(instrument, program, is_drum), drums on channel 9.  PARITY UNPINNED against note_seq's writer.
Controller events (`NoteSequence.control_changes`: the sustain pedal of piano files) are written onto the channel their
instrument's notes use, and read back; the reader numbers instruments 9 (channel 9) or 0 (every other channel), so the
pedal of any non-drum channel holds the notes of all of them: right for piano files, a stated limit otherwise.
TEMPO MAPS.  With `beats=` (ascending times in seconds, at least two: `mt3_amd.beats.track(...)[i].times`) the writer puts
beat i on tick (m + i) * resolution -- every beat is one quarter note -- and a set-tempo event of
round(1e6 * (b[i+1] - b[i])) microseconds per quarter on every beat but the last, after which the last tempo holds.  A
time t in interval i is tick round((m + i + (t - b[i]) / (b[i+1] - b[i])) * resolution); before the first beat the first
interval is extended backwards over m = `preroll(beats)[0]` whole beats, the fewest that put tick 0 at or before time 0.
Tick 0 is therefore time b[0] - m * (b[1] - b[0]) <= 0, and a file read back runs later than its source by minus that.
The reader keeps every set-tempo event with its tick (on equal ticks the last one read) and converts ticks to seconds
through the map; `midi_bytes_to_beats` returns the quarter-note ticks' times.  The tempo field is a whole number of
microseconds, so a written interval is off by at most 0.5 us; beats on the tracker's 10 ms frames are written exactly.
SIGNATURES AND CHORDS.  With `harmony=` (a `mt3_amd.harmony.Harmony` of the same beats; `beats=` is then required) the
tempo map's track also gets a key-signature event FF 59 02 sf mi at tick 0 when a key was found, a time-signature event
FF 58 04 nn 02 18 08 at tick 0 when a meter was found (nn quarter notes per bar), and a marker FF 06 with the chord's name
on the beat of every chord change (`N` is written `N.C.`).  The preroll then grows by the fewest whole beats that put a
downbeat on tick 0, so the bar lines of an editor fall on the downbeats.  `midi_bytes_to_signatures` reads the three kinds
of event back with their times.
"""
from __future__ import annotations

import bisect
import math
import struct
from typing import Dict, List, Optional, Sequence, Tuple

from .note_sequences import ControlChange, Note, NoteSequence

DEFAULT_QPM = 120.0


def _vlq(n: int) -> bytes:
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def _track(events: List[Tuple[int, int, bytes]]) -> bytes:
    """events: (tick, order, payload); delta-encoded, End-of-Track appended."""
    events.sort(key=lambda e: (e[0], e[1]))
    data, last = bytearray(), 0
    for tick, _, payload in events:
        data += _vlq(tick - last) + payload
        last = tick
    data += b"\x00\xff\x2f\x00"
    return b"MTrk" + struct.pack(">I", len(data)) + bytes(data)


def _tempo_event(tick: int, microseconds: int) -> Tuple[int, int, bytes]:
    return (tick, 0, b"\xff\x51\x03" + struct.pack(">I", microseconds)[1:])


def _check_beats(beats) -> List[float]:
    b = [float(t) for t in beats]
    if len(b) < 2 or not all(math.isfinite(t) for t in b) or any(t1 <= t0 for t0, t1 in zip(b, b[1:])):
        raise ValueError("beats must be at least two finite, strictly ascending times")
    if any(not 1 <= int(round(1e6 * (t1 - t0))) < 1 << 24 for t0, t1 in zip(b, b[1:])):
        raise ValueError("a beat interval must be 1 us .. 16.7 s: the tempo field has 24 bits")
    return b


def preroll(beats, harmony=None) -> Tuple[int, float]:
    """(m, t0) of a tempo map written from `beats`: the whole beats inserted before the first one, and the time of tick 0,
    b[0] - m * (b[1] - b[0]) <= 0.  With a `harmony` that has a meter, m is the smallest such number that also puts a
    downbeat on tick 0: (m + harmony.downbeat) % harmony.beats_per_bar == 0"""
    b = _check_beats(beats)
    m = max(int(math.ceil(b[0] / (b[1] - b[0]))), 0)
    while b[0] - m * (b[1] - b[0]) > 0:                      # (the quotient was rounded down across a whole number)
        m += 1
    if harmony is not None and harmony.beats_per_bar:
        m += -(m + harmony.downbeat) % harmony.beats_per_bar
    return m, b[0] - m * (b[1] - b[0])


def _harmony_events(harmony, n_beats: int, m: int, res: int) -> List[Tuple[int, int, bytes]]:
    """the key signature, the time signature (both before the tempo at tick 0) and the chord markers of one `Harmony`"""
    if len(harmony.chords) != n_beats:
        raise ValueError("harmony has %d chords for %d beats" % (len(harmony.chords), n_beats))
    from .harmony import chord_name
    events = []
    if harmony.key >= 0:
        events.append((0, -2, b"\xff\x59\x02" + struct.pack(">bB", harmony.sharps, harmony.key % 2)))
    if harmony.beats_per_bar:
        events.append((0, -1, b"\xff\x58\x04" + bytes([harmony.beats_per_bar, 2, 24, 8])))
    for i, state in enumerate(harmony.chords):
        if i == 0 or state != harmony.chords[i - 1]:
            name = chord_name(state, harmony.key).encode("ascii") if state else b"N.C."
            events.append(((m + i) * res, 1, b"\xff\x06" + _vlq(len(name)) + name))
    return events


def note_sequence_to_midi_bytes(ns: NoteSequence, qpm: float = DEFAULT_QPM, beats: Optional[Sequence[float]] = None,
                                harmony=None) -> bytes:
    res = ns.ticks_per_quarter or 220
    if harmony is not None and beats is None:
        raise ValueError("harmony= needs the beats it was found on: pass beats= too")
    if beats is None:
        to_tick = lambda t: int(round(t * res * qpm / 60.0))  # noqa: E731
        tempo = int(round(60_000_000 / qpm))
        tracks = [_track([_tempo_event(0, tempo)])]
    else:
        b = _check_beats(beats)
        m = preroll(b, harmony)[0]

        def to_tick(t):
            i = min(max(bisect.bisect_right(b, t) - 1, 0), len(b) - 2)
            return max(int(round((m + i + (t - b[i]) / (b[i + 1] - b[i])) * res)), 0)

        conductor = [_tempo_event((m + i) * res, int(round(1e6 * (b[i + 1] - b[i])))) for i in range(len(b) - 1)]
        if m:
            conductor.append(_tempo_event(0, int(round(1e6 * (b[1] - b[0])))))
        if harmony is not None:
            conductor += _harmony_events(harmony, len(b), m, res)
        tracks = [_track(conductor)]
    groups: Dict[Tuple[int, int, bool], List[Note]] = {}
    for n in ns.notes:
        groups.setdefault((n.instrument, n.program, bool(n.is_drum)), []).append(n)
    controls: Dict[int, List[ControlChange]] = {}
    for cc in ns.control_changes:
        controls.setdefault(cc.instrument, []).append(cc)
    for inst in sorted(controls):                            # a pedal without notes: a track of its own, no notes in it
        if not any(key[0] == inst for key in groups):
            groups[(inst, 0, inst == 9)] = []
    free = [c for c in range(16) if c != 9]
    for i, ((inst, program, drum), notes) in enumerate(sorted(groups.items())):
        ch = 9 if drum else free[i % len(free)]
        ev = [(0, 0, bytes([0xC0 | ch, program & 0x7F]))]
        for cc in controls.pop(inst, []):                    # with the instrument's first track; before notes at a tick
            ev.append((to_tick(cc.time), 0, bytes([0xB0 | ch, cc.control_number & 0x7F, cc.control_value & 0x7F])))
        for n in notes:
            on, off = to_tick(n.start_time), max(to_tick(n.end_time), to_tick(n.start_time) + 1)
            ev.append((on, 2, bytes([0x90 | ch, n.pitch & 0x7F, max(1, n.velocity) & 0x7F])))
            ev.append((off, 1, bytes([0x80 | ch, n.pitch & 0x7F, 0])))          # offs before ons at a tick
        tracks.append(_track(ev))
    header = b"MThd" + struct.pack(">IHHH", 6, 1, len(tracks), res)
    return header + b"".join(tracks)


def note_sequence_to_midi_file(ns: NoteSequence, path: str, qpm: float = DEFAULT_QPM,
                               beats: Optional[Sequence[float]] = None, harmony=None) -> None:
    with open(path, "wb") as f:
        f.write(note_sequence_to_midi_bytes(ns, qpm, beats, harmony))


sequence_proto_to_midi_file = note_sequence_to_midi_file       # note_seq's name for it


class _TempoMap:
    """ticks -> seconds through a file's set-tempo events; 500000 us per quarter until the first one"""

    def __init__(self, events: List[Tuple[int, int]], res: int):
        self.res, self.ticks, self.tempos, self.seconds = res, [0], [500000], [0.0]
        for tick, tempo in sorted(events, key=lambda e: e[0]):       # stable: on equal ticks the last one read holds
            if tick == self.ticks[-1]:
                self.tempos[-1] = tempo
            else:
                self.seconds.append(self(tick))
                self.ticks.append(tick)
                self.tempos.append(tempo)

    def __call__(self, tick: int) -> float:
        k = bisect.bisect_right(self.ticks, tick) - 1
        return self.seconds[k] + (tick - self.ticks[k]) * self.tempos[k] / 1e6 / self.res


def _parse(data: bytes, metas: Optional[list] = None):
    """-> (resolution, notes, controllers, tempo events, the last event's tick), everything in ticks; every key-signature,
    time-signature and marker event is also appended to `metas` as (tick, kind, payload)"""
    assert data[:4] == b"MThd"
    _, fmt, ntrk, res = struct.unpack(">IHHH", data[4:14])
    pos, tempos, last_tick = 14, [], 0
    raw, raw_cc = [], []
    for _ in range(ntrk):
        assert data[pos:pos + 4] == b"MTrk"
        ln = struct.unpack(">I", data[pos + 4:pos + 8])[0]
        body, pos = data[pos + 8:pos + 8 + ln], pos + 8 + ln
        i, tick, status, program, open_notes = 0, 0, 0, {}, {}
        while i < len(body):
            d = 0
            while True:
                b = body[i]
                i += 1
                d = (d << 7) | (b & 0x7F)
                if not b & 0x80:
                    break
            tick += d
            if body[i] & 0x80:
                status = body[i]
                i += 1
            if status == 0xFF:
                kind, ln2 = body[i], body[i + 1]
                if kind == 0x51:
                    tempos.append((tick, int.from_bytes(body[i + 2:i + 5], "big")))
                if kind in (0x59, 0x58, 0x06) and metas is not None:
                    metas.append((tick, kind, bytes(body[i + 2:i + 2 + ln2])))
                if kind != 0x2F:
                    last_tick = max(last_tick, tick)
                i += 2 + ln2
                continue
            if status in (0xF0, 0xF7):                       # SysEx: a VLQ length, then that many bytes
                ln2 = 0
                while True:
                    b = body[i]
                    i += 1
                    ln2 = (ln2 << 7) | (b & 0x7F)
                    if not b & 0x80:
                        break
                i += ln2
                continue
            hi, ch = status & 0xF0, status & 0x0F
            last_tick = max(last_tick, tick)
            if hi == 0xC0:
                program[ch] = body[i]
                i += 1
            elif hi in (0x80, 0x90):
                pitch, vel = body[i], body[i + 1]
                i += 2
                if hi == 0x90 and vel > 0:
                    open_notes.setdefault((ch, pitch), []).append((tick, vel))
                elif open_notes.get((ch, pitch)):
                    t0, v0 = open_notes[(ch, pitch)].pop(0)
                    raw.append((t0, tick, pitch, v0, program.get(ch, 0), ch == 9))
            elif hi == 0xB0:
                raw_cc.append((tick, body[i], body[i + 1], 9 if ch == 9 else 0))
                i += 2
            else:
                i += 2 if hi not in (0xD0,) else 1
    return res, raw, raw_cc, tempos, last_tick


def midi_bytes_to_note_sequence(data: bytes) -> NoteSequence:
    """Minimal SMF reader (note on/off, program change, controllers, the tempo map; SysEx skipped) -- enough to round-trip
    the writer and to read a piano file's pedal.  control_changes come in (tick, file) order."""
    res, raw, raw_cc, tempos, _ = _parse(data)
    sec = _TempoMap(tempos, res)
    ns = NoteSequence(ticks_per_quarter=res)
    for t0, t1, pitch, vel, prog, drum in sorted(raw):
        ns.notes.append(Note(sec(t0), sec(t1), pitch, vel, prog, drum, 9 if drum else 0))
        ns.total_time = max(ns.total_time, sec(t1))
    for tick, number, value, inst in sorted(raw_cc, key=lambda c: c[0]):
        ns.control_changes.append(ControlChange(sec(tick), number, value, inst))
    return ns


def midi_bytes_to_beats(data: bytes) -> List[float]:
    """The times in seconds of a file's quarter-note ticks, 0, resolution, 2 * resolution, ..., up to its last event (the
    End-of-Track events apart): the beats of a file written with `beats=`, the inserted ones (`preroll`) included."""
    res, _, _, tempos, last_tick = _parse(data)
    sec = _TempoMap(tempos, res)
    return [sec(tick) for tick in range(0, last_tick + 1, res)]


def midi_bytes_to_signatures(data: bytes) -> Dict[str, list]:
    """The key signatures, time signatures and markers of a file, each in file order with its time in seconds through the
    tempo map: {"key_signatures": [(time, sharps, mode)], "time_signatures": [(time, numerator, denominator)],
    "markers": [(time, text)]}.  sharps is -7 .. 7, mode 0 major / 1 minor; the denominator is the note value (4: quarters).
    Events shorter than their kind's payload are skipped."""
    metas: list = []
    res, _, _, tempos, _ = _parse(data, metas)
    sec = _TempoMap(tempos, res)
    out: Dict[str, list] = {"key_signatures": [], "time_signatures": [], "markers": []}
    for tick, kind, payload in metas:
        if kind == 0x59 and len(payload) >= 2:
            out["key_signatures"].append((sec(tick), struct.unpack(">b", payload[:1])[0], payload[1]))
        elif kind == 0x58 and len(payload) >= 2:
            out["time_signatures"].append((sec(tick), payload[0], 1 << payload[1]))
        elif kind == 0x06:
            out["markers"].append((sec(tick), payload.decode("latin-1")))
    return out
