"""mt3_notes_decode_traced (csrc/symbolic.cpp) and metrics_utils.event_predictions_to_ns_traced: the notes of
mt3_notes_decode, and for every note the token that started it and the token that ended it.  CPU-only."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mt3_amd import _lib, event_codec as EC, metrics_utils as MU, note_sequences as NS, vocabularies as V
from tests import symbolic_cases as K

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "symbolic_golden.json")))
SPEC = {"onsets": NS.NoteOnsetEncodingSpec, "notes": NS.NoteEncodingSpec, "ties": NS.NoteEncodingWithTiesSpec}


def _codec(ranges, max_shift=100, sps=100):
    return EC.Codec(max_shift, sps, [EC.EventRange(*r) for r in ranges])


def _fields(ns):
    return [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, n.instrument) for n in ns.notes]


def _both(codec, spec, tokens_list, starts, max_times=None):
    """the plain and the traced decode of the same segments; asserts that they return the same notes, counts and time"""
    ns0, inv0, drop0 = MU._run(codec, spec.spec_id, tokens_list, starts, max_times)
    ns1, inv1, drop1, tr = MU._run_full(codec, spec.spec_id, tokens_list, starts, max_times, True)
    assert _fields(ns1) == _fields(ns0) and (inv1, drop1) == (inv0, drop0) and ns1.total_time == ns0.total_time
    return ns1, tr


def _check_links(codec, tokens_list, ns, tr, starts=None):
    """[0] is a PITCH / DRUM token of the note's pitch; [1], where there is one, a PITCH token of that pitch or a TIE.
    With the segments' start times (combiner rule: a segment is cut at the next one's start): the end token does not
    come before the onset token, and a TIE that ends a note sits in the segment in which the note's end_time falls --
    a tie section closes at its segment's start."""
    assert tr.dtype == np.int64 and tr.shape == (len(ns.notes), 2, 2)
    rank = None if starts is None else {s: k for k, s in enumerate(sorted(range(len(starts)), key=lambda i: starts[i]))}
    for n, ((s0, p0), (s1, p1)) in zip(ns.notes, tr.tolist()):
        if rank is not None and s1 >= 0:
            assert (rank[s1], p1) > (rank[s0], p0)
            if codec.decode_event_index(int(tokens_list[s1][p1])).type == "tie":
                later = [starts[i] for i in range(len(starts)) if rank[i] > rank[s1]]
                assert starts[s1] <= n.end_time and (not later or n.end_time <= min(later))
        ev = codec.decode_event_index(int(tokens_list[s0][p0]))
        assert ev.type in ("pitch", "drum") and ev.value == n.pitch and (ev.type == "drum") == bool(n.is_drum)
        if s1 < 0:
            assert (s1, p1) == (-1, -1)
            continue
        ev = codec.decode_event_index(int(tokens_list[s1][p1]))
        assert (ev.type == "pitch" and ev.value == n.pitch) or ev.type == "tie"
        assert not n.is_drum


@pytest.mark.parametrize("case", K.SINGLE, ids=lambda c: c["name"])
def test_single_segment_cases(case):
    codec = _codec(case["ranges"])
    ns, tr = _both(codec, SPEC[case["mode"]], [case["tokens"]], [case["start"]], [case["max_time"]])
    assert len(ns.notes) == len(case["notes"])
    _check_links(codec, [case["tokens"]], ns, tr)


@pytest.mark.parametrize("case", K.COMBINE, ids=lambda c: c["name"])
def test_combiner_cases(case):
    codec = _codec(case["ranges"])
    toks, starts = [t for _, t in case["segments"]], [s for s, _ in case["segments"]]
    ns, tr = _both(codec, SPEC[case["mode"]], toks, starts)
    assert len(ns.notes) == len(case["notes"])
    _check_links(codec, toks, ns, tr, starts)


@pytest.mark.parametrize("i", range(len(GOLD["decode_cases"])))
def test_golden_cases(i):
    c = GOLD["decode_cases"][i]
    codec = V.build_codec(V.VocabularyConfig(num_velocity_bins=c["num_velocity_bins"]))
    toks, starts = [s["tokens"] for s in c["segments"]], [s["start_time"] for s in c["segments"]]
    ns, tr = _both(codec, SPEC[c["mode"]], toks, starts)
    assert [list(f) for f in _fields(ns)] == c["notes"]
    _check_links(codec, toks, ns, tr, starts)


# ---- hand-written cases on the MT3 codec, every index spelled out
MT3 = V.build_codec(V.VocabularyConfig(num_velocity_bins=1))


def _t(*events):
    """("shift", 10) / ("pitch", 60) / ... -> token indices of the MT3 codec"""
    return [MT3.encode_event(EC.Event(t, v)) for t, v in events]


TIE, ON, OFF = ("tie", 0), ("velocity", 1), ("velocity", 0)
NONE = [-1, -1]

HAND = [
    dict(name="tied_across_two_segments", mode="ties",
         segments=[(0.0, _t(TIE, ("shift", 10), ON, ("pitch", 60))),
                   (2.0, _t(("pitch", 60), TIE, ("shift", 50), OFF, ("pitch", 60)))],
         notes=[(0.1, 2.5, 60)], trace=[[[0, 3], [1, 4]]]),
    dict(name="untied_note_ended_by_the_tie_token", mode="ties",
         segments=[(0.0, _t(TIE, ("shift", 10), ON, ("pitch", 60), ("pitch", 64))),
                   (2.0, _t(("pitch", 64), TIE, ("shift", 20), OFF, ("pitch", 64)))],
         notes=[(0.1, 2.0, 60), (0.1, 2.2, 64)], trace=[[[0, 3], [1, 1]], [[0, 4], [1, 4]]]),
    dict(name="reonset_then_flushed_at_the_end", mode="ties",
         segments=[(0.0, _t(TIE, ON, ("pitch", 60), ("shift", 30), ("pitch", 60), ("shift", 60)))],
         notes=[(0.0, 0.3, 60), (0.3, 0.31, 60)], trace=[[[0, 2], [0, 4]], [[0, 4], NONE]]),
    dict(name="drum_hit", mode="ties",
         segments=[(0.0, _t(TIE, ("shift", 7), ON, ("drum", 36)))],
         notes=[(0.07, 0.08, 36)], trace=[[[0, 3], NONE]]),
    dict(name="onsets_only_spec", mode="onsets",
         segments=[(0.0, _t(("shift", 5), ("pitch", 60), ("shift", 10), ("pitch", 62)))],
         notes=[(0.05, 0.06, 60), (0.10, 0.11, 62)], trace=[[[0, 1], NONE], [[0, 3], NONE]]),
    dict(name="flushed_note_of_an_earlier_segment", mode="ties",
         segments=[(0.0, _t(TIE, ON, ("pitch", 72))), (2.0, _t(("pitch", 72), TIE, ("shift", 5)))],
         notes=[(0.0, 2.0, 72)], trace=[[[0, 2], NONE]]),
    # predictions handed over out of order: the indices are into the caller's list, not the sorted one
    dict(name="segments_in_reverse_order", mode="ties",
         segments=[(2.0, _t(("pitch", 60), TIE, ("shift", 50), OFF, ("pitch", 60))),
                   (0.0, _t(TIE, ("shift", 10), ON, ("pitch", 60)))],
         notes=[(0.1, 2.5, 60)], trace=[[[1, 3], [0, 4]]]),
    # an empty segment in between: positions stay relative to each segment's own row
    dict(name="empty_segment_between", mode="ties",
         segments=[(0.0, _t(TIE, ON, ("pitch", 50))), (2.0, []), (4.0, _t(("pitch", 50), TIE, OFF, ("pitch", 50)))],
         notes=[(0.0, 4.0, 50)], trace=[[[0, 2], [2, 3]]]),
]


@pytest.mark.parametrize("case", HAND, ids=lambda c: c["name"])
def test_hand_written_indices(case):
    preds = [{"start_time": st, "est_tokens": np.array(toks, np.int32)} for st, toks in case["segments"]]
    res = MU.event_predictions_to_ns_traced(preds, MT3, SPEC[case["mode"]])
    plain = MU.event_predictions_to_ns(preds, MT3, SPEC[case["mode"]])
    assert _fields(res["est_ns"]) == _fields(plain["est_ns"]) and res["est_ns"].total_time == plain["est_ns"].total_time
    assert {k: res[k] for k in ("est_invalid_events", "est_dropped_events", "start_times")} == \
        {k: plain[k] for k in ("est_invalid_events", "est_dropped_events", "start_times")}
    got = [(n.start_time, n.end_time, n.pitch) for n in res["est_ns"].notes]
    assert len(got) == len(case["notes"])
    for g, e in zip(got, case["notes"]):
        assert g[2] == e[2] and abs(g[0] - e[0]) < 1e-12 and abs(g[1] - e[1]) < 1e-12
    assert res["note_tokens"].dtype == np.int64
    assert res["note_tokens"].tolist() == case["trace"]
    _check_links(MT3, [t for _, t in case["segments"]], res["est_ns"], res["note_tokens"], [s for s, _ in case["segments"]])


def test_empty_inputs_and_null_trace():
    res = MU.event_predictions_to_ns_traced([], MT3, NS.NoteEncodingWithTiesSpec)
    assert res["est_ns"].notes == [] and res["note_tokens"].shape == (0, 2, 2)
    res = MU.event_predictions_to_ns_traced([{"est_tokens": np.zeros(0, np.int32), "start_time": 0.0}], MT3,
                                            NS.NoteEncodingWithTiesSpec)
    assert res["est_ns"].notes == [] and res["note_tokens"].shape == (0, 2, 2)


def test_symbol_is_exported_and_typed_and_a_null_trace_is_the_plain_decode():
    lib = _lib.load()
    assert "mt3_notes_decode_traced" in _lib.SIGNATURES and hasattr(lib, "mt3_notes_decode_traced")
    assert lib.mt3_notes_decode_traced.argtypes == _lib.SIGNATURES["mt3_notes_decode_traced"][1]
    assert lib.mt3_abi_version() == 4
    case = HAND[1]
    toks = np.concatenate([np.array(t, np.int32) for _, t in case["segments"]])
    offs = np.cumsum([0] + [len(t) for _, t in case["segments"]]).astype(np.int64)
    st = np.array([s for s, _ in case["segments"]], np.float64)
    out = []
    for traced in (False, True):
        notes = np.zeros(8, MU.NOTE_DTYPE)
        n, inv, drop, total = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        args = (C.byref(MT3.desc), _lib.SPEC_TIES, 2, toks.ctypes.data, offs.ctypes.data, st.ctypes.data, None, None,
                C.c_void_p(notes.ctypes.data), 8, C.byref(n), C.byref(inv), C.byref(drop), C.byref(total))
        _lib.check(lib.mt3_notes_decode_traced(*args, None) if traced else lib.mt3_notes_decode(*args))
        out.append((notes[: n.value].tobytes(), n.value, inv.value, drop.value, total.value))
    assert out[0] == out[1] and out[0][1] == 2
    # a malformed call is refused as mt3_notes_decode refuses it, under the traced entry point's own name
    n = C.c_int64()
    assert lib.mt3_notes_decode_traced(None, _lib.SPEC_TIES, 0, None, None, None, None, None, None, 0, C.byref(n), None, None,
                                       None, None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_notes_decode_traced: ")


def test_traced_decode_under_address_and_ub_sanitizers(tmp_path):
    """tests/host/note_trace_fuzz.cpp, a program of its own linked with the host sources under test"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "mt3_amd", "csrc")
    exe = str(tmp_path / "note_trace_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(root, "include"), "-I", csrc,
                           os.path.join(root, "tests", "host", "note_trace_fuzz.cpp"), os.path.join(csrc, "symbolic.cpp"),
                           os.path.join(csrc, "errors.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
