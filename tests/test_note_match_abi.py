"""mt3_op_match_notes on a box without a GPU: the symbols and their prototypes, and every argument check of
include/mt3_hip.h -- all of which come before any HIP call, so the "device" pointers here are host memory that must come
back untouched.  No CUDA call in this file."""
import ctypes as C
import inspect

import numpy as np
import pytest

from mt3_amd import _lib, metrics, note_matching, transcribe

NAN, INF = float("nan"), float("inf")


def test_symbols_are_exported_and_typed():
    lib = _lib.load()
    _P = C.c_void_p
    assert _lib.SIGNATURES["mt3_op_match_notes"] == (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P,
                                                               C.c_int64, C.c_int32, _P, _P])
    assert _lib.SIGNATURES["mt3_note_match_state_words"] == (C.c_int64, [C.c_int32, C.c_int32])
    for name in ("mt3_op_match_notes", "mt3_note_match_state_words"):
        fn = getattr(lib, name)
        assert fn.restype is _lib.SIGNATURES[name][0] and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4
    assert C.sizeof(_lib.MatchRule) == 40 == note_matching.RULE_DTYPE.itemsize
    assert C.sizeof(_lib.MatchProblem) == 40 == note_matching.PROBLEM_DTYPE.itemsize
    for struct, dtype in ((_lib.MatchRule, note_matching.RULE_DTYPE), (_lib.MatchProblem, note_matching.PROBLEM_DTYPE)):
        assert [(n, getattr(struct, n).offset) for n, _ in struct._fields_] == [(n, dtype.fields[n][1]) for n in dtype.names]
    assert (_lib.NOTE_MATCH_MAX_RULES, _lib.NOTE_MATCH_NO_OFFSET) == (16, -1.0)


def test_state_words():
    lib = _lib.load()
    assert lib.mt3_note_match_state_words(0, 0) == 0
    assert lib.mt3_note_match_state_words(3, 5) == 6 * 3 + 2 * 5 == note_matching.REF_WORDS * 3 + note_matching.EST_WORDS * 5
    assert lib.mt3_note_match_state_words(2 ** 31 - 1, 2 ** 31 - 1) == 8 * (2 ** 31 - 1)
    assert lib.mt3_note_match_state_words(-1, 5) == -1 and lib.mt3_note_match_state_words(5, -1) == -1


def _problems(*rows):
    t = np.zeros(len(rows), note_matching.PROBLEM_DTYPE)
    for i, row in enumerate(rows):
        t[i] = row + (0,)
    return t


def _rules(*rows):
    t = np.zeros(len(rows), note_matching.RULE_DTYPE)
    for i, row in enumerate(rows):
        t[i] = row + (0,)
    return t


class _Job:
    """a well-formed two-problem call on host memory; `call(name=value)` swaps one argument"""

    def __init__(self):
        self.notes = np.zeros(64, np.float64)
        self.work = np.full(128, 7, np.int32)
        self.matched = np.full(2, 99, np.int32)
        p = self.notes.ctypes.data
        # problem 0: refs [0, 3), estimates [3, 7), 6 * 3 + 2 * 4 = 26 words; problem 1 shares the estimates
        self.args = dict(d_onset=p, d_offset=p, d_log2=p, n_notes=10,
                         problems=_problems((0, 3, 0, 3, 4, 0), (7, 3, 26, 3, 4, 1)), n_problems=2,
                         rules=_rules((0.05, 50.0, 0.2, 0.05, 0), (0.05, 50.0, -1.0, 0.05, 1)), n_rules=2,
                         d_workspace=self.work.ctypes.data, workspace_words=52, warm_start=0,
                         d_matched=self.matched.ctypes.data, stream=None)

    def call(self, **swap):
        a = dict(self.args, **swap)
        self.keep = a
        tab = lambda v: None if v is None else v.ctypes.data        # noqa: E731
        return _lib.load().mt3_op_match_notes(a["d_onset"], a["d_offset"], a["d_log2"], a["n_notes"], a["n_problems"],
                                              tab(a["problems"]), a["n_rules"], tab(a["rules"]), a["d_workspace"],
                                              a["workspace_words"], a["warm_start"], a["d_matched"], a["stream"])

    def untouched(self):
        return (self.work == 7).all() and (self.matched == 99).all() and not self.notes.any()


def test_match_notes_rejects_bad_arguments_before_any_device_call():
    lib, job = _lib.load(), _Job()
    good_rule = (0.05, 50.0, 0.2, 0.05, 0)
    bad = [
        (dict(n_problems=-1), b"n_problems"),
        (dict(n_notes=-1), b"n_notes"),
        (dict(n_rules=-1), b"n_rules"), (dict(n_rules=17), b"n_rules"),
        (dict(workspace_words=-1), b"workspace_words"),
        (dict(rules=None), b"null rule table"),
        (dict(problems=None), b"null problem table"),
        (dict(d_matched=None), b"null d_matched"),
        (dict(d_onset=None), b"null note array"), (dict(d_offset=None), b"null note array"),
        (dict(d_log2=None), b"null note array"),
        (dict(d_workspace=None), b"null d_workspace"),
        (dict(problems=_problems((0, 3, 0, -3, 4, 0), (7, 3, 26, 3, 4, 1))), b"negative note count"),
        (dict(problems=_problems((0, 3, 0, 3, -4, 0), (7, 3, 26, 3, 4, 1))), b"negative note count"),
        (dict(problems=_problems((-1, 3, 0, 3, 4, 0), (7, 3, 26, 3, 4, 1))), b"inside [0, n_notes]"),
        (dict(problems=_problems((8, 3, 0, 3, 4, 0), (7, 3, 26, 3, 4, 1))), b"inside [0, n_notes]"),      # refs end at 11
        (dict(problems=_problems((0, 7, 0, 3, 4, 0), (7, 3, 26, 3, 4, 1))), b"inside [0, n_notes]"),      # estimates end at 11
        (dict(problems=_problems((0, -2, 0, 3, 4, 0), (7, 3, 26, 3, 4, 1))), b"inside [0, n_notes]"),
        (dict(problems=_problems((2 ** 62, 3, 0, 3, 4, 0), (7, 3, 26, 3, 4, 1))), b"inside [0, n_notes]"),
        (dict(problems=_problems((0, 3, 0, 3, 4, 2), (7, 3, 26, 3, 4, 1))), b"rule index"),
        (dict(problems=_problems((0, 3, 0, 3, 4, -1), (7, 3, 26, 3, 4, 1))), b"rule index"),
        (dict(n_rules=1), b"rule index"),                                       # problem 1 names rule 1
        (dict(problems=_problems((0, 3, 0, 3, 4, 0), (7, 3, 25, 3, 4, 1))), b"overlap"),                  # one word inside problem 0
        (dict(problems=_problems((0, 3, 26, 3, 4, 0), (7, 3, 0, 3, 4, 1))), b"overlap"),                  # out of order
        (dict(problems=_problems((0, 3, -1, 3, 4, 0), (7, 3, 26, 3, 4, 1))), b"overlap"),
        (dict(workspace_words=51), b"past workspace_words"),                    # one word short
        (dict(problems=_problems((0, 3, 0, 3, 4, 0), (7, 3, 2 ** 62, 3, 4, 1))), b"past workspace_words"),
    ]
    for field in range(4):                                                      # a tolerance that is negative or not finite
        for value in (-0.01, NAN, INF, -INF):
            rule = good_rule[:field] + (value,) + good_rule[field + 1:]
            bad.append((dict(rules=_rules(rule, good_rule)), b"offset_ratio" if field == 2 else b"tolerance"))
    bad.append((dict(rules=_rules(good_rule, good_rule[:2] + (-2.0,) + good_rule[3:])), b"offset_ratio"))
    for swap, word in bad:
        assert job.call(**swap) == _lib.MT3_ERR_INVALID, swap
        err = lib.mt3_last_error()
        assert err.startswith(b"mt3_op_match_notes: ") and word in err, (swap, err)
    assert job.untouched()                                  # host memory: nothing may have touched it


def test_calls_with_zero_problems_succeed():
    job = _Job()
    assert job.call(n_problems=0) == _lib.MT3_OK
    assert job.call(n_problems=0, problems=None, n_rules=0, rules=None, n_notes=0, d_onset=None, d_offset=None, d_log2=None,
                    d_workspace=None, workspace_words=0, d_matched=None) == _lib.MT3_OK
    assert job.untouched()


def test_packing_shares_notes_and_sorts_estimates_stably():
    ref = (np.array([[0.0, 1.0], [0.5, 1.5]]), np.array([60.0, 62.0]))
    est = (np.array([[0.5, 1.0], [0.0, 1.0], [0.5, 2.0]]), np.array([62.0, 60.0, 64.0]))
    P = note_matching.Problem
    packed = note_matching.pack([P(*ref, *est), P(*ref, *est, offset_ratio=None), P(*ref, *est, onset_tolerance=0.5),
                                 P(ref[0].copy(), ref[1], *est)])
    assert packed.notes.shape == (3, 2 + 3 + 2)             # the fourth problem's reference copy is packed again
    assert packed.problems["ref0"].tolist() == [0, 0, 0, 5] and packed.problems["est0"].tolist() == [2, 2, 2, 2]
    assert packed.problems["rule"].tolist() == [0, 1, 2, 0] and len(packed.rules) == 3
    assert packed.rules["offset_ratio"].tolist() == [0.2, -1.0, 0.2]
    assert packed.problems["state0"].tolist() == [0, 18, 36, 54] and packed.workspace_words == 72
    assert packed.est_order[0].tolist() == [1, 0, 2]        # equal onsets keep the caller's order
    assert packed.notes[0].tolist() == [0.0, 0.5, 0.0, 0.5, 0.5, 0.0, 0.5]
    assert (packed.notes[2] == np.log2([60.0, 62.0, 60.0, 62.0, 64.0, 60.0, 62.0])).all()
    image = note_matching.warm_words(packed, [np.array([1, 0]), None, np.array([7, -1]), np.array([-1, 2])])
    assert image[0:2].tolist() == [0, 1] and image[18:20].tolist() == [-1, -1]
    assert image[36:38].tolist() == [7, -1] and image[54:56].tolist() == [-1, 2]


def test_python_surface():
    assert list(inspect.signature(note_matching.match).parameters)[:2] == ["problems", "warm_start"]
    assert list(inspect.signature(metrics.transcription_scores_many).parameters) == ["pairs", "pitch_unit"]
    assert list(inspect.signature(metrics.program_aware_note_scores_many).parameters) == ["pairs", "granularity_type"]
    sweep = inspect.signature(metrics.note_onset_tolerance_sweep_many).parameters
    assert list(sweep) == ["pairs", "tolerances"] and sweep["tolerances"].default == (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)
    tm = inspect.signature(metrics.transcription_metrics).parameters
    assert list(tm) == ["pairs", "track_specs", "frame_fps", "frame_velocity_threshold"]
    assert (tm["track_specs"].default, tm["frame_fps"].default, tm["frame_velocity_threshold"].default) == (None, 62.5, 30)
    assert callable(metrics.matched_notes)
    # jobs that need no matching make no device call: nothing, or only empty sides
    from mt3_amd.note_sequences import Note, NoteSequence
    assert metrics.transcription_scores_many([]) == [] and metrics.program_aware_note_scores_many([]) == []
    empty, some = NoteSequence(), NoteSequence(notes=[Note(0.0, 1.0, 60, 100), Note(1.0, 1.0, 62, 100)])
    for pair in ((empty, some), (some, empty)):
        assert metrics.transcription_scores_many([pair]) == [metrics.transcription_scores(*pair)]
        assert metrics.program_aware_note_scores_many([pair]) == [metrics.program_aware_note_scores(*pair)]
        assert set(metrics.note_onset_tolerance_sweep_many([pair])[0].values()) == {0.0}
        assert metrics.matched_notes(*pair).shape == (0, 2)


def test_command_line_flag(tmp_path):
    wav = tmp_path / "tune.wav"
    wav.write_bytes(b"")                                   # plan() only checks that the files exist
    refs = tmp_path / "refs"
    refs.mkdir()
    (refs / "tune.mid").write_bytes(b"")
    assert transcribe.plan(["--checkpoint", "random:0", str(wav)])[0].score_against is None
    args, outputs = transcribe.plan(["--checkpoint", "random:0", "--score-against", str(refs), "-o", str(tmp_path / "out.mid"),
                                     str(wav)])
    assert outputs == [str(tmp_path / "out.mid")]
    assert args.score_against == str(refs)
    assert transcribe.reference_path(str(refs), str(wav)) == str(refs / "tune.mid")
    assert transcribe.scores_path(["/x/y/a.mid", "/x/y/b.mid"]) == "/x/y/scores.json"
    with pytest.raises(SystemExit):                        # a reference that is not there is refused before anything loads
        transcribe.plan(["--checkpoint", "random:0", "--score-against", str(tmp_path), str(wav)])
    other = tmp_path / "elsewhere"
    other.mkdir()
    (other / "song.wav").write_bytes(b"")
    (refs / "song.mid").write_bytes(b"")
    with pytest.raises(SystemExit):                        # two output directories: no single place for scores.json
        transcribe.plan(["--checkpoint", "random:0", "--score-against", str(refs), str(wav), str(other / "song.wav")])
    _, outputs = transcribe.plan(["--checkpoint", "random:0", "--score-against", str(refs), "-o", str(tmp_path / "out"),
                                  str(wav), str(other / "song.wav")])
    assert transcribe.scores_path(outputs) == str(tmp_path / "out" / "scores.json")
