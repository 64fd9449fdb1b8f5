"""mt3_op_note_levels and mt3_op_level_velocities on a box without a GPU: exported and typed, declared in the header with
matching arity, their constants and file record mirrored, every argument error comes back as MT3_ERR_INVALID -- before any
device work -- with a text that starts with the function's name and names the reason; and the Python surface and the
command line's flags."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from mt3_amd import _lib, velocity
from tests import velocity_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS, VELOCITIES = "mt3_op_note_levels", "mt3_op_level_velocities"


def test_the_symbols_are_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mt3_hip.h")).read()
    for name, arity in ((LEVELS, 16), (VELOCITIES, 11)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == arity
    for name, value in (("KEYS", 129), ("THRESHOLDS", 126), ("MAX_WINDOW", 64), ("MAX_MEL", 4096)):
        assert getattr(_lib, "VELOCITY_" + name) == value and "#define MT3_VELOCITY_%s %d" % (name, value) in header
    assert C.sizeof(_lib.VelocityFile) == velocity.FILE_DTYPE.itemsize == 32
    assert [n for n, _ in _lib.VelocityFile._fields_] == list(velocity.FILE_DTYPE.names)
    assert [getattr(_lib.VelocityFile, n).offset for n in velocity.FILE_DTYPE.names] == \
        [velocity.FILE_DTYPE.fields[n][1] for n in velocity.FILE_DTYPE.names]
    assert lib.mt3_abi_version() == 4                                  # additive entry points
    assert "velocity.hip" in __import__("mt3_amd.build", fromlist=["x"]).HIP_SOURCES


POINTERS = ("logmel", "frame", "key", "h_bin_first", "h_bins", "d_bin_first", "d_bins", "level", "th", "velocity_in",
            "velocity", "anchor", "measured")


def _buffers(null, table):
    """host arrays standing in for the device arrays: none is touched before the arguments are refused"""
    assert set(null) <= set(POINTERS)
    buf = {n: None if null.get(n) else (C.c_double * 512)() for n in POINTERS}
    for name, a in zip(("h_bin_first", "h_bins"), table):
        if buf[name] is not None:
            C.memmove(buf[name], a.ctypes.data, a.nbytes)
    return lambda n: None if buf[n] is None else C.cast(buf[n], C.c_void_p)


def _levels(lib, n_rows=32, n_mel=4, files=((0, 0, 8, 5, 32),), n_files=None, n_notes=8, window=8, n_bins=None, table=None,
            **null):
    table = cases.hand_table() if table is None else table
    p = _buffers(null, table)
    records = None if files is None else cases.files(*files)
    return getattr(lib, LEVELS)(
        p("logmel"), n_rows, n_mel, None if records is None else records.ctypes.data,
        len(files) if n_files is None else n_files, p("frame"), p("key"), n_notes, p("h_bin_first"), p("h_bins"),
        p("d_bin_first"), p("d_bins"), len(table[1]) if n_bins is None else n_bins, window, p("level"), None)


def _velocities(lib, files=((0, 0, 8, 5, 32),), n_files=None, n_notes=8, quantile=0.5, **null):
    p = _buffers(null, cases.hand_table())
    records = None if files is None else cases.files(*files)
    return getattr(lib, VELOCITIES)(
        p("level"), n_notes, None if records is None else records.ctypes.data, len(files) if n_files is None else n_files,
        quantile, p("th"), p("velocity_in"), p("velocity"), p("anchor"), p("measured"), None)


def _bad_table(**change):
    first, bins = cases.hand_table()
    first, bins = first.copy(), bins.copy()
    for k, v in change.get("first", {}).items():
        first[k] = v
    for k, v in change.get("bins", {}).items():
        bins[k] = v
    return first, bins


FILE_ERRORS = [
    (dict(n_notes=-1), b"n_notes must not be negative"),
    (dict(n_files=-2), b"n_files must not be negative"),
    (dict(files=None, n_files=1), b"null file table"),
    (dict(files=((-1, 0, 2, 2, 32),)), b"note range must lie inside [0, n_notes]"),
    (dict(files=((0, 0, -2, 0, 32),)), b"note range must lie inside [0, n_notes]"),
    (dict(files=((0, 0, 9, 5, 32),)), b"note range must lie inside [0, n_notes]"),
    (dict(files=((9, 0, 0, 0, 32),)), b"note range must lie inside [0, n_notes]"),
    (dict(files=((4, 0, 5, 5, 32),)), b"note range must lie inside [0, n_notes]"),
    (dict(files=((0, 0, 5, 5, 16), (4, 16, 4, 4, 16))), b"note ranges overlap or are out of order"),
    (dict(files=((4, 0, 4, 4, 16), (0, 16, 4, 4, 16))), b"note ranges overlap or are out of order"),
    (dict(files=((0, 0, 8, 9, 32),)), b"n_pitched must lie in 0 .. n_notes"),
    (dict(files=((0, 0, 8, -1, 32),)), b"n_pitched must lie in 0 .. n_notes"),
]


def test_bad_level_calls_are_refused_before_any_device_work():
    lib = _lib.load()
    calls = FILE_ERRORS + [
        (dict(window=0), b"window must be 1 .. 64"),
        (dict(window=65), b"window must be 1 .. 64"),
        (dict(window=-8), b"window must be 1 .. 64"),
        (dict(n_mel=0), b"n_mel must be 1 .. 4096"),
        (dict(n_mel=4097), b"n_mel must be 1 .. 4096"),
        (dict(n_rows=-1), b"n_rows must not be negative"),
        (dict(n_bins=-1), b"n_bins must not be negative"),
        (dict(n_mel=3), b"a bin of the table is >= n_mel"),            # the hand table lists bin 3
        (dict(table=_bad_table(bins={4: 4})), b"a bin of the table is >= n_mel"),
        (dict(table=_bad_table(bins={0: -1})), b"a bin of the table is >= n_mel"),
        (dict(table=_bad_table(first={0: 1})), b"bin_first must rise from 0 to n_bins"),
        (dict(table=_bad_table(first={5: 3})), b"bin_first must rise from 0 to n_bins"),
        (dict(n_bins=9), b"bin_first must rise from 0 to n_bins"),
        (dict(files=((0, 0, 8, 5, 33),)), b"rows must lie inside the log-mel's [0, n_rows]"),
        (dict(files=((0, 30, 8, 5, 3),)), b"rows must lie inside the log-mel's [0, n_rows]"),
        (dict(files=((0, -1, 8, 5, 3),)), b"rows must lie inside the log-mel's [0, n_rows]"),
        (dict(files=((0, 0, 8, 5, -1),)), b"rows must lie inside the log-mel's [0, n_rows]"),
        (dict(files=((0, 33, 8, 5, 0),)), b"rows must lie inside the log-mel's [0, n_rows]"),
        (dict(files=((0, 0, 4, 4, 16), (4, 20, 4, 4, 13))), b"rows must lie inside the log-mel's [0, n_rows]"),
        (dict(logmel=True), b"null log-mel"),
        (dict(frame=True), b"null note column"),
        (dict(key=True), b"null note column"),
        (dict(level=True), b"null level"),
        (dict(h_bin_first=True), b"null bin_first"),
        (dict(d_bin_first=True), b"null bin_first"),
        (dict(h_bins=True), b"null bins"),
        (dict(d_bins=True), b"null bins"),
    ]
    for kw, what in calls:
        assert _levels(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(LEVELS.encode() + b": ") and what in msg, (kw, msg)


def test_bad_velocity_calls_are_refused_before_any_device_work():
    lib = _lib.load()
    calls = FILE_ERRORS + [
        (dict(quantile=-0.01), b"quantile must lie in [0, 1]"),
        (dict(quantile=1.01), b"quantile must lie in [0, 1]"),
        (dict(quantile=float("nan")), b"quantile must lie in [0, 1]"),
        (dict(level=True), b"null note column"),
        (dict(velocity_in=True), b"null note column"),
        (dict(velocity=True), b"null note column"),
        (dict(th=True), b"null thresholds"),
        (dict(anchor=True), b"null output"),
        (dict(measured=True), b"null output"),
    ]
    for kw, what in calls:
        assert _velocities(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(VELOCITIES.encode() + b": ") and what in msg, (kw, msg)


def test_no_files_is_ok_and_launches_nothing():
    lib = _lib.load()
    null = {name: True for name in POINTERS}
    assert _levels(lib, files=(), n_notes=0, **null) == _lib.MT3_OK
    assert _levels(lib, files=(), n_notes=8, n_rows=0, **null) == _lib.MT3_OK
    assert _velocities(lib, files=(), n_notes=0, **null) == _lib.MT3_OK
    assert _velocities(lib, files=(), n_notes=8, quantile=1.0, **null) == _lib.MT3_OK


class _NotATensor:
    is_cuda = False


def test_estimate_refuses_bad_arguments_before_anything_is_uploaded():
    from mt3_amd import note_sequences
    ns = note_sequences.NoteSequence(notes=[note_sequences.Note(0.0, 1.0, 60, 100)], total_time=1.0)
    with pytest.raises(ValueError, match="logmels has 1 entries for 2 sequences"):
        velocity.estimate([_NotATensor()], [ns, ns])
    for kw, what in ((dict(window=0), "window must be 1 .. 64"), (dict(window=65), "window must be 1 .. 64"),
                     (dict(window=2.5), "window must be 1 .. 64"), (dict(quantile=1.5), r"quantile must lie in \[0, 1\]"),
                     (dict(quantile=float("nan")), r"quantile must lie in \[0, 1\]"), (dict(gamma=0.0), "gamma must be"),
                     (dict(anchor_velocity=-1), "anchor_velocity must be"),
                     (dict(frames_per_second=0), "frames_per_second must be")):
        with pytest.raises(ValueError, match=what):
            velocity.estimate([_NotATensor()], [ns], **kw)
    pytest.importorskip("torch")
    with pytest.raises(ValueError, match="file 0: the log-mel must be a contiguous CUDA float32"):
        velocity.estimate([_NotATensor()], [ns])
    assert velocity.estimate([], []) == [] and velocity.estimate([], [], return_levels=True) == ([], [])
    with pytest.raises(ValueError, match="130 offsets"):
        velocity._check_table(np.zeros(3, np.int32), np.zeros(0, np.int32), 4)
    with pytest.raises(ValueError, match="outside the log-mel's 0 .. 2"):
        velocity._check_table(*cases.hand_table(), 3)
    for bad, what in ((note_sequences.Note(float("nan"), 1.0, 60, 100), "times must be finite"),
                      (note_sequences.Note(0.0, 1.0, 128, 100), "pitches are 0 .. 127, got 128")):
        with pytest.raises(ValueError, match="file 1: .*" + what):
            velocity.pack([ns, note_sequences.NoteSequence(notes=[bad])], [8, 8], [8, 8], 125.0)


def test_pack_puts_the_pitched_notes_first():
    from mt3_amd import note_sequences as NS
    a = NS.NoteSequence(notes=[NS.Note(0.1, 1.0, 36, 1, is_drum=True), NS.Note(0.0, 1.0, 60, 2), NS.Note(0.5, 1.0, 38, 3, 0, True),
                               NS.Note(0.016, 1.0, 72, 4), NS.Note(-0.001, 1.0, 0, 5)])
    b = NS.NoteSequence(notes=[NS.Note(1e12, 1.0, 127, 6)])
    p = velocity.pack([a, NS.NoteSequence(), b], [300, 256, 10], [512, 256, 256], 125.0)
    n = p.n_notes
    assert n == 6 and p.n_rows == 1024 and len(p.notes) == 12 * n
    frame, key, vel = (p.notes[4 * n * k: 4 * n * (k + 1)].view("<i4").tolist() for k in range(3))
    assert key == [60, 72, 0, 128, 128, 127] and vel == [2, 4, 5, 1, 3, 6]
    assert frame == [0, 2, -1, 12, 62, 2 ** 31 - 1]
    assert [s.tolist() for s in p.src] == [[1, 3, 4, 0, 2], [], [0]]
    assert p.files.tolist() == [(0, 0, 5, 3, 300, 0), (5, 512, 0, 0, 256, 0), (5, 768, 1, 1, 10, 0)]


def test_python_surface_and_command_line(tmp_path):
    from mt3_amd import inference, transcribe
    p = inspect.signature(velocity.estimate).parameters
    assert [(n, p[n].default) for n in p][:8] == [
        ("logmels", inspect.Parameter.empty), ("sequences", inspect.Parameter.empty), ("window", 8), ("harmonics", 6),
        ("gamma", 2.0), ("quantile", 0.5), ("anchor_velocity", 80), ("return_levels", False)]
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[2:])
    assert list(inspect.signature(velocity.harmonic_bins).parameters) == ["mel_matrix", "harmonics", "sample_rate", "fft_size"]
    for name in ("__call__", "transcribe_many", "transcribe_wav", "transcribe_wavs"):
        q = inspect.signature(getattr(inference.InferenceModel, name)).parameters["velocities"]
        assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY, name
    q = inspect.signature(inference.InferenceModel.note_velocities).parameters
    assert list(q)[:4] == ["self", "audio", "ns", "sample_rate"] and q["sample_rate"].default == 16000
    assert q["sample_rate"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(inference.InferenceModel.note_velocities_many).parameters)[:3] == ["self", "pairs",
                                                                                                     "sample_rates"]
    wav = tmp_path / "tune.wav"
    wav.write_bytes(b"")                                   # plan() only checks that the files exist
    args, _ = transcribe.plan(["--checkpoint", "random:0", str(wav)])
    assert not args.velocities and transcribe.velocity_keywords(args) is None
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--velocities", str(wav)])
    assert args.velocities and transcribe.velocity_keywords(args) == {}
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--velocities", "--velocity-gamma", "1", "--velocity-anchor", "64",
                               "--render", "8000", "--pianoroll", "50", str(wav)])
    assert transcribe.velocity_keywords(args) == {"gamma": 1.0, "anchor_velocity": 64.0}
    for flags in (["--velocity-gamma", "1"], ["--velocity-anchor", "64"], ["--velocities", "--velocity-gamma", "0"],
                  ["--velocities", "--velocity-anchor", "nan"], ["--velocities", "--model", "ismir2021"]):
        with pytest.raises(SystemExit):
            transcribe.plan(["--checkpoint", "random:0"] + flags + [str(wav)])
