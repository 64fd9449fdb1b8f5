"""mt3_op_track_beats and mt3_op_snap_notes on a box without a GPU: exported and typed, declared in the header, the
constants of the binding and the header agree, and every argument error that needs no device comes back as MT3_ERR_INVALID
with a text that starts with the function's name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mt3_amd import _lib, beats
from mt3_amd import note_sequences as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mt3_op_track_beats", "mt3_op_snap_notes")


def test_the_symbols_are_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mt3_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        decl = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name     # one argument per declared parameter
    for name, value in (("FPS", 100), ("LAG_MIN", 25), ("LAG_MAX", 200), ("PEN_STRIDE", 301), ("TILE", 1024),
                        ("MAX_SUBDIVISIONS", 48)):
        assert getattr(_lib, "BEATS_" + name) == value and "#define MT3_BEATS_%s %d\n" % (name, value) in header, name
    assert _lib.BEATS_MAX_FRAMES == 1 << 20 and "#define MT3_BEATS_MAX_FRAMES (1 << 20)" in header
    assert C.sizeof(_lib.BeatsFile) == beats.FILE_DTYPE.itemsize == 32
    assert C.sizeof(_lib.SnapFile) == beats.SNAP_FILE_DTYPE.itemsize == 24
    assert [n for n, _ in _lib.BeatsFile._fields_] == list(beats.FILE_DTYPE.names)
    assert [n for n, _ in _lib.SnapFile._fields_] == list(beats.SNAP_FILE_DTYPE.names)
    assert beats.PEN_STRIDE == 2 * beats.LAG_MAX - (beats.LAG_MAX + 1) // 2 + 1 and beats.LAG_MIN_HALF == 13
    assert lib.mt3_abi_version() == 4


def _p(a):
    return C.cast(a, C.c_void_p) if a is not None else None


def _buf(v, n, t):
    return None if v is None else (t * max(n, 1))()


def _track(lib, frames="ok", n_notes=8, files=((0, 0, 0, 8, 100),), n_files=None, prior="ok", n_prior=176, pen="ok",
           n_pen=176 * 301, rows="ok", back="ok", total_frames=100, period="ok", count="ok", out="ok", total_beats=9,
           score="ok"):
    """the call with host arrays standing in for the device arrays: none is read before the arguments are refused"""
    f = None if files is None else np.array([tuple(r) for r in files], beats.FILE_DTYPE)
    n_files = (0 if f is None else len(f)) if n_files is None else n_files
    return lib.mt3_op_track_beats(
        _p(_buf(frames, 8, C.c_int32)), n_notes, None if f is None else f.ctypes.data, n_files, _p(_buf(prior, 176, C.c_int64)),
        n_prior, _p(_buf(pen, 8, C.c_int64)), n_pen, _p(_buf(rows, 8, C.c_int32)), _p(_buf(back, 8, C.c_uint16)), total_frames,
        _p(_buf(period, 8, C.c_int32)), _p(_buf(count, 8, C.c_int32)), _p(_buf(out, 8, C.c_int32)), total_beats,
        _p(_buf(score, 8, C.c_int64)), None)


def test_track_beats_rejects_bad_calls_before_any_device_work():
    lib = _lib.load()
    calls = [
        (dict(frames=None), b"null onset frames"),
        (dict(files=None, n_files=1), b"null file table"),
        (dict(prior=None), b"null prior or penalty table"),
        (dict(pen=None), b"null prior or penalty table"),
        (dict(rows=None), b"null scratch rows or back pointers"),
        (dict(back=None), b"null scratch rows or back pointers"),
        (dict(period=None), b"null period, n_beats or score"),
        (dict(count=None), b"null period, n_beats or score"),
        (dict(score=None), b"null period, n_beats or score"),
        (dict(out=None), b"null beats"),
        (dict(n_notes=-1), b"n_notes must not be negative"),
        (dict(n_files=-2), b"n_files must not be negative"),
        (dict(total_frames=-1), b"total_frames and total_beats"),
        (dict(total_beats=-1), b"total_frames and total_beats"),
        (dict(n_prior=175), b"the prior table holds 176 lags"),
        (dict(n_prior=177), b"the prior table holds 176 lags"),
        (dict(n_pen=176 * 301 - 1), b"the penalty table holds 176 rows of 301"),
        (dict(n_pen=0), b"the penalty table holds 176 rows of 301"),
        (dict(files=((0, 0, 0, 8, -1),)), b"n_frames must be 0 .. 2^20 - 1"),
        (dict(files=((0, 0, 0, 8, 1 << 20),)), b"n_frames must be 0 .. 2^20 - 1"),
        (dict(files=((-1, 0, 0, 8, 100),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((1, 0, 0, 8, 100),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 0, 0, -1, 100),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, -1, 0, 8, 100),)), b"frame range must lie inside [0, total_frames]"),
        (dict(files=((0, 1, 0, 8, 100),)), b"frame range must lie inside [0, total_frames]"),
        (dict(files=((0, 0, -1, 8, 100),)), b"beat range"),
        (dict(files=((0, 0, 1, 8, 100),)), b"beat range"),                       # 100 / 13 + 2 = 9 slots from 1 on: 10 > 9
        (dict(total_beats=8), b"beat range"),
        (dict(files=((0, 0, 0, 5, 40), (4, 40, 5, 4, 40)), total_beats=10), b"note ranges overlap or are out of order"),
        (dict(files=((4, 0, 0, 4, 40), (0, 40, 5, 4, 40)), total_beats=10), b"note ranges overlap or are out of order"),
        (dict(files=((0, 0, 0, 4, 40), (4, 39, 5, 4, 40)), total_beats=10), b"frame ranges overlap or are out of order"),
        (dict(files=((0, 40, 0, 4, 40), (4, 0, 5, 4, 40)), total_beats=10), b"frame ranges overlap or are out of order"),
        (dict(files=((0, 0, 0, 4, 40), (4, 40, 4, 4, 40)), total_beats=10), b"beat ranges overlap or are out of order"),
        (dict(files=((0, 0, 5, 4, 40), (4, 40, 0, 4, 40)), total_beats=10), b"beat ranges overlap or are out of order"),
    ]
    for kw, what in calls:
        assert _track(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_track_beats: ") and what in msg, (kw, msg)
    # no files: nothing to do, whatever the device pointers are
    assert _track(lib, files=(), frames=None, prior=None, pen=None, rows=None, back=None, period=None, count=None, out=None,
                  score=None, n_notes=0, total_frames=0, total_beats=0) == _lib.MT3_OK


def _snap(lib, start="ok", end="ok", n_notes=8, frames="ok", n_frames=6, files=((0, 0, 8, 6),), n_files=None, sub=4,
          out_start="ok", out_end="ok"):
    f = None if files is None else np.array([tuple(r) for r in files], beats.SNAP_FILE_DTYPE)
    n_files = (0 if f is None else len(f)) if n_files is None else n_files
    return lib.mt3_op_snap_notes(_p(_buf(start, 8, C.c_double)), _p(_buf(end, 8, C.c_double)), n_notes,
                                 _p(_buf(frames, 8, C.c_int32)), n_frames, None if f is None else f.ctypes.data, n_files, sub,
                                 _p(_buf(out_start, 8, C.c_double)), _p(_buf(out_end, 8, C.c_double)), None)


def test_snap_notes_rejects_bad_calls_before_any_device_work():
    lib = _lib.load()
    calls = [
        (dict(start=None), b"null start, end or output column"),
        (dict(end=None), b"null start, end or output column"),
        (dict(out_start=None), b"null start, end or output column"),
        (dict(out_end=None), b"null start, end or output column"),
        (dict(frames=None), b"null beat frames"),
        (dict(files=None, n_files=1), b"null file table"),
        (dict(n_notes=-1), b"n_notes must not be negative"),
        (dict(n_frames=-1), b"n_beat_frames must not be negative"),
        (dict(n_files=-1), b"n_files must not be negative"),
        (dict(sub=0), b"subdivisions must be 1 .. 48"),
        (dict(sub=49), b"subdivisions must be 1 .. 48"),
        (dict(sub=-4), b"subdivisions must be 1 .. 48"),
        (dict(files=((-1, 0, 8, 6),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((1, 0, 8, 6),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 0, -1, 6),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 1, 8, 6),)), b"beat range must lie inside [0, n_beat_frames]"),
        (dict(files=((0, 0, 8, 7),)), b"beat range must lie inside [0, n_beat_frames]"),
        (dict(files=((0, 0, 8, -1),)), b"beat range must lie inside [0, n_beat_frames]"),
        (dict(files=((0, 0, 5, 3), (4, 3, 4, 3))), b"note ranges overlap or are out of order"),
        (dict(files=((4, 0, 4, 3), (0, 3, 4, 3))), b"note ranges overlap or are out of order"),
        (dict(files=((0, 0, 4, 4), (4, 3, 4, 3))), b"beat ranges overlap or are out of order"),
        (dict(files=((0, 3, 4, 3), (4, 0, 4, 3))), b"beat ranges overlap or are out of order"),
    ]
    for kw, what in calls:
        assert _snap(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_snap_notes: ") and what in msg, (kw, msg)
    assert _snap(lib, files=(), start=None, end=None, frames=None, out_start=None, out_end=None, n_notes=0,
                 n_frames=0) == _lib.MT3_OK


def _one(start, end=None):
    return N.NoteSequence(notes=[N.Note(start, start + 0.1 if end is None else end, 60, 90)])


@pytest.mark.parametrize("call", [beats.track, lambda s: beats.snap(s, [np.array([10, 60])] * 2)])
def test_the_wrappers_refuse_before_anything_is_uploaded(call):
    for bad in (_one(0.0), "notes", [_one(0.0), 3], None):
        with pytest.raises(ValueError, match="takes a list of NoteSequences"):
            call(bad)
    for bad in (float("nan"), float("inf"), -0.01):
        with pytest.raises(ValueError, match="file 1: note times must be finite and not negative"):
            call([_one(0.0), _one(bad, 1.0)])
    with pytest.raises(ValueError, match="file 0: note times must be finite and not negative"):
        call([_one(0.0, float("nan")), _one(0.0)])


def test_the_wrappers_take_an_empty_job_without_a_device():
    assert beats.track([]) == [] and beats.snap([], []) == []
