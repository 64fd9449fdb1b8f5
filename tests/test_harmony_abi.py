"""mt3_op_analyze_harmony on a box without a GPU: exported and typed, declared in the header, the constants of the binding
and the header agree, and every argument error that needs no device comes back as MT3_ERR_INVALID with a text that starts
with the function's name."""
import ctypes as C
import os
import re

import numpy as np

from mt3_amd import _lib, harmony

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mt3_op_analyze_harmony"


def test_the_symbol_is_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mt3_hip.h")).read()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    decl = re.search(r"^int %s\((.*?)\);" % NAME, header, re.M | re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[NAME][1])             # one argument per declared parameter
    for name, value in (("STATES", 25), ("KEYS", 24), ("BEAT_TILE", 32), ("NOTE_TILE", 256), ("ONSET_WINDOW", 3),
                        ("MAX_WEIGHT", 255), ("WORKSPACE_BYTES_PER_BEAT", 27)):
        assert getattr(_lib, "HARMONY_" + name) == value and "#define MT3_HARMONY_%s %d\n" % (name, value) in header, name
    assert _lib.HARMONY_MAX_CHANGE_PENALTY == 1 << 20 and "#define MT3_HARMONY_MAX_CHANGE_PENALTY (1 << 20)" in header
    assert C.sizeof(_lib.HarmonyFile) == harmony.FILE_DTYPE.itemsize == 24
    assert [n for n, _ in _lib.HarmonyFile._fields_] == list(harmony.FILE_DTYPE.names)
    assert harmony.key_profiles().shape == (_lib.HARMONY_KEYS, 12) and harmony.STATES == 1 + 2 * 12
    assert lib.mt3_abi_version() == 4


def _p(a):
    return C.cast(a, C.c_void_p) if a is not None else None


def _buf(v, n, t):
    return None if v is None else (t * max(n, 1))()


def _call(lib, start="ok", end="ok", key="ok", h_key=(60, 64, 67 + 256, 0, 127, 60, 60, 60), n_notes=8, beats="ok",
          h_beats=(10, 50, 90, 130, 170, 210), n_beats=6, files=((0, 0, 8, 6),), d_files="ok", n_files=None, profiles="ok",
          n_profiles=288, penalty=100, weights=(1, 4, 2), workspace="ok", workspace_bytes=27 * 6, scores="ok", info="ok",
          chords="ok"):
    """the call with host arrays standing in for the device arrays: none is read before the arguments are refused"""
    f = None if files is None else np.array([tuple(r) for r in files], harmony.FILE_DTYPE)
    n_files = (0 if f is None else len(f)) if n_files is None else n_files
    hk = None if h_key is None else np.array(h_key, np.int32)
    hb = None if h_beats is None else np.array(h_beats, np.int32)
    ws = _buf(workspace, 256, C.c_uint16)
    ws_at = None if ws is None else C.addressof(ws) + (1 if workspace == "odd" else 0)
    return lib.mt3_op_analyze_harmony(
        _p(_buf(start, 8, C.c_int32)), _p(_buf(end, 8, C.c_int32)), _p(_buf(key, 8, C.c_int32)),
        None if hk is None else hk.ctypes.data, n_notes, _p(_buf(beats, 8, C.c_int32)), None if hb is None else hb.ctypes.data,
        n_beats, None if f is None else f.ctypes.data, None if d_files is None or f is None else f.ctypes.data, n_files,
        _p(_buf(profiles, 288, C.c_int32)), n_profiles, penalty, *weights, ws_at, workspace_bytes,
        _p(_buf(scores, 24, C.c_int64)), _p(_buf(info, 4, C.c_int32)), _p(_buf(chords, 8, C.c_int8)), None)


def test_analyze_harmony_rejects_bad_calls_before_any_device_work():
    lib = _lib.load()
    calls = [
        (dict(start=None), b"null note column"),
        (dict(end=None), b"null note column"),
        (dict(key=None), b"null note column"),
        (dict(h_key=None), b"null note column"),
        (dict(beats=None), b"null beat frames"),
        (dict(h_beats=None), b"null beat frames"),
        (dict(files=None, n_files=1), b"null file table"),
        (dict(d_files=None), b"null file table"),
        (dict(profiles=None), b"null profile table"),
        (dict(scores=None), b"null key_scores or info"),
        (dict(info=None), b"null key_scores or info"),
        (dict(chords=None), b"null chords"),
        (dict(workspace=None), b"null workspace"),
        (dict(workspace="odd"), b"the workspace must be 2-byte aligned"),
        (dict(workspace_bytes=27 * 6 - 1), b"the workspace holds 27 bytes per beat"),
        (dict(n_notes=-1), b"n_notes must not be negative"),
        (dict(n_beats=-1), b"n_beats must not be negative"),
        (dict(n_files=-2), b"n_files must not be negative"),
        (dict(n_profiles=287), b"the profile table holds 24 rows of 12"),
        (dict(n_profiles=0), b"the profile table holds 24 rows of 12"),
        (dict(penalty=-1), b"change_penalty must be 0 .. 2^20"),
        (dict(penalty=(1 << 20) + 1), b"change_penalty must be 0 .. 2^20"),
        (dict(weights=(-1, 4, 2)), b"onset_weight, change_weight and bass_weight must be 0 .. 255"),
        (dict(weights=(1, 256, 2)), b"onset_weight, change_weight and bass_weight must be 0 .. 255"),
        (dict(weights=(1, 4, 1000)), b"onset_weight, change_weight and bass_weight must be 0 .. 255"),
        (dict(files=((-1, 0, 8, 6),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((1, 0, 8, 6),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 0, -1, 6),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 1, 8, 6),)), b"beat range must lie inside [0, n_beats]"),
        (dict(files=((0, 0, 8, 7),)), b"beat range must lie inside [0, n_beats]"),
        (dict(files=((0, 0, 8, -1),)), b"beat range must lie inside [0, n_beats]"),
        (dict(files=((0, 0, 5, 3), (4, 3, 4, 3))), b"note ranges overlap or are out of order"),
        (dict(files=((4, 0, 4, 3), (0, 3, 4, 3))), b"note ranges overlap or are out of order"),
        (dict(files=((0, 0, 4, 4), (4, 3, 4, 3))), b"beat ranges overlap or are out of order"),
        (dict(files=((0, 3, 4, 3), (4, 0, 4, 3))), b"beat ranges overlap or are out of order"),
        (dict(h_key=(60, 64, 128, 0, 0, 0, 0, 0)), b"a key is pitch + 256 * is_drum with a pitch of 0 .. 127"),
        (dict(h_key=(60, 64, -1, 0, 0, 0, 0, 0)), b"a key is pitch + 256 * is_drum with a pitch of 0 .. 127"),
        (dict(h_key=(60, 64, 512, 0, 0, 0, 0, 0)), b"a key is pitch + 256 * is_drum with a pitch of 0 .. 127"),
        (dict(h_key=(60, 64, 256 + 128, 0, 0, 0, 0, 0)), b"a key is pitch + 256 * is_drum with a pitch of 0 .. 127"),
        (dict(h_beats=(10, 50, 50, 130, 170, 210)), b"beat frames must ascend strictly inside 0 .. 2^20 - 1"),
        (dict(h_beats=(10, 50, 40, 130, 170, 210)), b"beat frames must ascend strictly inside 0 .. 2^20 - 1"),
        (dict(h_beats=(-1, 50, 90, 130, 170, 210)), b"beat frames must ascend strictly inside 0 .. 2^20 - 1"),
        (dict(h_beats=(10, 50, 90, 130, 170, 1 << 20)), b"beat frames must ascend strictly inside 0 .. 2^20 - 1"),
        # 4096 notes (only the first file's keys are read) times an interval of 2^19 frames: 2^31
        (dict(files=((0, 0, 8, 2), (8, 2, 4096, 2)), n_notes=8 + 4096, h_key=(60,) * (8 + 4096),
              h_beats=(10, 50, 0, 1 << 19, 0, 0)), b"notes times its longest beat interval must stay below 2^31"),
    ]
    for kw, what in calls:
        assert _call(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_analyze_harmony: ") and what in msg, (kw, msg)
    # no files: nothing to do, whatever the device pointers are
    assert _call(lib, files=(), start=None, end=None, key=None, h_key=None, beats=None, h_beats=None, profiles=None,
                 workspace=None, scores=None, info=None, chords=None, n_notes=0, n_beats=0, workspace_bytes=0) == _lib.MT3_OK


def test_the_wrapper_takes_an_empty_job_without_a_device():
    assert harmony.analyze([], []) == [] and harmony.analyze_reference([], []) == []
