"""The three synchronisation ops and mt3_sync_workspace_bytes on a box without a GPU: exported and typed, declared in the
header, the constants of the binding and the header agree, and every argument error that needs no device comes back as
MT3_ERR_INVALID with a text that starts with the function's name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mt3_amd import _lib, sync
from mt3_amd import note_sequences as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("mt3_op_logmel_chroma", "mt3_op_note_chroma", "mt3_op_sync_paths")


def test_the_symbols_are_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mt3_hip.h")).read()
    for name, ret in [(n, "int") for n in OPS] + [("mt3_sync_workspace_bytes", "int64_t")]:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        decl = re.search(r"^%s %s\((.*?)\);" % (ret, name), header, re.M | re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    for name, value in (("CLASSES", 12), ("MAX_POOL", 16), ("HARMONICS", 6), ("LANES", 1024), ("STRIP", 16)):
        assert getattr(_lib, "SYNC_" + name) == value and "#define MT3_SYNC_%s %d\n" % (name, value) in header, name
    assert _lib.SYNC_MAX_FRAMES == 1 << 18 and "#define MT3_SYNC_MAX_FRAMES (1 << 18)" in header
    assert _lib.SYNC_MAX_CELLS == 1 << 31 and "#define MT3_SYNC_MAX_CELLS ((int64_t)1 << 31)" in header
    assert (2 * _lib.SYNC_MAX_FRAMES + _lib.SYNC_STRIP) * 3060 < 2 ** 31          # every D fits int32
    assert C.sizeof(_lib.SyncFile) == sync.FILE_DTYPE.itemsize == 64
    assert [n for n, _ in _lib.SyncFile._fields_] == list(sync.FILE_DTYPE.names)
    assert len(sync.OFFSETS) == _lib.SYNC_HARMONICS
    assert lib.mt3_abi_version() == 4


def _table(rows):
    """(row0, first, a0, s0, path0, work0, n_frames, n_notes, n, m) per file"""
    return np.array([tuple(r) for r in rows], sync.FILE_DTYPE)


def test_the_workspace_formula_is_the_library_s():
    lib = _lib.load()
    for n, m in ((0, 5), (5, 0), (1, 1), (7, 16), (7, 17), (300, 16 * 1024), (300, 16 * 1024 + 1), (3, 16 * 2048 + 40),
                 (1 << 18, 1 << 13)):
        t = _table([(0, 0, 0, 0, 0, 0, 0, 0, n, m)])
        assert lib.mt3_sync_workspace_bytes(t.ctypes.data, 1) == 4 * sync.workspace_words(n, m), (n, m)
    t = sync.file_table([50, 0, 80], [3, 0, 4], [12, 9, 40], 5)
    assert lib.mt3_sync_workspace_bytes(t.ctypes.data, 3) == 4 * (int(t["work0"][-1]) + sync.workspace_words(16, 40))
    assert lib.mt3_sync_workspace_bytes(None, 0) == 0
    for bad, what in (((1 << 18) + 1, 1), (1, (1 << 18) + 1), (-1, 1)):
        t = _table([(0, 0, 0, 0, 0, 0, 0, 0, bad, what)])
        assert lib.mt3_sync_workspace_bytes(t.ctypes.data, 1) == -1
        assert lib.mt3_last_error().startswith(b"mt3_sync_workspace_bytes: n and m must be 0 .. 2^18")
    t = _table([(0, 0, 0, 0, 0, 0, 0, 0, 1 << 18, (1 << 13) + 1)])
    assert lib.mt3_sync_workspace_bytes(t.ctypes.data, 1) == -1 and b"2^31 cells" in lib.mt3_last_error()
    assert lib.mt3_sync_workspace_bytes(None, 1) == -1 and b"null file table" in lib.mt3_last_error()


def _p(a):
    return C.cast(a, C.c_void_p) if a is not None else None


def _buf(v, t, n=64):
    return None if v is None else (t * n)()


OK_FILE = (0, 0, 0, 0, 0, 0, 20, 4, 4, 6)         # 20 rows pooled by 5 -> 4 frames; 4 notes; m = 6


def _files(files, n_files, d_files):
    f = None if files is None else _table(files)
    n_files = (0 if f is None else len(f)) if n_files is None else n_files
    dev = None if d_files is None else (C.c_int64 * 64)()
    return f, n_files, None if f is None else f.ctypes.data, _p(dev)


def _logmel(lib, logmel="ok", n_rows=20, n_mel=8, files=(OK_FILE,), n_files=None, d_files="ok", bins="ok", pool=5,
            range=4.0, floor=0.0, out="ok", total_a=4):
    """the call with host arrays standing in for the device arrays: none is read before the arguments are refused"""
    f, n_files, h, d = _files(files, n_files, d_files)
    return lib.mt3_op_logmel_chroma(_p(_buf(logmel, C.c_float)), n_rows, n_mel, h, d, n_files, _p(_buf(bins, C.c_int8)),
                                    pool, range, floor, _p(_buf(out, C.c_uint8)), total_a, None)


def _with(base=OK_FILE, **kw):
    rec = dict(zip(sync.FILE_DTYPE.names, base))
    rec.update(kw)
    return tuple(rec[k] for k in sync.FILE_DTYPE.names)


def test_logmel_chroma_rejects_bad_calls_before_any_device_work():
    lib = _lib.load()
    calls = [
        (dict(pool=0), b"pool must be 1 .. 16 rows"),
        (dict(pool=17), b"pool must be 1 .. 16 rows"),
        (dict(n_mel=0), b"n_mel must be 1 .. 4096"),
        (dict(n_mel=4097), b"n_mel must be 1 .. 4096"),
        (dict(range=0.0), b"range must be finite and > 0"),
        (dict(range=float("inf")), b"range must be finite and > 0"),
        (dict(range=float("nan")), b"range must be finite and > 0"),
        (dict(floor=float("nan")), b"floor must not be NaN"),
        (dict(n_rows=-1), b"n_rows and total_a must not be negative"),
        (dict(total_a=-1), b"n_rows and total_a must not be negative"),
        (dict(n_files=-1), b"n_files must not be negative"),
        (dict(files=None, n_files=1), b"null file table (host or device)"),
        (dict(d_files=None), b"null file table (host or device)"),
        (dict(files=(_with(n=5),)), b"a file's n must be ceil(n_frames / pool)"),
        (dict(files=(_with(n_frames=-1),)), b"a file's n must be ceil(n_frames / pool)"),
        (dict(n_rows=19), b"a file's row range must lie inside [0, n_rows]"),
        (dict(files=(_with(row0=-1),)), b"a file's row range must lie inside [0, n_rows]"),
        (dict(total_a=3), b"a file's audio feature range must lie inside [0, total_a]"),
        (dict(files=(_with(a0=-1),)), b"a file's audio feature range must lie inside [0, total_a]"),
        (dict(files=(OK_FILE, _with(a0=3)), total_a=8), b"audio feature ranges overlap or are out of order"),
        (dict(logmel=None), b"null log-mel, bins or output"),
        (dict(bins=None), b"null log-mel, bins or output"),
        (dict(out=None), b"null log-mel, bins or output"),
    ]
    for kw, what in calls:
        assert _logmel(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_logmel_chroma: ") and what in msg, (kw, msg)
    assert _logmel(lib, files=(), d_files=None, logmel=None, bins=None, out=None, n_rows=0, total_a=0) == _lib.MT3_OK


def _notes(lib, j0="ok", j1="ok", pitch="ok", n_notes=4, files=(OK_FILE,), n_files=None, d_files="ok", weights=(255,),
           n_harmonics=None, scratch="ok", out="ok", total_s=6):
    f, n_files, h, d = _files(files, n_files, d_files)
    w = None if weights is None else np.array(weights, np.int32)
    return lib.mt3_op_note_chroma(_p(_buf(j0, C.c_int32)), _p(_buf(j1, C.c_int32)), _p(_buf(pitch, C.c_int32)), n_notes, h,
                                  d, n_files, None if w is None else w.ctypes.data,
                                  (0 if w is None else len(w)) if n_harmonics is None else n_harmonics,
                                  _p(_buf(scratch, C.c_int32, 128)), _p(_buf(out, C.c_uint8, 128)), total_s, None)


def test_note_chroma_rejects_bad_calls_before_any_device_work():
    lib = _lib.load()
    calls = [
        (dict(n_notes=-1), b"n_notes and total_s must not be negative"),
        (dict(total_s=-1), b"n_notes and total_s must not be negative"),
        (dict(weights=None, n_harmonics=1), b"1 .. 6 harmonic weights"),
        (dict(weights=()), b"1 .. 6 harmonic weights"),
        (dict(weights=(1,) * 7), b"1 .. 6 harmonic weights"),
        (dict(weights=(255, 256)), b"a harmonic weight must be 0 .. 255"),
        (dict(weights=(-1,)), b"a harmonic weight must be 0 .. 255"),
        (dict(n_files=-1), b"n_files must not be negative"),
        (dict(files=None, n_files=1), b"null file table (host or device)"),
        (dict(d_files=None), b"null file table (host or device)"),
        (dict(files=(_with(m=(1 << 18) + 1),), total_s=1 << 19), b"m must be 0 .. 2^18 feature frames"),
        (dict(n_notes=3), b"a file's note range must lie inside [0, n_notes]"),
        (dict(files=(_with(first=-1),)), b"a file's note range must lie inside [0, n_notes]"),
        (dict(files=(_with(n_notes=-1),)), b"a file's note range must lie inside [0, n_notes]"),
        (dict(total_s=5), b"a file's score feature range must lie inside [0, total_s]"),
        (dict(files=(_with(n_notes=2), _with(first=1, n_notes=2, s0=6)), total_s=12), b"note ranges overlap or are out of order"),
        (dict(files=(_with(n_notes=2), _with(first=2, n_notes=2, s0=5)), total_s=12),
         b"score feature ranges overlap or are out of order"),
        (dict(scratch=None), b"null scratch or output"),
        (dict(out=None), b"null scratch or output"),
        (dict(j0=None), b"null note column (j0, j1 or pitch)"),
        (dict(j1=None), b"null note column (j0, j1 or pitch)"),
        (dict(pitch=None), b"null note column (j0, j1 or pitch)"),
    ]
    for kw, what in calls:
        assert _notes(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_note_chroma: ") and what in msg, (kw, msg)
    assert _notes(lib, files=(), d_files=None, j0=None, j1=None, pitch=None, scratch=None, out=None, n_notes=0,
                  total_s=0) == _lib.MT3_OK


WORDS = sync.workspace_words(4, 6)


def _paths(lib, a="ok", total_a=4, s="ok", total_s=6, files=(OK_FILE,), n_files=None, d_files="ok", work="ok",
           work_bytes=4 * WORDS, path_i="ok", path_j="ok", total_path=9, length="ok", total="ok"):
    f, n_files, h, d = _files(files, n_files, d_files)
    return lib.mt3_op_sync_paths(_p(_buf(a, C.c_uint8, 128)), total_a, _p(_buf(s, C.c_uint8, 128)), total_s, h, d, n_files,
                                 _p(_buf(work, C.c_int32, 128)), work_bytes, _p(_buf(path_i, C.c_int32)),
                                 _p(_buf(path_j, C.c_int32)), total_path, _p(_buf(length, C.c_int32)),
                                 _p(_buf(total, C.c_int32)), None)


def test_sync_paths_rejects_bad_calls_before_any_device_work():
    lib = _lib.load()
    over = (1 << 18) + 1
    two = (_with(), _with(a0=4, s0=6, path0=9, work0=WORDS))
    calls = [
        (dict(total_a=-1), b"must not be negative"),
        (dict(total_s=-1), b"must not be negative"),
        (dict(total_path=-1), b"must not be negative"),
        (dict(work_bytes=-1), b"must not be negative"),
        (dict(n_files=-1), b"n_files must not be negative"),
        (dict(files=None, n_files=1), b"null file table (host or device)"),
        (dict(d_files=None), b"null file table (host or device)"),
        (dict(files=(_with(n=over),), total_a=over), b"n and m must be 0 .. 2^18 feature frames"),        # frames over the limit
        (dict(files=(_with(m=over),), total_s=over), b"n and m must be 0 .. 2^18 feature frames"),
        (dict(files=(_with(n=-1),)), b"n and m must be 0 .. 2^18 feature frames"),
        (dict(files=(_with(n=1 << 18, m=(1 << 13) + 1),), total_a=1 << 18, total_s=1 << 14),
         b"n * m must not exceed 2^31 cells"),                                                           # cells over the limit
        (dict(total_a=3), b"a file's audio feature range must lie inside [0, total_a]"),
        (dict(total_s=5), b"a file's score feature range must lie inside [0, total_s]"),
        (dict(total_path=8), b"a file's path range must lie inside [0, total_path]"),
        (dict(files=(two[0], _with(two[1], a0=3)), total_a=8, total_s=12, total_path=18, work_bytes=8 * WORDS),
         b"audio feature ranges overlap or are out of order"),                                           # overlapping ranges
        (dict(files=(two[0], _with(two[1], s0=5)), total_a=8, total_s=12, total_path=18, work_bytes=8 * WORDS),
         b"score feature ranges overlap or are out of order"),
        (dict(files=(two[0], _with(two[1], path0=8)), total_a=8, total_s=12, total_path=18, work_bytes=8 * WORDS),
         b"path ranges overlap or are out of order"),
        (dict(files=(two[0], _with(two[1], work0=WORDS - 1)), total_a=8, total_s=12, total_path=18, work_bytes=8 * WORDS),
         b"workspace ranges overlap or are out of order"),
        (dict(files=(two[1], two[0]), total_a=8, total_s=12, total_path=18, work_bytes=8 * WORDS),
         b"ranges overlap or are out of order"),
        (dict(length=None), b"null path_len or total"),
        (dict(total=None), b"null path_len or total"),
        (dict(a=None), b"null features or path"),
        (dict(s=None), b"null features or path"),
        (dict(path_i=None), b"null features or path"),
        (dict(path_j=None), b"null features or path"),
        (dict(work=None), b"null workspace"),                                                            # a null workspace
        (dict(work_bytes=4 * WORDS - 4), b"the workspace is too short"),                                 # a short workspace
        (dict(work_bytes=0), b"the workspace is too short"),
        (dict(files=two, total_a=8, total_s=12, total_path=18, work_bytes=8 * WORDS - 4), b"the workspace is too short"),
    ]
    for kw, what in calls:
        assert _paths(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_sync_paths: ") and what in msg, (kw, msg)
    assert _paths(lib, files=(), d_files=None, a=None, s=None, work=None, path_i=None, path_j=None, length=None, total=None,
                  total_a=0, total_s=0, total_path=0, work_bytes=0) == _lib.MT3_OK


def _one(start, end=None, pitch=60):
    return N.NoteSequence(notes=[N.Note(start, start + 0.1 if end is None else end, pitch, 90)])


def test_synchronize_refuses_before_anything_is_uploaded():
    with pytest.raises(ValueError, match="logmels has 1 entries for 2 sequences"):
        sync.synchronize([None], [_one(0.0), _one(0.0)])
    for pool in (0, 17, 2.5):
        with pytest.raises(ValueError, match="pool must be 1 .. 16"):
            sync.synchronize([None], [_one(0.0)], pool=pool)
    for weights in ((), (1,) * 7, (256,), (-1,), (1.5,)):
        with pytest.raises(ValueError, match="harmonic_weights must be 1 .. 6 integers 0 .. 255"):
            sync.synchronize([None], [_one(0.0)], harmonic_weights=weights)
    with pytest.raises(ValueError, match="range must be a finite number > 0"):
        sync.synchronize([None], [_one(0.0)], range=0.0)
    with pytest.raises(ValueError, match="file 0: the log-mel must be a contiguous CUDA float32"):
        sync.synchronize([np.zeros((1, 256, 512), np.float32)], [_one(0.0)])
    assert sync.synchronize([], []) == []
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="file 1: note times must be finite"):
            sync.pack([_one(0.0), _one(bad, 1.0)], [10, 10], [10, 10], 5, 25.0)
    with pytest.raises(ValueError, match="file 0: note times must not be negative"):
        sync.pack([_one(-0.5, 1.0)], [10], [10], 5, 25.0)
    with pytest.raises(ValueError, match="file 0: pitches are 0 .. 127, got 128"):
        sync.pack([_one(0.0, pitch=128)], [10], [10], 5, 25.0)
