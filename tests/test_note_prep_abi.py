"""mt3_op_prepare_notes on a box without a GPU: exported and typed, declared in the header with matching arity, its
constants and its file record mirrored, the host packing as the header states it, and every argument error comes back as
MT3_ERR_INVALID -- before any device work -- with a text that starts with the function's name and names the reason."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mt3_amd import _lib, note_prep
from tests import note_prep_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mt3_op_prepare_notes"
POINTERS = ("start", "end", "key", "pos", "pedal_time", "pedal_inst_state", "out_end", "out_src", "counts", "total_time",
            "scratch")


def test_the_symbol_is_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mt3_hip.h")).read()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    decl = re.search(r"^int %s\((.*?)\);" % NAME, header, re.M | re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[NAME][1]) == 18
    assert _lib.NOTE_PREP_SUSTAIN == 0 and "#define MT3_NOTE_PREP_SUSTAIN 0" in header
    assert _lib.NOTE_PREP_TRIM == 1 and "#define MT3_NOTE_PREP_TRIM 1" in header
    assert _lib.NOTE_PREP_TILE == 256 and "#define MT3_NOTE_PREP_TILE 256" in header
    assert "#define MT3_NOTE_PREP_SCRATCH_WORDS(n_notes, n_pedal) (3 * (int64_t)(n_notes) + (int64_t)(n_pedal))" in header
    assert C.sizeof(_lib.NotePrepFile) == note_prep.FILE_DTYPE.itemsize == 40
    assert [n for n, _ in _lib.NotePrepFile._fields_] == list(note_prep.FILE_DTYPE.names)
    assert [getattr(_lib.NotePrepFile, n).offset for n in note_prep.FILE_DTYPE.names] == \
        [note_prep.FILE_DTYPE.fields[n][1] for n in note_prep.FILE_DTYPE.names]
    assert lib.mt3_abi_version() == 4                                  # an additive entry point


def test_pack_sorts_as_the_header_states():
    ns, _, _ = ref.HAND["two_instruments_opposite_pedals"]
    files = [note_prep.columns(ns, 0), note_prep.columns(ref.HAND["never_released"][0], 1)]
    p = note_prep.pack(files, note_prep.SUSTAIN)
    n = p.n_notes
    assert n == 6 and p.n_pedal == 7 and len(p.notes) == 24 * n and len(p.pedal) == 12 * p.n_pedal
    start, end = p.notes[: 8 * n].view("<f8"), p.notes[8 * n: 16 * n].view("<f8")
    key, pos = p.notes[16 * n: 20 * n].view("<i4"), p.notes[20 * n:].view("<i4")
    assert key.tolist() == [60, 60, 128 + 60, 128 + 60, 60, 64] and pos.tolist() == [0, 2, 1, 3, 0, 1]
    assert start.tolist() == [0.0, 2.5, 0.0, 2.5, 0.0, 1.0] and end.tolist() == [1.0, 3.0, 1.0, 3.0, 1.0, 3.0]
    assert p.pedal[: 8 * 7].view("<f8").tolist() == [0.0, 2.0, 4.0, 0.0, 2.0, 4.0, 0.5]
    assert p.pedal[8 * 7:].view("<i4").tolist() == [0, 1, 0, 3, 2, 3, 0]          # instrument << 1 | OFF
    assert p.files.tolist() == [(0, 0, 4, 6, 4.0, 3.0), (4, 6, 2, 1, 3.0, 5.0)]
    t = note_prep.pack(files, note_prep.TRIM)
    assert t.n_pedal == 0 and len(t.pedal) == 0 and t.files["n_pedal"].tolist() == [0, 0]
    assert t.notes[16 * n: 20 * n].view("<i4").tolist() == [60, 60, 60, 60, 60, 64]      # is_drum << 14 | program << 7 | pitch
    assert t.notes[20 * n:].view("<i4").tolist() == [0, 1, 2, 3, 0, 1]


def test_prepare_refuses_bad_notes_before_anything_is_uploaded():
    bad = [
        (ref.seq([(60, 100, float("nan"), 1.0)]), "times must be finite"),
        (ref.seq([(60, 100, 0.0, float("inf"))]), "times must be finite"),
        (ref.seq([(128, 100, 0.0, 1.0)]), "pitches are 0 .. 127, got 128"),
        (ref.seq([(60, 100, 0.0, 1.0, 0, 128)]), "programs are 0 .. 127, got 128"),
        (ref.seq([(60, 100, 0.0, 1.0, 65536)]), "instruments are 0 .. 65535, got 65536"),
        (ref.seq([(60, 100, 0.0, 1.0)], [(0.0, 127, -1)]), "instruments are 0 .. 65535, got -1"),
        (ref.seq([(60, 100, 0.0, 1.0)], [(float("nan"), 127)]), "control changes: note times must be finite"),
        (ref.seq([(60, 100, 2.0, 1.0)]), "a note ends before it starts"),
        (ref.seq([(60, 100, 0.0, 1.0)], total_time=float("inf")), "total_time must be finite"),
    ]
    for ns, what in bad:
        with pytest.raises(ValueError, match=re.escape("file 1: ") + ".*" + re.escape(what)):
            note_prep.prepare([ref.seq([]), ns])


def test_python_surface_and_command_line(tmp_path):
    import inspect
    from mt3_amd import inference, transcribe
    for name in ("targets", "score_notes_many", "align_notes", "align_notes_many"):
        p = inspect.signature(getattr(inference.InferenceModel, name)).parameters
        assert p["sustain"].default is False and p["sustain"].kind is inspect.Parameter.KEYWORD_ONLY, name
    p = inspect.signature(note_prep.prepare).parameters
    assert [(n, p[n].default) for n in p] == [("sequences", inspect.Parameter.empty), ("sustain", True), ("trim", False),
                                              ("as_arrays", False)]
    wav, refs = tmp_path / "tune.wav", tmp_path / "refs"
    wav.write_bytes(b"")                                   # plan() only checks that the files exist
    refs.mkdir()
    (refs / "tune.mid").write_bytes(b"")
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--score-midi", str(refs), "--sustain", str(wav)])
    assert args.sustain and not args.trim_overlaps
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--align-midi", str(refs), "--trim-overlaps", str(wav)])
    assert args.trim_overlaps and not args.sustain
    args, _ = transcribe.plan(["--checkpoint", "random:0", "--score-against", str(refs), str(wav)])
    assert not args.sustain and not args.trim_overlaps
    for flag in ("--sustain", "--trim-overlaps"):
        with pytest.raises(SystemExit):
            transcribe.plan(["--checkpoint", "random:0", flag, str(wav)])


def _call(lib, mode=0, n_notes=8, n_pedal=4, files=((0, 0, 8, 4, 1.0, 1.0),), n_files=None, scratch_words=None,
          misalign=False, **null):
    """the call with host arrays standing in for the device arrays: none is touched before the arguments are refused.
    files: (first, pedal_first, n_notes, n_pedal, t_last, total_time) each; null=True for a pointer name makes it NULL"""
    table = None
    if files is not None:
        table = np.zeros(len(files), note_prep.FILE_DTYPE)
        for i, f in enumerate(files):
            table[i] = tuple(f)
    n_files = (0 if table is None else len(table)) if n_files is None else n_files
    assert set(null) <= set(POINTERS)
    buf = {n: None if null.get(n) else (C.c_double * 64)() for n in POINTERS}
    p = lambda n: None if buf[n] is None else C.cast(buf[n], C.c_void_p)          # noqa: E731
    scratch = p("scratch")
    if misalign:
        scratch = C.c_void_p(scratch.value + 4)
    words = 3 * max(n_notes, 0) + (max(n_pedal, 0) if mode == 0 else 0)
    return getattr(lib, NAME)(mode, p("start"), p("end"), p("key"), p("pos"), n_notes, p("pedal_time"),
                              p("pedal_inst_state"), n_pedal, None if table is None else table.ctypes.data, n_files,
                              p("out_end"), p("out_src"), p("counts"), p("total_time"), scratch,
                              words if scratch_words is None else scratch_words, None)


def test_bad_calls_are_refused_before_any_device_work():
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    calls = [(dict({name: True}), b"null note column") for name in ("start", "end", "key", "pos")]
    calls += [(dict({name: True}), b"null pedal column") for name in ("pedal_time", "pedal_inst_state")]
    calls += [(dict({name: True}), b"null output column") for name in ("out_end", "out_src")]
    calls += [
        (dict(counts=True), b"null counts"),
        (dict(total_time=True), b"null total_time"),
        (dict(scratch=True), b"null scratch"),
        (dict(misalign=True), b"8-byte aligned"),
        (dict(files=None, n_files=1), b"null file table"),
        (dict(mode=2), b"unknown mode"),
        (dict(mode=-1), b"unknown mode"),
        (dict(n_notes=-1), b"n_notes must not be negative"),
        (dict(n_pedal=-1), b"n_pedal must not be negative"),
        (dict(n_files=-2), b"n_files must not be negative"),
        (dict(files=((-1, 0, 2, 4, 1.0, 1.0),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 0, -2, 4, 1.0, 1.0),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 0, 9, 4, 1.0, 1.0),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((9, 0, 0, 4, 1.0, 1.0),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((4, 0, 5, 4, 1.0, 1.0),)), b"note range must lie inside [0, n_notes]"),
        (dict(files=((0, 0, 5, 2, 1.0, 1.0), (4, 2, 4, 2, 1.0, 1.0))), b"note ranges overlap or are out of order"),
        (dict(files=((4, 0, 4, 2, 1.0, 1.0), (0, 2, 4, 2, 1.0, 1.0))), b"note ranges overlap or are out of order"),
        (dict(files=((0, -1, 8, 2, 1.0, 1.0),)), b"pedal range must lie inside [0, n_pedal]"),
        (dict(files=((0, 0, 8, -1, 1.0, 1.0),)), b"pedal range must lie inside [0, n_pedal]"),
        (dict(files=((0, 0, 8, 5, 1.0, 1.0),)), b"pedal range must lie inside [0, n_pedal]"),
        (dict(files=((0, 3, 8, 2, 1.0, 1.0),)), b"pedal range must lie inside [0, n_pedal]"),
        (dict(files=((0, 0, 4, 3, 1.0, 1.0), (4, 2, 4, 2, 1.0, 1.0))), b"pedal ranges overlap or are out of order"),
        (dict(files=((0, 2, 4, 2, 1.0, 1.0), (4, 0, 4, 2, 1.0, 1.0))), b"pedal ranges overlap or are out of order"),
        (dict(files=((0, 0, 8, 4, nan, 1.0),)), b"t_last and total_time must be finite"),
        (dict(files=((0, 0, 8, 4, 1.0, inf),)), b"t_last and total_time must be finite"),
        (dict(scratch_words=27), b"scratch too small"),
        (dict(scratch_words=-1), b"scratch too small"),
        (dict(mode=1, scratch_words=23), b"scratch too small"),
    ]
    for kw, what in calls:
        assert _call(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_prepare_notes: ") and what in msg, (kw, msg)


def test_no_files_is_ok_and_launches_nothing():
    lib = _lib.load()
    null = {name: True for name in POINTERS}
    assert _call(lib, n_notes=0, n_pedal=0, files=(), **null) == _lib.MT3_OK
    assert _call(lib, n_notes=8, files=None, n_files=0, **null) == _lib.MT3_OK
    assert _call(lib, mode=1, n_notes=8, files=None, n_files=0, **null) == _lib.MT3_OK
