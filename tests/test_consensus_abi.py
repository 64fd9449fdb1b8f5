"""mt3_op_note_consensus on a box without a GPU: exported and typed, declared in the header with matching arity, its
constants mirrored, and every argument error comes back as MT3_ERR_INVALID -- before any device work -- with a text that
starts with the function's name and names the reason."""
import ctypes as C
import os
import re

import numpy as np

from mt3_amd import _lib, consensus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mt3_op_note_consensus"


def test_the_symbol_is_exported_typed_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mt3_hip.h")).read()
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    decl = re.search(r"^int %s\((.*?)\);" % NAME, header, re.M | re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[NAME][1]) == 20
    assert _lib.CONSENSUS_MAX_VOTERS == 64 and "#define MT3_CONSENSUS_MAX_VOTERS 64" in header
    assert _lib.CONSENSUS_TILE == 256 and "#define MT3_CONSENSUS_TILE 256" in header
    assert _lib.CONSENSUS_SCRATCH_WORDS_PER_NOTE == 4
    assert "#define MT3_CONSENSUS_SCRATCH_WORDS(n_notes) (4 * (int64_t)(n_notes))" in header
    assert C.sizeof(_lib.ConsensusFile) == consensus.FILE_DTYPE.itemsize == 24
    assert [n for n, _ in _lib.ConsensusFile._fields_] == list(consensus.FILE_DTYPE.names)
    assert consensus.MAX_VOTERS == 64
    assert lib.mt3_abi_version() == 4


def _call(lib, n_notes=8, files=((0, 8, 3, 2),), n_files=None, tolerance=0.05, scratch_words=None, **null):
    """the call with host arrays standing in for the device arrays: none is touched before the arguments are refused.
    files: (first, n_notes, n_voters, min_votes) each; null=True for a pointer name makes it NULL"""
    table = None
    if files is not None:
        table = np.zeros(len(files), consensus.FILE_DTYPE)
        for i, f in enumerate(files):
            table[i] = tuple(f) + (0,)
    n_files = (0 if table is None else len(table)) if n_files is None else n_files
    names = ("onset", "offset", "key", "velocity", "voter", "out_onset", "out_offset", "out_key", "out_velocity",
             "out_votes", "out_members", "note_votes", "counts", "scratch")
    assert set(null) <= set(names)
    buf = {n: None if null.get(n) else (C.c_double * 64)() for n in names}
    p = lambda n: None if buf[n] is None else C.cast(buf[n], C.c_void_p)          # noqa: E731
    return getattr(lib, NAME)(p("onset"), p("offset"), p("key"), p("velocity"), p("voter"), n_notes,
                              None if table is None else table.ctypes.data, n_files, tolerance, p("out_onset"),
                              p("out_offset"), p("out_key"), p("out_velocity"), p("out_votes"), p("out_members"),
                              p("note_votes"), p("counts"), p("scratch"),
                              4 * max(n_notes, 0) if scratch_words is None else scratch_words, None)


def test_bad_calls_are_refused_before_any_device_work():
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    calls = [(dict({name: True}), b"null note column") for name in ("onset", "offset", "key", "velocity", "voter")]
    calls += [(dict({name: True}), b"null consensus column")
              for name in ("out_onset", "out_offset", "out_key", "out_velocity", "out_votes", "out_members")]
    calls += [
        (dict(note_votes=True), b"null note_votes"),
        (dict(counts=True), b"null counts"),
        (dict(scratch=True), b"null scratch"),
        (dict(files=None, n_files=1), b"null file table"),
        (dict(n_notes=-1), b"n_notes must not be negative"),
        (dict(n_files=-2), b"n_files must not be negative"),
        (dict(files=((-1, 2, 3, 2),)), b"inside [0, n_notes]"),
        (dict(files=((0, -2, 3, 2),)), b"inside [0, n_notes]"),
        (dict(files=((0, 9, 3, 2),)), b"inside [0, n_notes]"),
        (dict(files=((9, 0, 3, 2),)), b"inside [0, n_notes]"),
        (dict(files=((4, 5, 3, 2),)), b"inside [0, n_notes]"),
        (dict(files=((0, 5, 3, 2), (4, 4, 3, 2))), b"overlap or are out of order"),
        (dict(files=((4, 4, 3, 2), (0, 4, 3, 2))), b"overlap or are out of order"),
        (dict(files=((0, 8, 0, 1),)), b"n_voters must be 1 .. 64"),
        (dict(files=((0, 8, 65, 1),)), b"n_voters must be 1 .. 64"),
        (dict(files=((0, 8, -1, 1),)), b"n_voters must be 1 .. 64"),
        (dict(files=((0, 8, 3, 0),)), b"min_votes must be 1 .. n_voters"),
        (dict(files=((0, 8, 3, 4),)), b"min_votes must be 1 .. n_voters"),
        (dict(files=((0, 4, 3, 2), (4, 4, 2, 3))), b"min_votes must be 1 .. n_voters"),
        (dict(tolerance=-1e-9), b"tolerance must be finite and not negative"),
        (dict(tolerance=nan), b"tolerance must be finite and not negative"),
        (dict(tolerance=inf), b"tolerance must be finite and not negative"),
        (dict(scratch_words=31), b"scratch too small"),
        (dict(scratch_words=-1), b"scratch too small"),
    ]
    for kw, what in calls:
        assert _call(lib, **kw) == _lib.MT3_ERR_INVALID, kw
        msg = lib.mt3_last_error()
        assert msg.startswith(b"mt3_op_note_consensus: ") and what in msg, (kw, msg)


def test_no_files_is_ok_and_launches_nothing():
    lib = _lib.load()
    null = {name: True for name in ("onset", "offset", "key", "velocity", "voter", "out_onset", "out_offset", "out_key",
                                    "out_velocity", "out_votes", "out_members", "note_votes", "counts", "scratch")}
    assert _call(lib, n_notes=0, files=(), **null) == _lib.MT3_OK
    assert _call(lib, n_notes=8, files=None, n_files=0, **null) == _lib.MT3_OK
