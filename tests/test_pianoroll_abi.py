"""mt3_op_pianoroll / mt3_op_frame_counts on a box without a GPU: the symbols and their prototypes, and every argument
check of include/mt3_hip.h -- all of which come before any HIP call, so the "device" pointers here are host memory that
must come back untouched.  No CUDA call in this file."""
import ctypes as C
import inspect

import numpy as np

from mt3_amd import _lib, inference, metrics, metrics_utils, pianoroll, transcribe

I64 = lambda *v: np.array(v, np.int64)          # noqa: E731
I32 = lambda *v: np.array(v, np.int32)          # noqa: E731


def test_symbols_are_exported_and_typed():
    lib = _lib.load()
    _P = C.c_void_p
    assert _lib.SIGNATURES["mt3_op_pianoroll"] == (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, _P,
                                                             C.c_double, C.c_int32, _P, C.c_int64, _P])
    assert _lib.SIGNATURES["mt3_op_frame_counts"] == (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P])
    for name in ("mt3_op_pianoroll", "mt3_op_frame_counts"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4
    assert (pianoroll.PITCHES, pianoroll.MIN_NOTE_SECONDS) == (128, 0.05)


class _Job:
    """a well-formed two-roll call on host memory; `with_(name=value)` swaps one argument"""

    def __init__(self):
        self.notes = np.zeros(64, np.float64)
        self.out = np.full(128 * 16, 7.0, np.float32)
        p = self.notes.ctypes.data
        self.args = dict(d_start=p, d_end=p, d_pitch=p, d_velocity=p, d_is_drum=p, n_notes=6, n_rolls=2,
                         note_offsets=I64(0, 2, 6), col_offsets=I64(0, 4), widths=I32(4, 5), fps=62.5, is_drum=0,
                         d_out=self.out.ctypes.data, out_capacity=128 * 16, stream=None)

    def call(self, **swap):
        a = dict(self.args, **swap)
        self.keep = a
        tab = lambda v: None if v is None else v.ctypes.data        # noqa: E731
        return _lib.load().mt3_op_pianoroll(a["d_start"], a["d_end"], a["d_pitch"], a["d_velocity"], a["d_is_drum"],
                                            a["n_notes"], a["n_rolls"], tab(a["note_offsets"]), tab(a["col_offsets"]),
                                            tab(a["widths"]), a["fps"], a["is_drum"], a["d_out"], a["out_capacity"],
                                            a["stream"])


def test_pianoroll_rejects_bad_arguments_before_any_device_call():
    lib, job = _lib.load(), _Job()
    bad = [
        (dict(n_rolls=-1), b"n_rolls"),
        (dict(n_notes=-1), b"n_notes"),
        (dict(fps=0.0), b"fps"), (dict(fps=-62.5), b"fps"), (dict(fps=float("nan")), b"fps"), (dict(fps=float("inf")), b"fps"),
        (dict(note_offsets=None), b"null table"), (dict(col_offsets=None), b"null table"), (dict(widths=None), b"null table"),
        (dict(d_start=None), b"null note array"), (dict(d_end=None), b"null note array"), (dict(d_pitch=None), b"null note array"),
        (dict(d_velocity=None), b"null note array"), (dict(d_is_drum=None), b"null note array"),
        (dict(d_out=None), b"null d_out"),
        (dict(note_offsets=I64(0, 4, 3)), b"must not decrease"),
        (dict(note_offsets=I64(-1, 2, 6)), b"inside [0, n_notes]"),
        (dict(note_offsets=I64(0, 2, 7)), b"inside [0, n_notes]"),
        (dict(note_offsets=I64(0, 2 ** 31, 2 ** 31), n_notes=2 ** 31), b"2^31 - 1 notes"),
        (dict(widths=I32(4, -5)), b"negative width"),
        (dict(col_offsets=I64(-1, 4)), b"column offset"),
        (dict(col_offsets=I64(0, 2 ** 62)), b"column offset"),
        (dict(col_offsets=I64(0, 3)), b"overlap"),                  # roll 1 starts inside roll 0
        (dict(col_offsets=I64(5, 0)), b"overlap"),                  # out of order
        (dict(out_capacity=128 * 9 - 1), b"out_capacity"),          # one float short
        (dict(out_capacity=-1), b"out_capacity"),
    ]
    for swap, word in bad:
        assert job.call(**swap) == _lib.MT3_ERR_INVALID, swap
        err = lib.mt3_last_error()
        assert err.startswith(b"mt3_op_pianoroll: ") and word in err, (swap, err)
    assert (job.out == 7.0).all() and not job.notes.any()          # host memory: nothing may have touched it


def test_pianoroll_calls_that_do_nothing_succeed():
    job = _Job()
    assert job.call(n_rolls=0) == _lib.MT3_OK
    assert job.call(n_rolls=0, n_notes=0, note_offsets=None, col_offsets=None, widths=None, d_start=None, d_end=None,
                    d_pitch=None, d_velocity=None, d_is_drum=None, d_out=None, out_capacity=0) == _lib.MT3_OK
    # rolls that are all empty: nothing to write, so no buffer is needed and no device either
    assert job.call(widths=I32(0, 0), col_offsets=I64(0, 0), d_out=None, out_capacity=0) == _lib.MT3_OK
    assert (job.out == 7.0).all()


def _counts(lib, d_rolls, cap, n, ref_c, ref_w, est_c, est_w, thr, d_counts):
    tab = lambda v: None if v is None else v.ctypes.data            # noqa: E731
    return lib.mt3_op_frame_counts(d_rolls, cap, n, tab(ref_c), tab(ref_w), tab(est_c), tab(est_w), thr, d_counts, None)


def test_frame_counts_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    rolls, counts = np.full(128 * 16, 7.0, np.float32), np.full(6, 99, np.uint64)
    r, c, cap = rolls.ctypes.data, counts.ctypes.data, 128 * 16
    good = (I64(0, 4), I32(4, 5), I64(9, 9), I32(7, 0))
    bad = [
        ((r, cap, -1, *good, 30, c), b"n_pairs"),
        ((r, -1, 2, *good, 30, c), b"rolls_capacity"),
        ((r, cap, 2, None, *good[1:], 30, c), b"null table"),
        ((r, cap, 2, good[0], None, *good[2:], 30, c), b"null table"),
        ((r, cap, 2, *good[:2], None, good[3], 30, c), b"null table"),
        ((r, cap, 2, *good[:3], None, 30, c), b"null table"),
        ((r, cap, 2, *good, 30, None), b"null d_counts"),
        ((None, cap, 2, *good, 30, c), b"null d_rolls"),
        ((r, cap, 2, I64(0, 4), I32(4, -5), *good[2:], 30, c), b"reference roll"),
        ((r, cap, 2, I64(-1, 4), I32(4, 5), *good[2:], 30, c), b"reference roll"),
        ((r, cap, 2, *good[:2], I64(9, 9), I32(8, 0), 30, c), b"estimated roll"),      # ends one column past the capacity
        ((r, cap, 2, *good[:2], I64(9, 2 ** 62), I32(7, 0), 30, c), b"estimated roll"),
        ((r, cap, 2, *good, 2 ** 24 + 1, c), b"velocity_threshold"),
        ((r, cap, 2, *good, -2 ** 24 - 1, c), b"velocity_threshold"),
    ]
    for args, word in bad:
        assert _counts(lib, *args) == _lib.MT3_ERR_INVALID, args
        err = lib.mt3_last_error()
        assert err.startswith(b"mt3_op_frame_counts: ") and word in err, err
    assert _counts(lib, r, cap, 0, *good, 30, c) == _lib.MT3_OK                       # zero pairs: a valid no-op
    assert _counts(lib, None, 0, 0, None, None, None, None, 30, None) == _lib.MT3_OK
    assert (rolls == 7.0).all() and (counts == 99).all()


def test_python_surface():
    assert list(inspect.signature(pianoroll.pianorolls).parameters) == ["sequences", "fps", "is_drum"]
    assert list(inspect.signature(pianoroll.frame_counts).parameters) == ["ref_sequences", "est_sequences", "fps",
                                                                          "velocity_threshold", "is_drum"]
    sig = inspect.signature(pianoroll.frame_counts).parameters
    assert (sig["fps"].default, sig["velocity_threshold"].default, sig["is_drum"].default) == (62.5, 30, False)
    assert list(inspect.signature(metrics_utils.get_prettymidi_pianoroll).parameters) == ["ns", "fps", "is_drum"]
    assert list(inspect.signature(metrics_utils.frame_metrics).parameters) == ["ref_pianoroll", "est_pianoroll",
                                                                              "velocity_threshold"]
    assert list(inspect.signature(metrics.frame_scores).parameters) == ["ref_ns", "est_ns", "fps", "velocity_threshold",
                                                                        "is_drum"]
    assert callable(metrics.frame_scores_many) and callable(inference.InferenceModel.pianoroll)
    assert pianoroll.pianorolls([]) == [] and pianoroll.frame_counts([], []).shape == (0, 3)
    assert metrics.frame_scores_many([]) == []


def test_command_line_flag():
    wav = __file__                                     # plan() only checks that the input exists
    assert transcribe.plan(["--checkpoint", "random:0", wav])[0].pianoroll is None
    assert transcribe.plan(["--checkpoint", "random:0", "--pianoroll", "--no-drums", wav])[0].pianoroll == 62.5
    assert transcribe.plan(["--checkpoint", "random:0", "--pianoroll", "100", wav])[0].pianoroll == 100.0
    assert transcribe.pianoroll_path("/x/y/song.mid") == "/x/y/song.npy"
