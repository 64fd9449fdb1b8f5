"""mt3_op_render_notes on a box without a GPU: the symbol and its prototype, and every argument check of
include/mt3_hip.h -- all of which come before any HIP call, so the "device" pointers here are host memory that must come
back untouched -- then the Python surface and the command line's flag.  No CUDA call in this file."""
import ctypes as C
import inspect

import numpy as np
import pytest

from mt3_amd import _lib, inference, metrics_utils, render, transcribe
from mt3_amd.note_sequences import Note, NoteSequence

I64 = lambda *v: np.array(v, np.int64)          # noqa: E731


def test_symbol_is_exported_and_typed():
    lib = _lib.load()
    _P = C.c_void_p
    assert _lib.SIGNATURES["mt3_op_render_notes"] == (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, _P,
                                                                C.c_int32, C.c_int32, _P, C.c_int64, _P, _P])
    fn = lib.mt3_op_render_notes
    assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES["mt3_op_render_notes"][1]
    assert lib.mt3_abi_version() == 4
    assert (render.TILE, render.MAX_SAMPLE_RATE, render.RELEASE_SECONDS, render.DRUM_SECONDS) == (1024, 384000, 0.04, 0.15)


class _Job:
    """a well-formed two-sequence call on host memory; `call(name=value)` swaps one argument"""

    def __init__(self):
        self.notes = np.zeros(64, np.float64)
        self.out = np.full(4096, 7.0, np.float32)
        self.peaks = np.full(2, 5.0, np.float32)
        p = self.notes.ctypes.data
        self.args = dict(d_start=p, d_end=p, d_reach=p, d_pitch=p, d_velocity=p, d_is_drum=p, n_notes=6, n_seq=2,
                         note_offsets=I64(0, 2, 6), sample_offsets=I64(10, 1500), n_samples=I64(1000, 2000),
                         sample_rate=16000, normalize=1, d_out=self.out.ctypes.data, out_capacity=4096,
                         d_peaks=self.peaks.ctypes.data, stream=None)

    def call(self, **swap):
        a = dict(self.args, **swap)
        self.keep = a
        tab = lambda v: None if v is None else v.ctypes.data        # noqa: E731
        return _lib.load().mt3_op_render_notes(a["d_start"], a["d_end"], a["d_reach"], a["d_pitch"], a["d_velocity"],
                                               a["d_is_drum"], a["n_notes"], a["n_seq"], tab(a["note_offsets"]),
                                               tab(a["sample_offsets"]), tab(a["n_samples"]), a["sample_rate"],
                                               a["normalize"], a["d_out"], a["out_capacity"], a["d_peaks"], a["stream"])

    def untouched(self):
        return (self.out == 7.0).all() and (self.peaks == 5.0).all() and not self.notes.any()


def test_rejects_bad_arguments_before_any_device_call():
    lib, job = _lib.load(), _Job()
    bad = [
        (dict(n_seq=-1), b"n_seq"),
        (dict(n_notes=-1), b"n_notes"),
        (dict(sample_rate=0), b"sample_rate"), (dict(sample_rate=-16000), b"sample_rate"),
        (dict(sample_rate=384001), b"sample_rate"),
        (dict(note_offsets=None), b"null table"), (dict(sample_offsets=None), b"null table"),
        (dict(n_samples=None), b"null table"),
        (dict(d_start=None), b"null note array"), (dict(d_end=None), b"null note array"),
        (dict(d_reach=None), b"null note array"), (dict(d_pitch=None), b"null note array"),
        (dict(d_velocity=None), b"null note array"), (dict(d_is_drum=None), b"null note array"),
        (dict(d_out=None), b"null d_out"),
        (dict(d_peaks=None), b"null d_peaks"),
        (dict(note_offsets=I64(0, 4, 3)), b"must not decrease"),
        (dict(note_offsets=I64(-1, 2, 6)), b"inside [0, n_notes]"),
        (dict(note_offsets=I64(0, 2, 7)), b"inside [0, n_notes]"),
        (dict(note_offsets=I64(0, 2 ** 31, 2 ** 31), n_notes=2 ** 31), b"2^31 - 1 notes"),
        (dict(n_samples=I64(1000, -1)), b"h_n_samples"),
        (dict(n_samples=I64(1000, 2 ** 40 + 1), out_capacity=2 ** 62), b"h_n_samples"),
        (dict(sample_offsets=I64(-1, 1500)), b"sample offset"),
        (dict(sample_offsets=I64(10, 2 ** 62)), b"sample offset"),
        (dict(sample_offsets=I64(10, 1009)), b"overlap"),           # sequence 1 starts inside sequence 0
        (dict(sample_offsets=I64(2000, 10)), b"overlap"),           # out of order
        (dict(out_capacity=3499), b"out_capacity"),                 # one float short
        (dict(out_capacity=-1), b"out_capacity"),
    ]
    for swap, word in bad:
        assert job.call(**swap) == _lib.MT3_ERR_INVALID, swap
        err = lib.mt3_last_error()
        assert err.startswith(b"mt3_op_render_notes: ") and word in err, (swap, err)
    assert job.untouched()                                          # host memory: nothing may have touched it


def test_calls_that_do_nothing_succeed():
    job = _Job()
    assert job.call(n_seq=0) == _lib.MT3_OK
    assert job.call(n_seq=0, n_notes=0, note_offsets=None, sample_offsets=None, n_samples=None, d_start=None, d_end=None,
                    d_reach=None, d_pitch=None, d_velocity=None, d_is_drum=None, d_out=None, out_capacity=0,
                    d_peaks=None) == _lib.MT3_OK
    # sequences that are all empty: nothing to write, so no buffer is needed and no device either
    assert job.call(n_samples=I64(0, 0), d_out=None, d_peaks=None, out_capacity=1500) == _lib.MT3_OK
    assert job.untouched()


def _ns(*notes):
    return NoteSequence(notes=[Note(*n) for n in notes])


def test_python_surface():
    assert list(inspect.signature(render.render).parameters) == ["sequences", "sample_rate", "lengths", "normalize"]
    sig = inspect.signature(render.render).parameters
    assert (sig["sample_rate"].default, sig["lengths"].default, sig["normalize"].default) == (16000, None, True)
    assert list(inspect.signature(render.render_wav_data).parameters) == ["ns", "sample_rate"]
    assert list(inspect.signature(inference.InferenceModel.render).parameters) == ["ns", "sample_rate"]
    assert inspect.signature(inference.InferenceModel.render).parameters["sample_rate"].default == 16000
    assert render.render([]) == []


def test_render_length_is_the_one_length_function():
    f, i = (lambda *v: np.array(v, np.float64)), (lambda *v: np.array(v, np.int64))
    assert render.render_length(f(), f(), i()) == 0
    assert render.render_length(f(1.0), f(1.01), i(1)) == 18400     # a drum note: start + 0.15 whatever its end
    assert render.render_length(f(1.0), f(1.01), i(0)) == 16800
    assert render.render_length(f(0.0, 1.0), f(1.2, 1.01), i(0, 1)) == 19840
    assert render.render_length(f(0.0), f(0.10003), i(0)) == 2241
    assert render.render_length(f(0.0), f(1.0), i(0), 44100) == 45864
    assert render.sounding_instants(f(1.0, 2.0), f(1.5, 9.0), i(0, 1)).tolist() == [1.54, 2.15]


def test_value_errors_come_before_any_upload():
    """on a box without a GPU an upload would raise something else: each of these must be the ValueError"""
    good = (0.0, 1.0, 60, 100)
    for notes, word in [([(0.0, 1.0, 128, 100)], "pitches"), ([(0.0, 1.0, -1, 100)], "pitches"),
                        ([(0.0, 1.0, 60, 128)], "velocities"), ([(0.0, 1.0, 60, -1)], "velocities"),
                        ([(-0.5, 1.0, 60, 100)], "finite and not negative"),
                        ([(0.0, float("inf"), 60, 100)], "finite and not negative"),
                        ([(float("nan"), 1.0, 60, 100)], "finite and not negative"),
                        ([(1.0, 0.5, 60, 100)], "ends before")]:
        with pytest.raises(ValueError, match=word):
            render.render([_ns(good), _ns(good, *notes)])
    for rate in (0, -1, 384001, 16000.5, float("nan")):
        with pytest.raises(ValueError, match="sample_rate"):
            render.render([_ns(good)], rate)
        with pytest.raises(ValueError, match="sample_rate"):
            render.render_wav_data(_ns(good), rate)
    with pytest.raises(ValueError, match="lengths"):
        render.render([_ns(good)], lengths=[10, 10])
    with pytest.raises(ValueError, match="samples"):
        render.render([_ns(good)], lengths=[-1])
    rec = np.zeros(1, metrics_utils.NOTE_DTYPE)                     # the record form is checked the same way
    rec[0] = (0.0, 1.0, 200, 100, 0, False, 0, 0)
    with pytest.raises(ValueError, match="pitches"):
        render.render([rec])


def test_packing_sorts_and_builds_the_running_reach():
    ns = _ns((2.0, 2.1, 60, 100), (0.0, 5.0, 50, 90), (1.0, 1.2, 38, 80, 0, True), (0.0, 5.0, 40, 90), (2.0, 2.1, 60, 99))
    packed, n, offs, n_samples = render._pack([NoteSequence(), ns], 16000, None)
    assert n == 5 and offs.tolist() == [0, 0, 5] and n_samples.tolist() == [0, 80640]
    f8 = packed[:8 * 15].view("<f8").reshape(3, 5)
    i4 = packed[8 * 15:].view("<i4").reshape(3, 5)
    assert f8[0].tolist() == [0.0, 0.0, 1.0, 2.0, 2.0] and f8[1].tolist() == [5.0, 5.0, 1.2, 2.1, 2.1]
    assert f8[2].tolist() == [5.04] * 5                             # the running maximum of the sounding instants
    assert i4[0].tolist() == [40, 50, 38, 60, 60] and i4[1].tolist() == [90, 90, 80, 99, 100] and i4[2].tolist() == [0, 0, 1, 0, 0]
    assert render._pack([ns], 16000, [123])[3].tolist() == [123]


def test_command_line_flag():
    wav = __file__                                     # plan() only checks that the input exists
    assert transcribe.plan(["--checkpoint", "random:0", wav])[0].render is None
    assert transcribe.plan(["--checkpoint", "random:0", "--render", "--no-drums", wav])[0].render == 16000
    assert transcribe.plan(["--checkpoint", "random:0", "--render", "44100", wav])[0].render == 44100
    both = transcribe.plan(["--checkpoint", "random:0", "--render", "--pianoroll", "100", "--well-formed", wav])[0]
    assert (both.render, both.pianoroll, both.well_formed) == (16000, 100.0, True)
    for rate in ("0", "384001"):
        with pytest.raises(SystemExit):
            transcribe.plan(["--checkpoint", "random:0", "--render", rate, wav])
    assert transcribe.render_path("/x/y/song.mid") == "/x/y/song.render.wav"
