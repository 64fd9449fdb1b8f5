"""The case tables of tests/test_gpu_frontend_forms.py (tests/frontend_cases.py) through the CPU emulation of the
frontend kernel's lane program (tests/host/frontend_emul.cpp: the same frontend_core.h / frontend_tables.h, g++), against
the numpy oracle at the same bounds.  Shows without a GPU that the chosen inputs stay inside the bounds, that the periodic
construction gives bit-identical rows per overhang class, that samples past the count are not read, and that the
emulation's log keeps the kernel's rule for non-finite samples."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import frontend_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emul_forms") / "libfrontend_emul.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "mt3_amd", "csrc"), os.path.join(ROOT, "tests", "host", "frontend_emul.cpp"),
                           "-o", out])
    return ctypes.CDLL(out)


def run_batch(lib, audio, counts):
    """[S, F * 128] -> [S, F, 512] on the product's default (float32-built) tables, one emulated segment at a time"""
    audio = np.ascontiguousarray(audio, np.float32)
    S, frames = audio.shape[0], audio.shape[1] // fc.HOP
    out = np.full((S, frames, fc.MEL), 7.0, np.float32)
    for s in range(S):
        assert lib.emul_logmel(audio[s].ctypes.data_as(ctypes.c_void_p), int(counts[s]), frames,
                               out[s].ctypes.data_as(ctypes.c_void_p), 1) == 0
    return out


@pytest.mark.parametrize("frames", fc.SEGMENT_FRAMES)
def test_shapes_counts_and_poison(emul, frames):
    audio, counts = fc.shape_batch(frames)
    out = run_batch(emul, audio, counts)
    fc.check_shape_batch(frames, out)
    for value in (0.0, np.nan, 3e38):
        np.testing.assert_array_equal(run_batch(emul, fc.poisoned(audio, counts, value), counts), out)


@pytest.mark.parametrize("length", fc.ODD_LENGTHS)
def test_lengths_that_are_no_multiple_of_the_hop(emul, length):
    x, padded = fc.odd_length_samples(length)
    n = len(padded) // fc.HOP
    frames = max(16, -(-n // 16) * 16)                         # spectrograms.compute_spectrogram's launch
    buf = np.zeros((1, frames * fc.HOP), np.float32)
    buf[0, :length] = x
    fc.check_segment(run_batch(emul, buf, [n])[0], ("odd", length), padded, n, f"{length} samples")


@pytest.mark.parametrize("frames", sorted(fc.PERIODIC))
def test_periodic_rows_are_identical(emul, frames):
    audio, counts = fc.periodic_batch(frames)
    fc.check_periodic(frames, run_batch(emul, audio, counts))


def test_int16_scale_stays_inside_the_bounds_with_libm_log(emul):
    """the scale batch at 2^15: with logf (about half an ulp) the lane program keeps the oracle's bounds at int16 scale,
    so what the GPU file adds there is the kernel's own log (safe_log_fast on v_log_f32)"""
    audio, counts = fc.scale_batch()
    scaled = audio * np.float32(2.0 ** 15)
    out = run_batch(emul, scaled, counts)
    for s, n in enumerate(counts):
        fc.check_segment(out[s], ("scale", 15, s), scaled[s], n, f"2^15 segment {s}")


def test_nonfinite_samples(emul):
    bad, clean = fc.nonfinite_batches()
    fc.check_nonfinite(run_batch(emul, bad, fc.NONFINITE_COUNTS), run_batch(emul, clean, fc.NONFINITE_COUNTS))


def test_the_checks_notice_wrong_counts_and_wrong_rows(emul):
    """the failure modes the GPU file targets, tried on the emulation: one count for every segment, a row swapped with
    its neighbour's"""
    audio, counts = fc.shape_batch(32)
    with pytest.raises(AssertionError):
        fc.check_shape_batch(32, run_batch(emul, audio, [counts[0]] * len(counts)))
    audio, counts = fc.periodic_batch(64)
    out = run_batch(emul, audio, counts)
    out[2, 40] = out[2, 41]                                    # overhang 8 where overhang 7 belongs (n = 49)
    with pytest.raises(AssertionError):
        fc.check_periodic(64, out)
