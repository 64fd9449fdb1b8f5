"""The device resampler's C ABI on a box without a GPU (mt3_resample_output_length, mt3_resampler_create / _run argument
checks, which all come before any HIP call), and the host side of the ingest it shares a filter with: kaiser_best_taps,
resample, read_wav."""
import ctypes as C
import io

import numpy as np
import pytest

from mt3_amd import _lib, audio_io


def _n_out_scipy(n_in, up, down):
    # scipy.signal.resample_poly: n_out = n_in * up // down + bool(n_in * up % down)
    return n_in * up // down + bool(n_in * up % down)


def test_symbols_are_exported_and_typed():
    lib = _lib.load()
    for name in ("mt3_resample_output_length", "mt3_resampler_create", "mt3_resampler_destroy", "mt3_resampler_run"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mt3_abi_version() == 4


def test_output_length_equals_scipys_n_out():
    lib = _lib.load()
    rng = np.random.default_rng(0)
    pairs = [(160, 441), (1, 3), (2, 3), (1, 2), (320, 441), (640, 441), (2, 1), (1, 6), (1, 12), (80, 441), (1, 1)]
    lengths = [1, 2, 7, 440, 441, 442, 28224, 56449, 26460000, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 33 + 5, 10 ** 12]
    lengths += [int(v) for v in rng.integers(1, 2 ** 40, 50)]
    for up, down in pairs + [(int(u), int(d)) for u, d in rng.integers(1, 2 ** 20, (30, 2))]:
        for n in lengths:
            assert lib.mt3_resample_output_length(n, up, down) == _n_out_scipy(n, up, down), (n, up, down)
            assert audio_io.resampled_length(n, 1, 1) == n
    for sr in (8000, 11025, 44100, 48000, 96000):
        up, down = audio_io.rate_ratio(sr)
        for n in (1, 7, 44100, 2 ** 31 + 3):
            assert audio_io.resampled_length(n, sr) == _n_out_scipy(n, up, down)
    assert lib.mt3_resample_output_length(-1, 1, 2) == -1
    assert lib.mt3_resample_output_length(5, 0, 2) == -1
    assert lib.mt3_resample_output_length(5, 2, 0) == -1


def _create(h, n_taps, up, down, out=True):
    lib = _lib.load()
    r = C.c_void_p()
    hp = h.ctypes.data if h is not None else None
    return lib.mt3_resampler_create(hp, n_taps, up, down, C.byref(r) if out else None)


def test_create_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    h = np.ones(2 ** 20 + 3, np.float64)
    bad = [
        (None, 5, 1, 2, True, b"null"),                      # NULL taps
        (h, 5, 1, 2, False, b"null"),                        # NULL out
        (h, 4, 1, 2, True, b"odd"),                          # even
        (h, 0, 1, 2, True, b"odd"),                          # zero
        (h, -3, 1, 2, True, b"odd"),                         # negative
        (h, 2 ** 20 + 1, 1, 2, True, b"2^20"),               # too many taps
        (h, 5, 0, 2, True, b">= 1"),                         # up < 1
        (h, 5, 1, 0, True, b">= 1"),                         # down < 1
        (h, 5, -160, 441, True, b">= 1"),
        (h, 5, 2, 4, True, b"gcd"),                          # not in lowest terms
        (h, 5, 320, 882, True, b"gcd"),
    ]
    for args in bad:
        *a, msg = args
        assert _create(*a) == _lib.MT3_ERR_INVALID, args[1:5]
        err = lib.mt3_last_error()
        assert b"mt3_resampler_create" in err and msg in err, err


def test_run_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    # the resampler handle itself is checked first: a NULL one is an error whatever the other arguments are
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.mt3_resampler_run(None, p, 8, p, 16, None) == _lib.MT3_ERR_INVALID
    assert b"mt3_resampler_run" in lib.mt3_last_error() and b"null" in lib.mt3_last_error()
    lib.mt3_resampler_destroy(None)                          # a no-op


@pytest.mark.parametrize("sr", [8000, 11025, 22050, 44100, 48000, 96000])
def test_taps_are_the_table_resample_applies(sr):
    from scipy.signal import resample_poly
    H, up, down = audio_io.kaiser_best_taps(sr)
    w, up2, down2 = audio_io.kaiser_best_window(sr)
    assert (up, down) == (up2, down2) == audio_io.rate_ratio(sr)
    assert H.dtype == np.float64 and len(H) % 2 == 1 and len(H) == audio_io.kaiser_best_num_taps(sr)
    assert np.array_equal(H, w * up)
    x = np.random.default_rng(sr).standard_normal(3001).astype(np.float32)
    got = audio_io.resample(x, sr)
    assert np.array_equal(got.view(np.int32), resample_poly(x.astype(np.float64), up, down, window=w).astype(np.float32).view(np.int32))
    # the kernel's formula, summed directly in float64: y[n] = sum_k x[k] H[n*down + half - k*up]
    half = (len(H) - 1) // 2
    n_out = audio_io.resampled_length(len(x), sr)
    assert n_out == len(got)
    xd = x.astype(np.float64)
    for n in list(range(5)) + list(range(n_out - 5, n_out)) + [n_out // 2]:
        k = np.arange(len(x))
        idx = n * down + half - k * up
        ok = (idx >= 0) & (idx < len(H))
        assert np.float32(np.sum(xd[ok] * H[idx[ok]])) == got[n]


def test_rates_over_the_tap_limit_are_rejected():
    assert audio_io.kaiser_best_num_taps(44101) > audio_io.MAX_DEVICE_TAPS
    with pytest.raises(ValueError):
        audio_io._resampler(44101, 16000)
    for sr in (8000, 11025, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000):
        assert audio_io.kaiser_best_num_taps(sr) <= audio_io.MAX_DEVICE_TAPS


@pytest.mark.parametrize("sr,dtype,channels", [(44100, np.int16, 2), (48000, np.int16, 1), (16000, np.int16, 1),
                                               (22050, np.uint8, 2), (8000, np.float32, 1), (11025, np.int32, 2)])
def test_read_wav_plus_resample_is_wav_data_to_samples(sr, dtype, channels):
    from scipy.io import wavfile
    rng = np.random.default_rng(sr)
    x = rng.uniform(-0.9, 0.9, (sr // 3, channels))
    if dtype == np.uint8:
        pcm = (x * 127 + 128).astype(np.uint8)
    elif dtype == np.float32:
        pcm = x.astype(np.float32)
    else:
        pcm = (x * np.iinfo(dtype).max).astype(dtype)
    buf = io.BytesIO()
    wavfile.write(buf, sr, pcm[:, 0] if channels == 1 else pcm)
    data = buf.getvalue()
    y, native = audio_io.read_wav(data)
    assert native == sr and y.dtype == np.float32 and y.shape == (sr // 3,)
    ref = audio_io.wav_data_to_samples(data)
    assert np.array_equal(audio_io.resample(y, native).view(np.int32), ref.view(np.int32))
