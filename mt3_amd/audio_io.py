"""Audio ingest: WAV bytes/file -> mono float32 at 16 kHz.

The notebook uses `note_seq.audio_io.wav_data_to_samples_librosa` and `librosa.resample`
(mt3/preprocessors.py:139-144); neither is available here.  This module decodes PCM WAV with the
standard library / scipy and resamples by band-limited sinc interpolation with resampy's
"kaiser_best" filter -- librosa's default `res_type` in the releases of the reference's time --
evaluated exactly on the polyphase grid (`resample(..., res_type="kaiser_best")`, the default since
round 6).  Filter parameters are from memory of resampy: PARITY UNPINNED against librosa itself
(inputs already at 16 kHz are bit-identical, no filter runs).

What the choice of filter is worth, MEASURED (tests/test_io_and_metrics.py::test_resampling_filters_measured,
44.1 kHz -> 16 kHz): scipy's default polyphase low-pass (`res_type="polyphase"`, rounds 3-5's ingest:
Kaiser(5.0), 10 zero crossings a side, cut-off AT the new Nyquist rate) passes a 8.2 kHz tone at
-8.7 dB and a 9 kHz tone at -30.6 dB -- they alias to 7.8 / 7.0 kHz, inside the mel range (20 Hz ..
7.6 kHz, mt3/spectrograms.py:27-28) -- where kaiser_best is below -150 dB from 8.2 kHz on; kaiser_best
in turn rolls off earlier (-3.1 dB at 7.5 kHz, -22.6 dB at 7.8 kHz; polyphase -1.8 / -4.0 dB).  Both are
flat to 0.01 dB up to 7 kHz.  On a fixture with partials up to 20 kHz the two 16 kHz signals differ at
29.7 dB SNR and their log-mels by up to 5.7 (natural log; mean 0.07) -- aliased partials in the upper mel
bands -- so the filter is NOT a detail for material with energy above 8 kHz.  On band-limited material
(five steady partials up to 6 kHz) the partials themselves (mel > 0.1) agree to 0.004 in the log-mel; the
floor between them (mel 1e-3 .. 1e-1, 40-70 dB below the partials) still moves by up to 1.8: that is the
polyphase filter's -66 dB stop band, not a property of the material.
"""
from __future__ import annotations

import collections
import io
import struct
import warnings
from fractions import Fraction

import numpy as np

SAMPLE_RATE = 16000


def read_wav(wav_data):
    """bytes or path -> (float32 mono in [-1, 1], native sample rate): the PCM decode and stereo mixdown of
    `wav_data_to_samples`, without the resample."""
    from scipy.io import wavfile
    src = io.BytesIO(wav_data) if isinstance(wav_data, (bytes, bytearray)) else wav_data
    native_sr, y = wavfile.read(src)
    if y.dtype == np.uint8:
        y = (y.astype(np.float32) - 128.0) / 128.0
    elif np.issubdtype(y.dtype, np.integer):
        y = y.astype(np.float32) / float(np.iinfo(y.dtype).max + 1)
    else:
        y = y.astype(np.float32)
    if y.ndim == 2:
        y = y.mean(axis=1)
    return y, int(native_sr)


def wav_data_to_samples(wav_data, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """bytes or path -> float32 mono in [-1, 1] at `sample_rate` (`read_wav` + host `resample`)."""
    y, native_sr = read_wav(wav_data)
    return resample(y, native_sr, sample_rate)


# resampy's "kaiser_best" filter, which `librosa.resample` / `librosa.load` used by default in the librosa releases of the
# reference's time (res_type='kaiser_best'; mt3/preprocessors.py:139-144, NB:165) [parameters from memory of resampy's
# published filter: a Kaiser-windowed sinc with 64 zero crossings, beta 14.7697, roll-off 0.9476 of the lower Nyquist rate]
KAISER_BEST = {"num_zeros": 64, "beta": 14.769656459379492, "rolloff": 0.9475937167399596}


def kaiser_sinc_kernel(tau: np.ndarray, scale: float, num_zeros: int, beta: float, rolloff: float) -> np.ndarray:
    """g(tau), tau in INPUT samples: y(t) = sum_n x[n] g(t - n).  scale = min(1, target_sr / orig_sr) stretches the filter
    when downsampling (and carries the gain): g = scale * rolloff * sinc(rolloff * scale * tau) * kaiser(scale * |tau| / zeros)."""
    t = scale * np.abs(np.asarray(tau, np.float64))
    inside = t <= num_zeros
    taper = np.i0(beta * np.sqrt(np.clip(1.0 - (t / num_zeros) ** 2, 0.0, 1.0))) / np.i0(beta)
    return np.where(inside, scale * rolloff * np.sinc(rolloff * t) * taper, 0.0)


def rate_ratio(orig_sr: int, target_sr: int = SAMPLE_RATE):
    """(up, down) in lowest terms: target_sr / orig_sr."""
    frac = Fraction(int(target_sr), int(orig_sr))
    return frac.numerator, frac.denominator


def kaiser_best_num_taps(orig_sr: int, target_sr: int = SAMPLE_RATE) -> int:
    """Length 2*half + 1 of the kaiser_best table for this rate pair (without building it)."""
    up, down = rate_ratio(orig_sr, target_sr)
    return 2 * int(np.ceil(KAISER_BEST["num_zeros"] / min(1.0, up / down) * up)) + 1


def kaiser_best_window(orig_sr: int, target_sr: int = SAMPLE_RATE):
    """(w, up, down): the FIR `resample(..., "kaiser_best")` hands to scipy.signal.resample_poly as `window`."""
    up, down = rate_ratio(orig_sr, target_sr)
    scale = min(1.0, up / down)
    half = int(np.ceil(KAISER_BEST["num_zeros"] / scale * up))              # taps each side at the up-sampled rate
    k = np.arange(-half, half + 1)
    return kaiser_sinc_kernel(k / up, scale, **KAISER_BEST) / up, up, down    # (resample_poly multiplies the filter by `up`)


def kaiser_best_taps(orig_sr: int, target_sr: int = SAMPLE_RATE):
    """(H, up, down): H = w * up in float64, the table resample_poly actually applies (and mt3_resampler_create takes):
    y[n] = sum_k x[k] H[n*down + half - k*up], n < ceil(len(x) * up / down)."""
    w, up, down = kaiser_best_window(orig_sr, target_sr)
    return w * up, up, down


def resample(y: np.ndarray, orig_sr: int, target_sr: int = SAMPLE_RATE, res_type: str = "kaiser_best") -> np.ndarray:
    """res_type: "polyphase" = scipy.signal.resample_poly's own Kaiser(5.0) low-pass of 20 x max(up, down) + 1
    taps; "kaiser_best" (default) = the band-limited sinc interpolation of resampy's kaiser_best filter (see KAISER_BEST), evaluated
    EXACTLY on the polyphase grid (resampy itself interpolates a 512-per-zero-crossing table linearly: ~1e-6 relative).
    Measured difference between the two on a 44.1 kHz fixture and its effect on the log-mel: module docstring,
    tests/test_io_and_metrics.py::test_resampling_filters_measured.  The device counterpart is `resample_device`."""
    if orig_sr == target_sr:
        return np.ascontiguousarray(y, np.float32)
    from scipy.signal import resample_poly
    if res_type == "polyphase":
        up, down = rate_ratio(orig_sr, target_sr)
        return resample_poly(y.astype(np.float64), up, down).astype(np.float32)
    if res_type != "kaiser_best":
        raise ValueError("res_type must be 'polyphase' or 'kaiser_best'")
    w, up, down = kaiser_best_window(orig_sr, target_sr)
    return resample_poly(y.astype(np.float64), up, down, window=w).astype(np.float32)


# ------------------------------------------------------------------ device resample (mt3_resampler_*)
MAX_DEVICE_TAPS = 1 << 20                    # mt3_resampler_create's limit
_resamplers = {}


def resampled_length(n_in: int, orig_sr: int, target_sr: int = SAMPLE_RATE) -> int:
    """ceil(n_in * up / down): the number of samples `resample` / `resample_device` produce."""
    if orig_sr == target_sr:
        return int(n_in)
    up, down = rate_ratio(orig_sr, target_sr)
    return -(-int(n_in) * up // down)


def _resampler(orig_sr: int, target_sr: int):
    """one mt3_resampler per rate pair (kaiser_best taps), created on first use"""
    key = (int(orig_sr), int(target_sr))
    if key not in _resamplers:
        import ctypes as C
        from . import _lib
        n_taps = kaiser_best_num_taps(orig_sr, target_sr)
        if n_taps > MAX_DEVICE_TAPS:
            raise ValueError("resample_device: %d Hz -> %d Hz needs a %d-tap filter; the device resampler takes at most "
                             "2^20 taps" % (orig_sr, target_sr, n_taps))
        h, up, down = kaiser_best_taps(orig_sr, target_sr)
        h = np.ascontiguousarray(h, np.float64)
        r = C.c_void_p()
        lib = _lib.load()
        rc = lib.mt3_resampler_create(h.ctypes.data, len(h), up, down, C.byref(r))
        if rc == _lib.MT3_ERR_INVALID:
            raise ValueError(lib.mt3_last_error().decode("utf-8", "replace"))
        _lib.check(rc)
        _resamplers[key] = r
    return _resamplers[key]


def resample_device(x, orig_sr: int, target_sr: int = SAMPLE_RATE, capacity: int = None):
    """`resample(x, orig_sr, target_sr)` on the GPU (mt3_resampler_run: the same kaiser_best table, summed in float64).
    x: float32 1-d torch tensor (CUDA or host) or numpy array.  Returns a CUDA float32 tensor of `capacity` samples
    (default: the resampled length) with zeros after the resampled length.  The work is stream-ordered on torch's
    current stream; equal rates copy x without running a kernel.  A rate pair whose table exceeds 2^20 taps raises
    ValueError."""
    import torch
    from . import _lib
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if t.dim() != 1 or t.dtype != torch.float32:
        raise ValueError("resample_device: x must be a 1-d float32 tensor or array")
    n_out = resampled_length(t.shape[0], orig_sr, target_sr)
    capacity = n_out if capacity is None else int(capacity)
    if capacity < n_out:
        raise ValueError("resample_device: capacity %d < %d output samples" % (capacity, n_out))
    if orig_sr == target_sr:
        out = torch.zeros(capacity, device="cuda", dtype=torch.float32)
        out[:n_out].copy_(t)
        return out
    if t.shape[0] < 1:
        raise ValueError("resample_device: empty input")
    r = _resampler(orig_sr, target_sr)
    t = t.to(device="cuda").contiguous()
    out = torch.empty(capacity, device="cuda", dtype=torch.float32)
    _lib.check(_lib.load().mt3_resampler_run(r, t.data_ptr(), t.shape[0], out.data_ptr(), capacity,
                                             torch.cuda.current_stream().cuda_stream))
    return out


# ------------------------------------------------------------------ device decode (mt3_pcm_decode, mt3_resampler_run_pcm)
WavInfo = collections.namedtuple("WavInfo", "sample_rate channels format data_offset data_bytes frames")
_SILENT_CHUNKS = (b"fact", b"LIST", b"JUNK", b"Fake")        # what scipy.io.wavfile.read skips without a warning
_GUID_TAIL = b"\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"      # {XXXXXXXX-0000-0010-8000-00AA00389B71}


def _open_wav(wav_data):
    return io.BytesIO(wav_data) if isinstance(wav_data, (bytes, bytearray, memoryview)) else open(wav_data, "rb")


def wav_info(wav_data):
    """bytes or path -> WavInfo(sample_rate, channels, MT3_PCM_* format, data_offset, data_bytes, frames) when the
    device decode gives `read_wav`'s samples for this file, else None (the caller then calls `read_wav`, with scipy's
    errors and warnings).  Standard library only; reads the chunk headers, not the samples.

    Accepted: little-endian RIFF/WAVE whose chunks up to the RIFF size are one `fmt `, one `data` after it, and
    `fact` / `LIST` / `JUNK` / `Fake` chunks (scipy skips those silently; any other chunk makes it warn), all of them
    wholly inside the file; format tag 1 (PCM: 8, 16, 24 or 32 bits), 3 (IEEE float: 32 or 64 bits) or 0xFFFE with one
    of those as sub-format; block_align == channels * bits / 8; 1 .. 7 channels; a data chunk of a whole number of
    frames, at least one.  Rejected, among others: RIFX, RF64, 12- and 20-bit samples, 64-bit integers, 8 or more
    channels, truncated files, a PCM header whose byte rate is not rate * block_align (scipy raises on it)."""
    from . import _lib
    if hasattr(wav_data, "read"):                     # an open file object: scipy's business
        return None
    with _open_wav(wav_data) as f:
        size = f.seek(0, 2)
        f.seek(0)
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:] != b"WAVE":
            return None
        riff_end = struct.unpack("<I", head[4:8])[0] + 8
        fmt = data = None
        pos = 12
        while pos < riff_end:                         # scipy's loop: `while fid.tell() < file_size`
            f.seek(pos)
            ck = f.read(8)
            if len(ck) < 8:
                return None                           # scipy: raises, or warns once it has the data
            n = struct.unpack("<I", ck[4:])[0]
            if pos + 8 + n > size:
                return None
            if ck[:4] == b"fmt ":
                if fmt is not None or data is not None or n < 16:
                    return None
                fmt = f.read(min(n, 40))
            elif ck[:4] == b"data":
                if fmt is None or data is not None:
                    return None
                data = (pos + 8, n)
            elif ck[:4] not in _SILENT_CHUNKS:
                return None
            pos += 8 + n + (n & 1)                    # chunks are padded to an even size
    if fmt is None or data is None:
        return None
    tag, channels, rate, byte_rate, block_align, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE:                                 # WAVE_FORMAT_EXTENSIBLE: cbSize, valid bits, mask, sub-format GUID
        if len(fmt) < 40 or struct.unpack("<H", fmt[16:18])[0] < 22 or fmt[28:40] != _GUID_TAIL:
            return None
        tag = struct.unpack("<I", fmt[24:28])[0]
    if tag == 1:
        if byte_rate != rate * block_align:
            return None
        pcm = {8: _lib.MT3_PCM_U8, 16: _lib.MT3_PCM_S16, 24: _lib.MT3_PCM_S24, 32: _lib.MT3_PCM_S32}.get(bits)
    elif tag == 3:
        pcm = {32: _lib.MT3_PCM_F32, 64: _lib.MT3_PCM_F64}.get(bits)
    else:
        return None
    if pcm is None or rate < 1 or not 1 <= channels <= _lib.PCM_MAX_CHANNELS or block_align != channels * bits // 8:
        return None
    offset, nbytes = data
    if nbytes < block_align or nbytes % block_align:
        return None
    return WavInfo(int(rate), int(channels), pcm, offset, nbytes, nbytes // block_align)


def _upload_chunk(wav_data, info):
    """the data chunk's bytes as a CUDA uint8 tensor: one copy out of the caller's buffer, or one read of that part of
    the file, then the upload"""
    import torch
    if isinstance(wav_data, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(wav_data, np.uint8, info.data_bytes, info.data_offset)
        with warnings.catch_warnings():               # torch warns that a view of `bytes` is read-only; it is only read
            warnings.simplefilter("ignore", UserWarning)
            host = torch.from_numpy(raw)
    else:
        host = torch.from_numpy(np.fromfile(wav_data, np.uint8, info.data_bytes, offset=info.data_offset))
    if host.numel() != info.data_bytes:
        raise ValueError("read_wav_device: the file changed while it was read")
    return host.to(device="cuda")


def read_wav_device(wav_data, target_sr: int = SAMPLE_RATE, capacity: int = None):
    """bytes or path -> (CUDA float32 tensor of `capacity` samples at `target_sr`, zeros after the resampled length;
    native sample rate; resampled length): `read_wav` + `resample_device` with the PCM decode and the channel mixdown
    on the GPU as well.  Only the file's data chunk is uploaded, as it is, and ONE kernel runs on torch's current
    stream: mt3_pcm_decode at equal rates, mt3_resampler_run_pcm otherwise (the same bits as the host decode followed
    by `resample_device`).  A file `wav_info` does not take (RIFX, 20-bit samples, 8 or more channels, a truncated
    chunk, ...) goes through `read_wav` on the host instead, with its errors and warnings.  capacity defaults to the
    resampled length.  A rate pair whose filter exceeds 2^20 taps raises ValueError."""
    import torch
    from . import _lib
    info = wav_info(wav_data)
    if info is None:
        y, native_sr = read_wav(wav_data)
        n_out = resampled_length(len(y), native_sr, target_sr)
        return resample_device(y, native_sr, target_sr, capacity=capacity), native_sr, n_out
    n_out = resampled_length(info.frames, info.sample_rate, target_sr)
    capacity = n_out if capacity is None else int(capacity)
    if capacity < n_out:
        raise ValueError("read_wav_device: capacity %d < %d output samples" % (capacity, n_out))
    r = None if info.sample_rate == target_sr else _resampler(info.sample_rate, target_sr)     # ValueError before the upload
    pcm = _upload_chunk(wav_data, info)
    out = torch.empty(capacity, device="cuda", dtype=torch.float32)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    if r is None:
        _lib.check(lib.mt3_pcm_decode(pcm.data_ptr(), info.frames, info.channels, info.format, out.data_ptr(), capacity,
                                      stream))
    else:
        _lib.check(lib.mt3_resampler_run_pcm(r, pcm.data_ptr(), info.frames, info.channels, info.format, out.data_ptr(),
                                             capacity, stream))
    return out, info.sample_rate, n_out


def samples_to_wav_data(samples: np.ndarray, sample_rate: int = SAMPLE_RATE) -> bytes:
    from scipy.io import wavfile
    buf = io.BytesIO()
    wavfile.write(buf, sample_rate, (np.clip(samples, -1, 1) * 32767.0).astype(np.int16))
    return buf.getvalue()
