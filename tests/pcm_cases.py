"""Shared by tests/test_pcm_abi.py and tests/test_gpu_pcm.py: WAV files packed by hand, sample data for every MT3_PCM_*
format, and the PCM decode + mixdown of include/mt3_hip.h restated in plain numpy (`decode_numpy`), which is the CPU
statement of what the kernels compute."""
import struct

import numpy as np

from mt3_amd import _lib

FORMATS = {                                       # name: (MT3_PCM_*, format tag, bits, numpy dtype of a wavfile.write array)
    "u8": (_lib.MT3_PCM_U8, 1, 8, np.uint8),
    "s16": (_lib.MT3_PCM_S16, 1, 16, np.int16),
    "s24": (_lib.MT3_PCM_S24, 1, 24, None),       # scipy cannot write it: hand-packed only
    "s32": (_lib.MT3_PCM_S32, 1, 32, np.int32),
    "f32": (_lib.MT3_PCM_F32, 3, 32, np.float32),
    "f64": (_lib.MT3_PCM_F64, 3, 64, np.float64),
}
GUID_TAIL = bytes.fromhex("000010008000" "00aa00389b71")


def chunk(ck_id: bytes, body: bytes) -> bytes:
    return ck_id + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def wav_file(rate, channels, tag, bits, payload, *, extensible=False, before=(), after=(), magic=b"RIFF",
             block_align=None, byte_rate=None, data_size=None, fmt=True):
    """a RIFF/WAVE file around `payload` (the data chunk's bytes); the keyword arguments bend the header"""
    block_align = channels * bits // 8 if block_align is None else block_align
    byte_rate = rate * block_align if byte_rate is None else byte_rate
    if extensible:
        body = struct.pack("<HHIIHH", 0xFFFE, channels, rate, byte_rate, block_align, bits) + \
            struct.pack("<HHI", 22, bits, 0) + struct.pack("<I", tag) + GUID_TAIL
    else:
        body = struct.pack("<HHIIHH", tag, channels, rate, byte_rate, block_align, bits)
    chunks = (chunk(b"fmt ", body) if fmt else b"") + b"".join(before)
    data = b"data" + struct.pack("<I", len(payload) if data_size is None else data_size) + payload + \
        (b"\0" if len(payload) & 1 else b"")
    rest = chunks + data + b"".join(after)
    return magic + struct.pack("<I", 4 + len(rest)) + b"WAVE" + rest


def samples(name, n, channels, seed):
    """[n, channels] sample data of format `name` as the bytes of a data chunk: random values plus the format's corner
    values (extremes, zeros of both signs, infinities, NaNs, subnormals, values that round on the way to float32)"""
    rng = np.random.default_rng(seed)
    count = n * channels
    if name == "u8":
        v = rng.integers(0, 256, count).astype(np.uint8)
        v[:3] = [0, 255, 128][: min(3, count)]
        return v.tobytes()
    if name == "s16":
        v = rng.integers(-2 ** 15, 2 ** 15, count).astype("<i2")
        v[:3] = [-2 ** 15, 2 ** 15 - 1, 0][: min(3, count)]
        return v.tobytes()
    if name == "s24":
        v = rng.integers(-2 ** 23, 2 ** 23, count).astype(np.int64)
        v[:3] = [-2 ** 23, 2 ** 23 - 1, -1][: min(3, count)]
        return (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    if name == "s32":
        v = rng.integers(-2 ** 31, 2 ** 31, count).astype("<i4")          # most need rounding to 24 bits
        v[:5] = [-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 25) - 2][: min(5, count)]      # ties to even
        return v.tobytes()
    v = rng.standard_normal(count) * 10.0 ** rng.integers(-3, 3, count)
    special = [-0.0, np.inf, -np.inf, np.nan, 1e-40, -3e-45, 3.0e38, 0.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e300, 1e-300]
    at = rng.permutation(count)[: len(special)]
    v[at] = special[: len(at)]
    with np.errstate(over="ignore"):
        return v.astype("<f4" if name == "f32" else "<f8").tobytes()


def decode_numpy(raw: bytes, fmt: int, channels: int) -> np.ndarray:
    """include/mt3_hip.h's table and mixdown, literally: data chunk bytes -> mono float32"""
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        if fmt == _lib.MT3_PCM_U8:
            s = (np.frombuffer(raw, np.uint8).astype(f32) - f32(128)) / f32(128)
        elif fmt == _lib.MT3_PCM_S16:
            s = np.frombuffer(raw, "<i2").astype(f32) / f32(2 ** 15)
        elif fmt == _lib.MT3_PCM_S24:
            b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.uint32)
            v32 = (b[:, 0] << 8 | b[:, 1] << 16 | b[:, 2] << 24).astype(np.uint32).view(np.int32)
            s = v32.astype(f32) / f32(2 ** 31)
        elif fmt == _lib.MT3_PCM_S32:
            s = np.frombuffer(raw, "<i4").astype(f32) / f32(2 ** 31)
        elif fmt == _lib.MT3_PCM_F32:
            s = np.frombuffer(raw, "<f4").copy()
        elif fmt == _lib.MT3_PCM_F64:
            s = np.frombuffer(raw, "<f8").astype(f32)
        else:
            raise ValueError(fmt)
        s = s.reshape(-1, channels)
        if channels == 1:
            return s[:, 0]
        acc = np.zeros(len(s), f32)
        for c in range(channels):
            acc = (acc + s[:, c]).astype(f32)
        return (acc / f32(channels)).astype(f32)


def same_samples(got, want, exact_nan=False):
    """bit equality of two float32 arrays; NaNs compare as NaN-where-NaN unless exact_nan"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    g, w = got.view(np.uint32), want.view(np.uint32)
    if exact_nan:
        return bool(np.array_equal(g, w))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(g[~nan], w[~nan]))
