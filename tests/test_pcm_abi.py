"""The device PCM decode's C ABI on a box without a GPU (mt3_pcm_decode / mt3_resampler_run_pcm argument checks, which all
come before any HIP call), the RIFF parser that decides which files take the device path (audio_io.wav_info) against
scipy.io.wavfile.read, the kernels' arithmetic restated in numpy (tests/pcm_cases.decode_numpy) against audio_io.read_wav
bit for bit, and the command line's argument handling.  No CUDA call in this file."""
import ctypes as C
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from mt3_amd import _lib, audio_io, transcribe
from tests import pcm_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_typed():
    lib = _lib.load()
    for name in ("mt3_pcm_decode", "mt3_resampler_run_pcm"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mt3_abi_version() == 4
    assert (_lib.MT3_PCM_U8, _lib.MT3_PCM_S16, _lib.MT3_PCM_S24, _lib.MT3_PCM_S32, _lib.MT3_PCM_F32,
            _lib.MT3_PCM_F64) == (0, 1, 2, 3, 4, 5)


def _bad_pcm_arguments(p):
    """(d_pcm, n_frames, channels, format, d_out, word of the message) for every MT3_ERR_INVALID case the two entries share"""
    return [
        (None, 8, 2, _lib.MT3_PCM_S16, p, b"null"),
        (p, 8, 2, _lib.MT3_PCM_S16, None, b"null"),
        (p, 0, 2, _lib.MT3_PCM_S16, p, b"n_frames"),
        (p, -3, 2, _lib.MT3_PCM_S16, p, b"n_frames"),
        (p, 8, 0, _lib.MT3_PCM_S16, p, b"channels"),
        (p, 8, 8, _lib.MT3_PCM_S16, p, b"channels"),
        (p, 8, 2, -1, p, b"format"),
        (p, 8, 2, _lib.MT3_PCM_F64 + 1, p, b"format"),
        (p, 2 ** 62, 1, _lib.MT3_PCM_U8, p, b"too large"),
    ]


def test_pcm_decode_rejects_bad_arguments_before_any_device_call():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for d_pcm, n, ch, fmt, d_out, msg in _bad_pcm_arguments(p):
        assert lib.mt3_pcm_decode(d_pcm, n, ch, fmt, d_out, 64, None) == _lib.MT3_ERR_INVALID, (n, ch, fmt)
        err = lib.mt3_last_error()
        assert b"mt3_pcm_decode" in err and msg in err, err
    assert lib.mt3_pcm_decode(p, 8, 2, _lib.MT3_PCM_S16, p, 7, None) == _lib.MT3_ERR_INVALID      # capacity one short
    assert b"out_capacity" in lib.mt3_last_error()
    assert lib.mt3_pcm_decode(p, 8, 2, _lib.MT3_PCM_S16, p, -1, None) == _lib.MT3_ERR_INVALID
    assert not any(buf)                               # host memory here: nothing may have touched it


def test_resampler_run_pcm_rejects_bad_arguments_before_any_device_call():
    """a resampler cannot be created without a GPU, so the handle is NULL throughout: the sample arguments are checked
    first and the handle last.  out_capacity one short needs a real handle: tests/test_gpu_pcm.py."""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for d_pcm, n, ch, fmt, d_out, msg in _bad_pcm_arguments(p):
        assert lib.mt3_resampler_run_pcm(None, d_pcm, n, ch, fmt, d_out, 64, None) == _lib.MT3_ERR_INVALID, (n, ch, fmt)
        err = lib.mt3_last_error()
        assert b"mt3_resampler_run_pcm" in err and msg in err, err
    assert lib.mt3_resampler_run_pcm(None, p, 8, 2, _lib.MT3_PCM_S16, p, 64, None) == _lib.MT3_ERR_INVALID
    assert b"null resampler" in lib.mt3_last_error()


# ------------------------------------------------------------------ wav_info and the arithmetic against scipy
def _scipy(wav):
    from scipy.io import wavfile
    with warnings.catch_warnings():
        warnings.simplefilter("error")                # a file the device path takes must read without a warning
        return wavfile.read(io.BytesIO(wav))


def _check_accepted(wav, name, rate, channels, exact_nan=False):
    fmt = pc.FORMATS[name][0]
    info = audio_io.wav_info(wav)
    assert info is not None, name
    sr, data = _scipy(wav)
    assert (info.sample_rate, info.channels, info.format) == (sr, channels, fmt) and sr == rate
    assert info.frames == data.shape[0] and (data.ndim == 1) == (channels == 1)
    raw = wav[info.data_offset: info.data_offset + info.data_bytes]
    assert len(raw) == info.data_bytes == info.frames * channels * pc.FORMATS[name][2] // 8
    with np.errstate(over="ignore", invalid="ignore"):
        want, sr2 = audio_io.read_wav(wav)
    assert sr2 == rate
    assert pc.same_samples(pc.decode_numpy(raw, fmt, channels), want, exact_nan=exact_nan), (name, channels)
    return info


@pytest.mark.parametrize("channels", [1, 2, 3, 7])
@pytest.mark.parametrize("name", ["u8", "s16", "s32", "f32", "f64"])
def test_wav_info_and_arithmetic_on_scipy_written_files(name, channels):
    from scipy.io import wavfile
    n = 4099
    raw = pc.samples(name, n, channels, seed=channels)
    x = np.frombuffer(raw, pc.FORMATS[name][3]).reshape(n, channels)
    buf = io.BytesIO()
    wavfile.write(buf, 22050, x[:, 0] if channels == 1 else x)
    info = _check_accepted(buf.getvalue(), name, 22050, channels, exact_nan=(name == "f32" and channels == 1))
    assert info.frames == n


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("name", sorted(pc.FORMATS))
def test_wav_info_and_arithmetic_on_hand_packed_files(name, channels):
    """every format x channel count, 24-bit included; an odd frame count makes odd-sized data chunks"""
    _, tag, bits, _ = pc.FORMATS[name]
    n = 2053
    wav = pc.wav_file(48000, channels, tag, bits, pc.samples(name, n, channels, seed=10 + channels))
    assert _check_accepted(wav, name, 48000, channels, exact_nan=(name == "f32" and channels == 1)).frames == n


def test_wav_info_skips_the_chunks_scipy_skips():
    payload = pc.samples("s24", 777, 2, seed=1)
    cases = {
        "extensible pcm": pc.wav_file(44100, 2, 1, 24, payload, extensible=True),
        "odd LIST before data": pc.wav_file(44100, 2, 1, 24, payload, before=[pc.chunk(b"LIST", b"INFOabc")]),
        "fact": pc.wav_file(44100, 2, 1, 24, payload, before=[pc.chunk(b"fact", b"\x09\x03\x00\x00")]),
        "JUNK, fact, LIST, and a LIST after data": pc.wav_file(
            44100, 2, 1, 24, payload, before=[pc.chunk(b"JUNK", b"\0" * 27), pc.chunk(b"fact", b"\0" * 4),
                                             pc.chunk(b"LIST", b"x" * 5)], after=[pc.chunk(b"LIST", b"INFOxyz")]),
    }
    for what, wav in cases.items():
        info = _check_accepted(wav, "s24", 44100, 2)
        assert info.frames == 777, what
    fl = pc.samples("f32", 500, 3, seed=2)
    _check_accepted(pc.wav_file(96000, 3, 3, 32, fl, extensible=True, before=[pc.chunk(b"fact", b"\0" * 4)]), "f32", 96000, 3)
    _check_accepted(pc.wav_file(8000, 1, 3, 64, pc.samples("f64", 500, 1, seed=3), extensible=True), "f64", 8000, 1)
    # bytes trailing the RIFF size are ignored by scipy and by the parser alike
    _check_accepted(pc.wav_file(44100, 2, 1, 24, payload) + b"trailing garbage", "s24", 44100, 2)


def _rejected_files():
    s16 = pc.samples("s16", 1000, 2, seed=4)
    whole = pc.wav_file(44100, 2, 1, 16, s16)
    assert len(whole) == 44 + 4000
    cut = {"data chunk cut by %d" % k: whole[: len(whole) - k] for k in (1, 2, 3, 4)}
    return dict(cut, **{
        "RIFX": pc.wav_file(44100, 2, 1, 16, s16, magic=b"RIFX"),
        "RF64 magic": pc.wav_file(44100, 2, 1, 16, s16, magic=b"RF64"),
        "20-bit": pc.wav_file(44100, 2, 1, 20, pc.samples("s24", 1000, 2, seed=5), block_align=6),
        "12-bit": pc.wav_file(44100, 1, 1, 12, s16, block_align=2),
        "64-bit integer": pc.wav_file(44100, 1, 1, 64, pc.samples("f64", 100, 1, seed=6)),
        "16-bit float": pc.wav_file(44100, 1, 3, 16, s16),
        "8 channels": pc.wav_file(44100, 8, 1, 16, pc.samples("s16", 1000, 8, seed=7)),
        "0 channels": pc.wav_file(44100, 0, 1, 16, s16, block_align=2),
        "data size larger than the file": pc.wav_file(44100, 2, 1, 16, s16, data_size=4004),
        "half a frame at the end": pc.wav_file(44100, 2, 1, 16, s16[:-2]),
        "zero frames": pc.wav_file(44100, 2, 1, 16, b""),
        "no fmt chunk": pc.wav_file(44100, 2, 1, 16, s16, fmt=False),
        "block_align does not match": pc.wav_file(44100, 2, 1, 16, s16, block_align=8),
        "byte rate does not match": pc.wav_file(44100, 2, 1, 16, s16, byte_rate=12345),
        "mu-law": pc.wav_file(8000, 1, 7, 8, s16),
        "a chunk scipy warns about": pc.wav_file(44100, 2, 1, 16, s16, before=[pc.chunk(b"bext", b"\0" * 10)]),
        "a second data chunk": pc.wav_file(44100, 2, 1, 16, s16, after=[pc.chunk(b"data", s16[:400])]),
        "not RIFF": b"OggS" + whole[4:],
        "not WAVE": whole[:8] + b"AVI " + whole[12:],
        "eleven bytes": whole[:11],
        "empty": b"",
    })


def test_wav_info_rejects_what_the_device_path_does_not_cover():
    for what, wav in _rejected_files().items():
        assert audio_io.wav_info(wav) is None, what
    assert audio_io.wav_info(io.BytesIO(pc.wav_file(44100, 2, 1, 16, b"\0" * 400))) is None       # an open file object


def test_wav_info_reads_a_path_like_the_bytes(tmp_path):
    wav = pc.wav_file(32000, 2, 1, 24, pc.samples("s24", 321, 2, seed=8), before=[pc.chunk(b"LIST", b"abc")])
    path = tmp_path / "x.wav"
    path.write_bytes(wav)
    assert audio_io.wav_info(str(path)) == audio_io.wav_info(wav) == audio_io.wav_info(path) == audio_io.wav_info(bytearray(wav))
    (tmp_path / "cut.wav").write_bytes(wav[:-3])
    assert audio_io.wav_info(str(tmp_path / "cut.wav")) is None


class _Stop(Exception):
    pass


def test_read_wav_device_falls_back_exactly_when_wav_info_says_none(monkeypatch):
    """the fallback decision without a GPU: read_wav_device consults wav_info, and goes to read_wav + resample_device
    when (and only when) it returns None"""
    calls = []
    real_info = audio_io.wav_info

    def info(wav):
        calls.append("wav_info")
        return real_info(wav)

    def host_decode(wav):
        calls.append("read_wav")
        return np.zeros(10, np.float32), 44100

    def device_resample(y, sr, target, capacity=None):
        calls.append("resample_device")
        return "resampled"

    def upload(wav, i):
        calls.append("upload")
        raise _Stop()

    monkeypatch.setattr(audio_io, "wav_info", info)
    monkeypatch.setattr(audio_io, "read_wav", host_decode)
    monkeypatch.setattr(audio_io, "resample_device", device_resample)
    monkeypatch.setattr(audio_io, "_upload_chunk", upload)
    monkeypatch.setattr(audio_io, "_resampler", lambda a, b: "resampler")
    for what, wav in _rejected_files().items():
        del calls[:]
        out, sr, n_out = audio_io.read_wav_device(wav)
        assert calls == ["wav_info", "read_wav", "resample_device"], what
        assert (out, sr, n_out) == ("resampled", 44100, audio_io.resampled_length(10, 44100))
    for rate in (44100, 16000):
        del calls[:]
        with pytest.raises(_Stop):
            audio_io.read_wav_device(pc.wav_file(rate, 2, 1, 16, pc.samples("s16", 100, 2, seed=9)))
        assert calls == ["wav_info", "upload"]
    monkeypatch.undo()
    with pytest.raises(ValueError):                   # more than 2^20 taps: refused before anything is uploaded
        audio_io.read_wav_device(pc.wav_file(44101, 1, 1, 16, pc.samples("s16", 100, 1, seed=9)))
    with pytest.raises(ValueError):
        audio_io.read_wav_device(pc.wav_file(44100, 1, 1, 16, pc.samples("s16", 441, 1, seed=9)), capacity=159)


# ------------------------------------------------------------------ the command line (no model is built)
def test_command_line_plans_its_outputs(tmp_path, capsys):
    a, b = tmp_path / "a.wav", tmp_path / "sub" / "b.wav"
    (tmp_path / "sub").mkdir()
    wav = pc.wav_file(16000, 1, 1, 16, b"\0" * 64)
    a.write_bytes(wav)
    b.write_bytes(wav)
    args, outs = transcribe.plan(["--checkpoint", "random:0", str(a), str(b)])
    assert outs == [str(tmp_path / "a.mid"), str(tmp_path / "sub" / "b.mid")]
    assert (args.model, args.dtype, args.checkpoint) == ("mt3", "float32", "random:0")
    out_dir = tmp_path / "out"
    _, outs = transcribe.plan(["--checkpoint", "x.npz", "--model", "ismir2021", "-o", str(out_dir), str(a), str(b)])
    assert outs == [str(out_dir / "a.mid"), str(out_dir / "b.mid")]
    _, outs = transcribe.plan(["--checkpoint", "x.npz", "-o", str(tmp_path / "one.mid"), str(a)])
    assert outs == [str(tmp_path / "one.mid")]
    _, outs = transcribe.plan(["--checkpoint", "x.npz", "-o", str(tmp_path / "sub"), str(a)])       # an existing directory
    assert outs == [str(tmp_path / "sub" / "a.mid")]
    bad = [
        (["--checkpoint", "x.npz", str(a), str(tmp_path / "missing.wav")], "no such file"),
        (["--checkpoint", "x.npz", "-o", str(a), str(a), str(b)], "need a directory"),              # -o is a file
        (["--checkpoint", "x.npz", "-o", str(out_dir), str(a), str(a)], "same output"),
        ([str(a)], "--checkpoint"),
        (["--checkpoint", "x.npz"], "IN.wav"),
    ]
    for argv, msg in bad:
        with pytest.raises(SystemExit) as e:
            transcribe.plan(argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, argv
    assert not out_dir.exists()                       # planning creates nothing


def test_command_line_exits_non_zero_on_a_missing_file(tmp_path):
    r = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", "random:0", str(tmp_path / "nope.wav")],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "no such file" in r.stderr
