"""The device PCM decode (mt3_pcm_decode, mt3_resampler_run_pcm, include/mt3_hip.h) against audio_io.read_wav and the
float resampler, bit for bit; audio_io.read_wav_device; InferenceModel.transcribe_wav / transcribe_wavs against the same
model on host-decoded samples; the command line end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, audio_io, checkpoints, inference, midi_io, network, synthetic  # noqa: E402
from tests import pcm_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")
GUARD = 4096
SENTINEL = 12345.0


def _upload(raw, misalign=0):
    """the bytes on the device, `misalign` bytes past an allocation's (aligned) start"""
    host = np.concatenate([np.full(misalign, 0xAA, np.uint8), np.frombuffer(raw, np.uint8)])
    return torch.from_numpy(host).cuda()[misalign:]


def _split(out, n, cap):
    y = out.cpu().numpy()
    return y[:n], y[n:cap], y[cap:]


def _decode(pcm, n, channels, fmt, cap_extra=777):
    """mt3_pcm_decode on torch's current stream into a buffer with GUARD sentinel samples past the capacity"""
    cap = n + cap_extra
    out = torch.full((cap + GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    _lib.check(_lib.load().mt3_pcm_decode(pcm.data_ptr(), n, channels, fmt, out.data_ptr(), cap,
                                          torch.cuda.current_stream().cuda_stream))
    return out, cap


def _run_pcm(pcm, n, channels, fmt, sr, cap_extra=777):
    n_out = audio_io.resampled_length(n, sr)
    cap = n_out + cap_extra
    out = torch.full((cap + GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    _lib.check(_lib.load().mt3_resampler_run_pcm(audio_io._resampler(sr, 16000), pcm.data_ptr(), n, channels, fmt,
                                                 out.data_ptr(), cap, torch.cuda.current_stream().cuda_stream))
    return _split(out, n_out, cap)


def _zero_tail_and_guard(tail, guard):
    return np.array_equal(tail.view(np.int32), np.zeros(len(tail), np.int32)) and bool((guard == SENTINEL).all())


def _host(name, channels, raw, rate=16000):
    """read_wav on a file around the data chunk `raw`"""
    _, tag, bits, _ = pc.FORMATS[name]
    with np.errstate(over="ignore", invalid="ignore"):
        y, sr = audio_io.read_wav(pc.wav_file(rate, channels, tag, bits, raw))
    assert sr == rate
    return y


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("name", sorted(pc.FORMATS))
def test_decode_is_read_wav_bit_for_bit(name, channels):
    fmt = pc.FORMATS[name][0]
    exact_nan = name == "f32" and channels == 1       # a mono float file passes through, NaN payloads included
    side = torch.cuda.Stream()
    for n in (1, 2, 255, 256, 257, 100003):
        raw = pc.samples(name, n, channels, seed=n + channels)
        want = _host(name, channels, raw)
        assert pc.same_samples(pc.decode_numpy(raw, fmt, channels), want, exact_nan)      # the table itself
        pcm = _upload(raw)
        out, cap = _decode(pcm, n, channels, fmt)
        y, tail, guard = _split(out, n, cap)
        assert pc.same_samples(y, want, exact_nan), (name, channels, n)
        assert _zero_tail_and_guard(tail, guard), (name, channels, n)
        side.wait_stream(torch.cuda.current_stream())                                    # the upload is done
        with torch.cuda.stream(side):
            out2, _ = _decode(pcm, n, channels, fmt)
        side.synchronize()
        assert np.array_equal(out2.cpu().numpy().view(np.int32), out.cpu().numpy().view(np.int32)), (name, channels, n)


def test_decode_with_capacity_equal_to_the_length():
    raw = pc.samples("s16", 1000, 2, seed=1)
    y, tail, guard = _split(*_decode(_upload(raw), 1000, 2, _lib.MT3_PCM_S16, cap_extra=0)[:1], 1000, 1000)
    assert pc.same_samples(y, _host("s16", 2, raw)) and len(tail) == 0 and (guard == SENTINEL).all()


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_s24_at_every_byte_alignment(channels):
    n = 10007
    raw = pc.samples("s24", n, channels, seed=24)
    want = _host("s24", channels, raw)
    for misalign in range(4):
        pcm = _upload(raw, misalign)
        assert pcm.data_ptr() % 4 == misalign
        out, cap = _decode(pcm, n, channels, _lib.MT3_PCM_S24)
        y, tail, guard = _split(out, n, cap)
        assert pc.same_samples(y, want), misalign
        assert _zero_tail_and_guard(tail, guard), misalign
        y, tail, guard = _run_pcm(pcm, n, channels, _lib.MT3_PCM_S24, 48000)
        ref = audio_io.resample_device(want, 48000).cpu().numpy()
        assert np.array_equal(y.view(np.int32), ref.view(np.int32)) and _zero_tail_and_guard(tail, guard), misalign


def _audio_like(name, n, channels, seed, sr):
    """finite, audio-shaped data of format `name` as data chunk bytes"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None] / sr
    x = 0.4 * np.sin(2 * np.pi * 440.0 * t + np.arange(channels)) + rng.uniform(-0.5, 0.5, (n, channels))
    if name == "u8":
        return np.rint(x * 127 + 128).astype(np.uint8).tobytes()
    if name == "s16":
        return np.rint(x * 32767).astype("<i2").tobytes()
    if name == "s24":
        v = np.rint(x * (2 ** 23 - 1)).astype(np.int64)
        return (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    assert name == "f32"
    return x.astype("<f4").tobytes()


@pytest.mark.parametrize("sr", [44100, 48000, 22050, 8000, 96000])
@pytest.mark.parametrize("name,channels", [("s16", 2), ("s24", 2), ("f32", 1), ("u8", 1)])
def test_fused_resample_is_the_float_resampler_on_read_wav_bit_for_bit(name, channels, sr):
    fmt = pc.FORMATS[name][0]
    H, up, _ = audio_io.kaiser_best_taps(sr)
    span = -(-len(H) // up)                           # the filter's length in input samples
    for n in (1, 5, span // 2 - 1, 2 * sr + 1):       # the first three are shorter than one tap span
        raw = _audio_like(name, n, channels, seed=n, sr=sr)
        want = _host(name, channels, raw, rate=sr)
        ref = audio_io.resample_device(want, sr).cpu().numpy()
        y, tail, guard = _run_pcm(_upload(raw), n, channels, fmt, sr)
        assert y.shape == ref.shape, (name, sr, n)
        assert np.array_equal(y.view(np.int32), ref.view(np.int32)), (name, sr, n)
        assert _zero_tail_and_guard(tail, guard), (name, sr, n)


def test_fused_resample_on_a_side_stream():
    sr, n = 44100, 3 * 44100
    raw = _audio_like("s16", n, 2, seed=2, sr=sr)
    pcm = _upload(raw)
    y, tail, guard = _run_pcm(pcm, n, 2, _lib.MT3_PCM_S16, sr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y2, tail2, guard2 = _run_pcm(pcm, n, 2, _lib.MT3_PCM_S16, sr)
    assert np.array_equal(y.view(np.int32), y2.view(np.int32)) and _zero_tail_and_guard(tail2, guard2)


@pytest.fixture(scope="module")
def ten_minutes():
    """10 minutes of 44.1 kHz stereo int16 (106 MB), built once: (data chunk bytes, frames)"""
    sr, n = 44100, 600 * 44100
    rng = np.random.default_rng(7)
    mono = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n, dtype=np.float32) / sr) + rng.uniform(-0.4, 0.4, n).astype(np.float32)
    pcm = np.empty((n, 2), "<i2")
    pcm[:, 0] = np.rint(mono * 32767)
    pcm[:, 1] = np.rint(mono * 30000)
    return pcm.tobytes(), n


def test_ten_minutes_of_stereo_int16_in_one_call(ten_minutes):
    """byte offsets reach 1.06e8 and n*down passes 2^31: the index arithmetic is int64 on both sides of the staging"""
    raw, n = ten_minutes
    want = _host("s16", 2, raw, rate=44100)
    ref = audio_io.resample_device(want, 44100).cpu().numpy()
    pcm = _upload(raw)
    y, tail, guard = _run_pcm(pcm, n, 2, _lib.MT3_PCM_S16, 44100)
    assert len(y) == 9600000 and np.array_equal(y.view(np.int32), ref.view(np.int32))
    assert _zero_tail_and_guard(tail, guard)
    out, cap = _decode(pcm, n, 2, _lib.MT3_PCM_S16)
    y, tail, guard = _split(out, n, cap)
    assert pc.same_samples(y, want) and _zero_tail_and_guard(tail, guard)


def test_run_pcm_rejects_a_short_capacity_and_writes_nothing():
    lib = _lib.load()
    r = audio_io._resampler(44100, 16000)
    n_out = audio_io.resampled_length(1000, 44100)
    pcm = _upload(pc.samples("s16", 1000, 2, seed=3))
    y = torch.full((1000,), 7.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.mt3_resampler_run_pcm(r, pcm.data_ptr(), 1000, 2, _lib.MT3_PCM_S16, y.data_ptr(), n_out - 1, s) == _lib.MT3_ERR_INVALID
    assert b"out_capacity" in lib.mt3_last_error()
    assert lib.mt3_pcm_decode(pcm.data_ptr(), 1000, 2, _lib.MT3_PCM_S16, y.data_ptr(), 999, s) == _lib.MT3_ERR_INVALID
    assert lib.mt3_resampler_run_pcm(r, pcm.data_ptr(), 1000, 8, _lib.MT3_PCM_S16, y.data_ptr(), 1000, s) == _lib.MT3_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def _ordered(a):
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.mark.parametrize("sr", [44100, 48000, 8000])
def test_the_float_resampler_is_where_it_was(sr):
    """mt3_resampler_run shares its kernel with the PCM path now: still the host resample within one ulp
    (tests/test_gpu_resample.py's rule)"""
    x = np.random.default_rng(sr).uniform(-1, 1, 3 * sr + 17).astype(np.float32)
    ref = audio_io.resample(x, sr)
    y = audio_io.resample_device(x, sr).cpu().numpy()
    u = np.abs(_ordered(y) - _ordered(ref))
    assert y.shape == ref.shape and u.max() <= 1 and (u > 0).sum() <= max(1, len(ref) // 100000)


# ------------------------------------------------------------------ read_wav_device
def _wav(name, channels, sr, raw, **kw):
    _, tag, bits, _ = pc.FORMATS[name]
    return pc.wav_file(sr, channels, tag, bits, raw, **kw)


@pytest.mark.parametrize("sr", [16000, 44100])
def test_read_wav_device_on_a_path_and_on_bytes(tmp_path, sr):
    n = 2 * sr + 11
    wav = _wav("s24", 2, sr, _audio_like("s24", n, 2, seed=5, sr=sr), before=[pc.chunk(b"LIST", b"INFOabc")])
    path = tmp_path / "x.wav"
    path.write_bytes(wav)
    y, native = audio_io.read_wav(wav)
    ref = audio_io.resample_device(y, native, capacity=len(y) + 500).cpu().numpy()
    for arg in (wav, bytearray(wav), str(path), path):
        out, rate, n_out = audio_io.read_wav_device(arg, capacity=len(y) + 500)
        assert rate == sr and n_out == audio_io.resampled_length(n, sr) and out.is_cuda and out.dtype == torch.float32
        assert np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32))
    out, _, n_out = audio_io.read_wav_device(wav)
    assert out.shape == (n_out,) and np.array_equal(out.cpu().numpy().view(np.int32), ref[:n_out].view(np.int32))
    with pytest.raises(ValueError):
        audio_io.read_wav_device(wav, capacity=n_out - 1)


def test_read_wav_device_falls_back_to_the_host_decode():
    sr, n = 44100, 44100
    s24 = _audio_like("s24", n, 2, seed=6, sr=sr)
    files = {"8 channels": _wav("s16", 8, sr, _audio_like("s16", n, 8, seed=6, sr=sr)),
             "20-bit": pc.wav_file(sr, 2, 1, 20, s24, block_align=6)}
    for what, wav in files.items():
        assert audio_io.wav_info(wav) is None, what
        y, native = audio_io.read_wav(wav)
        out, rate, n_out = audio_io.read_wav_device(wav)
        assert (rate, n_out) == (sr, 16000), what
        assert np.array_equal(out.cpu().numpy().view(np.int32), audio_io.resample_device(y, native).cpu().numpy().view(np.int32))


# ------------------------------------------------------------------ InferenceModel.transcribe_wav / transcribe_wavs
def _tuples(ns):
    return [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, n.instrument) for n in ns.notes]


def _tokens_and_times(m, make_examples):
    examples, x = make_examples()
    return x.cpu().numpy(), m.predict_tokens({"encoder_input_tokens": x}), [ex["input_times"] for ex in examples]


def _three_files(y16):
    """a 16 kHz mono int16 file, a 44.1 kHz stereo int16 file and a 48 kHz 24-bit stereo file of the same music"""
    y16 = np.clip(np.asarray(y16, np.float64), -1.0, 1.0)
    y44 = np.clip(audio_io.resample(y16.astype(np.float32), 16000, 44100), -1.0, 1.0).astype(np.float64)
    y48 = np.clip(audio_io.resample(y16.astype(np.float32), 16000, 48000), -1.0, 1.0).astype(np.float64)
    s16 = np.rint(y16 * 32767).astype("<i2").tobytes()
    st44 = np.rint(np.stack([y44, 0.9 * y44], 1) * 32767).astype("<i2").tobytes()
    v = np.rint(np.stack([0.9 * y48, y48], 1) * (2 ** 23 - 1)).astype(np.int64)
    st48 = (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    return [_wav("s16", 1, 16000, s16), _wav("s16", 2, 44100, st44), _wav("s24", 2, 48000, st48, extensible=True)]


def _check_wav_equals_host_decode(m, wavs):
    singles = []
    for wav in wavs:
        assert audio_io.wav_info(wav) is not None
        y, sr = audio_io.read_wav(wav)
        lm_a, tok_a, times_a = _tokens_and_times(m, lambda: m._wav_examples(wav))
        lm_b, tok_b, times_b = _tokens_and_times(m, lambda: m._examples(y, sr))
        assert np.array_equal(lm_a.view(np.int32), lm_b.view(np.int32))       # the same samples reached the frontend
        assert len(times_a) == len(times_b) and all(np.array_equal(a, b) for a, b in zip(times_a, times_b))
        assert np.array_equal(tok_a, tok_b)
        notes = _tuples(m.transcribe_wav(wav))
        assert notes == _tuples(m(y, sample_rate=sr))
        assert len(notes) >= 5
        singles.append(notes)
    decoded = [audio_io.read_wav(wav) for wav in wavs]
    assert [_tuples(ns) for ns in m.transcribe_wavs(wavs)] == singles
    assert [_tuples(ns) for ns in m.transcribe_many([y for y, _ in decoded], sample_rates=[sr for _, sr in decoded])] == singles
    assert m.transcribe_wavs([]) == []
    return singles


@pytest.fixture(scope="module")
def trained_files():
    _, y16 = synthetic.synth_music(3 * 2.048 + 0.7, seed=21, device="cpu")
    return _three_files(y16)


def test_transcribe_wav_on_the_trained_fixture(trained_files, tmp_path):
    m = inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32")
    singles = _check_wav_equals_host_decode(m, trained_files)
    path = tmp_path / "b.wav"
    path.write_bytes(trained_files[1])
    assert _tuples(m.transcribe_wav(str(path))) == singles[1]
    # files the device path does not take go through read_wav on the host and transcribe all the same
    sr, n = 44100, 3 * 44100
    for wav in (_wav("s16", 8, sr, _audio_like("s16", n, 8, seed=8, sr=sr)),
                pc.wav_file(sr, 2, 1, 20, _audio_like("s24", n, 2, seed=8, sr=sr), block_align=6)):
        assert audio_io.wav_info(wav) is None
        assert _tuples(m.transcribe_wav(wav)) == _tuples(m(*audio_io.read_wav(wav)))
    with pytest.raises(ValueError):
        m.transcribe_wav(b"RIFF\x04\0\0\0JUNK")       # scipy's error, as read_wav raises it


def test_transcribe_wav_ismir2021_preset():
    """T = 512 segments, boosted random weights (as tests/test_gpu_resample.py does)"""
    cfg = network.T5Config(dtype="float32", vocab_size=1664, num_encoder_layers=2, num_decoder_layers=2)
    params = synthetic.boost_note_events(network.init_random_params(cfg, seed=1, norm_scale_jitter=0.1),
                                         num_velocity_bins=127, eos=3.0, tie=1.0, velocity=2.0)
    m = inference.InferenceModel(params, "ismir2021", config=cfg)
    y16 = synthetic.synth_audio(3, seed=0, device="cpu", seg_samples=512 * 128).reshape(-1)[: 2 * 512 * 128 + 9000].numpy()
    _check_wav_equals_host_decode(m, _three_files(y16))


def test_command_line_end_to_end(trained_files, tmp_path):
    a, b = tmp_path / "first.wav", tmp_path / "second.wav"
    a.write_bytes(trained_files[1])
    b.write_bytes(trained_files[2])
    out = tmp_path / "midi"
    r = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", CKPT, "-o", str(out), str(a), str(b)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = inference.InferenceModel(CKPT, "mt3")
    for ns, name in zip(m.transcribe_wavs([str(a), str(b)]), ("first.mid", "second.mid")):
        want = midi_io.note_sequence_to_midi_bytes(ns)
        got = (out / name).read_bytes()
        assert len(ns.notes) >= 5 and got == want
        assert _tuples(midi_io.midi_bytes_to_note_sequence(got)) == _tuples(midi_io.midi_bytes_to_note_sequence(want))
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"not a wav file at all")
    r = subprocess.run([sys.executable, "-m", "mt3_amd.transcribe", "--checkpoint", "random:0", str(bad)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "ValueError" in r.stderr and not (tmp_path / "bad.mid").exists()
