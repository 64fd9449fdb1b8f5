"""The device resampler (mt3_resampler_run, include/mt3_hip.h) against the host ingest's audio_io.resample, and
InferenceModel at native sample rates against the same model on host-resampled 16 kHz samples."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, audio_io, checkpoints, inference, network, synthetic  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 192000]
GUARD = 4096
SENTINEL = 12345.0


def _ordered(a):
    """f32 bits on a line where adjacent floats differ by 1 (+0 and -0 both 0)"""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return np.abs(_ordered(a) - _ordered(b))


def _run(x, sr, cap_extra=777):
    """the kernel straight through the ABI into a buffer with GUARD sentinel samples past the capacity"""
    lib = _lib.load()
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    n_out = audio_io.resampled_length(len(x), sr)
    cap = n_out + cap_extra
    out = torch.full((cap + GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.mt3_resampler_run(audio_io._resampler(sr, 16000), xd.data_ptr(), len(x), out.data_ptr(), cap, s))
    y = out.cpu().numpy()
    return y[:n_out], y[n_out:cap], y[cap:]


def _inputs(sr):
    H, up, _ = audio_io.kaiser_best_taps(sr)
    half_in = -(-len(H) // up) // 2                  # half the filter's length in input samples
    lengths = sorted({1, 7, half_in - 1, half_in, half_in + 1, sr, 10 * sr})
    rng = np.random.default_rng(sr)
    for n in lengths:
        t = np.arange(n) / sr
        imp = np.zeros(n, np.float32)
        imp[0] = 1.0
        imp[-1] = -0.75
        yield "noise", n, rng.uniform(-1, 1, n).astype(np.float32)
        yield "tones", n, (0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.3 * np.sin(2 * np.pi * 7321.5 * t + 1)
                           + 0.2 * np.sin(2 * np.pi * 0.45 * sr * t)).astype(np.float32)
        yield "impulses", n, imp


@pytest.mark.parametrize("sr", RATES)
def test_kernel_matches_host_resample(sr):
    differing, total = 0, 0
    for kind, n, x in _inputs(sr):
        ref = audio_io.resample(x, sr)
        y, tail, guard = _run(x, sr)
        assert y.shape == ref.shape, (kind, n)
        u = _ulps(y, ref)
        assert u.max() <= 1, (kind, n, int(u.max()))
        differing += int((u > 0).sum())
        total += len(ref)
        assert np.array_equal(tail.view(np.int32), np.zeros_like(tail).view(np.int32)), (kind, n)   # +0.0 exactly
        assert (guard == SENTINEL).all(), (kind, n)
    print("%d Hz: %d of %d samples differ from the host by one ulp" % (sr, differing, total))
    assert differing <= max(1, total // 100000)


def test_resample_device_api():
    x = np.random.default_rng(3).uniform(-1, 1, 44100 * 3).astype(np.float32)
    ref = audio_io.resample(x, 44100)
    for arg in (x, torch.from_numpy(x), torch.from_numpy(x).cuda()):
        y = audio_io.resample_device(arg, 44100)
        assert y.is_cuda and y.dtype == torch.float32 and y.shape == (len(ref),)
        assert _ulps(y.cpu().numpy(), ref).max() <= 1
    y = audio_io.resample_device(x, 44100, capacity=len(ref) + 100).cpu().numpy()
    assert _ulps(y[:len(ref)], ref).max() <= 1 and not y[len(ref):].any()
    y = audio_io.resample_device(x[:16000], 16000, capacity=16500).cpu().numpy()      # equal rates: a copy
    assert np.array_equal(y[:16000], x[:16000]) and not y[16000:].any()
    with pytest.raises(ValueError):
        audio_io.resample_device(x, 44100, capacity=len(ref) - 1)
    with pytest.raises(ValueError):
        audio_io.resample_device(x, 44101)


def test_run_rejects_bad_sizes_and_writes_nothing():
    lib = _lib.load()
    r = audio_io._resampler(44100, 16000)
    up, down = audio_io.rate_ratio(44100)
    x = torch.ones(1000, device="cuda")
    y = torch.full((1000,), 7.0, device="cuda")
    n_out = lib.mt3_resample_output_length(1000, up, down)
    s = torch.cuda.current_stream().cuda_stream
    for args, msg in (((None, 1000, y.data_ptr(), 1000), b"null"), ((x.data_ptr(), 1000, None, 1000), b"null"),
                      ((x.data_ptr(), 0, y.data_ptr(), 1000), b"n_in"), ((x.data_ptr(), -5, y.data_ptr(), 1000), b"n_in"),
                      ((x.data_ptr(), 1000, y.data_ptr(), n_out - 1), b"out_capacity")):
        assert lib.mt3_resampler_run(r, args[0], args[1], args[2], args[3], s) == _lib.MT3_ERR_INVALID
        assert msg in lib.mt3_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_ten_minutes_at_44k1_in_one_call():
    """n*down passes 2^31 after about 5 minutes of output: the kernel's index arithmetic is int64"""
    sr = 44100
    n = 600 * sr
    rng = np.random.default_rng(7)
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr) + rng.uniform(-0.4, 0.4, n)).astype(np.float32)
    ref = audio_io.resample(x, sr)
    y, tail, guard = _run(x, sr)
    assert len(y) * audio_io.rate_ratio(sr)[1] > 2 ** 31
    u = _ulps(y, ref)
    print("10 min at 44.1 kHz: %d of %d samples differ by one ulp" % (int((u > 0).sum()), len(ref)))
    assert u.max() <= 1 and (u > 0).sum() <= len(ref) // 100000
    assert not tail.any() and (guard == SENTINEL).all()


def test_non_default_stream_without_host_sync():
    sr = 48000
    x = np.random.default_rng(11).uniform(-1, 1, 20 * sr).astype(np.float32)
    ref = audio_io.resample(x, sr)
    xh = torch.from_numpy(x).pin_memory()
    yh = torch.empty(len(ref), dtype=torch.float32).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd = xh.to("cuda", non_blocking=True)
        y = audio_io.resample_device(xd, sr)
        yh.copy_(y, non_blocking=True)
    s.synchronize()
    assert _ulps(yh.numpy(), ref).max() <= 1
    assert np.array_equal(yh.numpy().view(np.int32), _run(x, sr)[0].view(np.int32))     # the same bits as on the default stream


# ------------------------------------------------------------------ InferenceModel at native rates
def _tuples(ns):
    return [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, n.instrument) for n in ns.notes]


def _tokens_and_times(m, audio, sr):
    examples, x = m._examples(audio, sr)
    logmel = x.cpu().numpy()
    return logmel, m.predict_tokens({"encoder_input_tokens": x}), [ex["input_times"] for ex in examples]


def _native(y16, sr):
    """a 'native' file: the 16 kHz samples host-resampled up to sr"""
    return audio_io.resample(y16, 16000, sr)


def _check_native_equals_host(m, y_native, sr):
    y16 = audio_io.resample(y_native, sr)
    lm_a, tok_a, times_a = _tokens_and_times(m, y_native, sr)
    lm_b, tok_b, times_b = _tokens_and_times(m, y16, 16000)
    assert lm_a.shape == lm_b.shape and len(times_a) == len(times_b)
    for a, b in zip(times_a, times_b):
        assert np.array_equal(a, b)
    print("%d Hz: log-mel max |diff| %.3g" % (sr, float(np.abs(lm_a - lm_b).max())))
    assert np.array_equal(tok_a, tok_b)
    notes = _tuples(m(y_native, sample_rate=sr))
    assert notes == _tuples(m(y16))
    return notes


def test_native_rate_transcription_on_the_trained_fixture():
    trained = checkpoints.load_compact_npz(CKPT)
    _, y16 = synthetic.synth_music(3 * 2.048 + 0.7, seed=21, device="cpu")
    m = inference.InferenceModel(trained, "mt3", dtype="float32")
    y44, y48 = _native(y16, 44100), _native(y16, 48000)
    n44 = _check_native_equals_host(m, y44, 44100)
    n48 = _check_native_equals_host(m, y48, 48000)
    assert len(n44) >= 5 and len(n48) >= 5
    assert _tuples(m(y16, sample_rate=16000)) == _tuples(m(y16))
    many = m.transcribe_many([y16, y44, y48], sample_rates=[16000, 44100, 48000])
    assert [_tuples(ns) for ns in many] == [_tuples(m(y16)), n44, n48]
    # teacher-forced scores of the same token rows
    rng = np.random.default_rng(5)
    n_seg = len(m._examples(y44, 44100)[0])
    targets = [np.concatenate([rng.integers(3, 1300, int(rng.integers(5, 60))), [1]]).astype(np.int32) for _ in range(n_seg)]
    s_a, t_a = m.score(y44, targets, True, sample_rate=44100)
    s_b, t_b = m.score(audio_io.resample(y44, 44100), targets, True)
    assert np.array_equal(s_a, s_b) and all(np.array_equal(a, b) for a, b in zip(t_a, t_b))
    for bad in (44101, 0, -16000):
        with pytest.raises(ValueError):
            m(y44, sample_rate=bad)
    with pytest.raises(ValueError):
        m.transcribe_many([y16, y44], sample_rates=[16000])


def test_native_rate_transcription_ismir2021_preset():
    """T = 512 segments, boosted random weights (as tests/test_gpu_end_to_end.py does)"""
    cfg = network.T5Config(dtype="float32", vocab_size=1664, num_encoder_layers=2, num_decoder_layers=2)
    params = synthetic.boost_note_events(network.init_random_params(cfg, seed=1, norm_scale_jitter=0.1),
                                         num_velocity_bins=127, eos=3.0, tie=1.0, velocity=2.0)
    m = inference.InferenceModel(params, "ismir2021", config=cfg)
    y16 = synthetic.synth_audio(3, seed=0, device="cpu", seg_samples=512 * 128).reshape(-1)[: 2 * 512 * 128 + 9000].numpy()
    assert len(_check_native_equals_host(m, _native(y16, 44100), 44100)) >= 5
    _check_native_equals_host(m, _native(y16, 22050), 22050)
