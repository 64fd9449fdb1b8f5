"""Shared by tests/test_frontend_forms_ref.py (the kernel's lane program on the CPU) and tests/test_gpu_frontend_forms.py
(the kernel): the case tables of the log-mel frontend's forms -- segment lengths, ragged frame counts, periodic audio,
poison past the count, non-finite samples -- and the comparison with the numpy oracle (oracle/frontend.py, float64
arithmetic on the product's default "tf32" tables) at the bounds tests/test_gpu_kernels.py::test_frontend_vs_oracle uses.

Everything is numpy and deterministic, so both files see the same samples and the oracle's answer is computed once per
process (`oracle_rows`) and handed out read-only."""
import numpy as np

from oracle import frontend as F

HOP, FFT, MEL = 128, 2048, 512
FLOOR = np.float32(np.log(np.float32(1e-5)))                     # safe_log's floor, as numpy's float32 evaluates it
LOG_FLT_MIN = np.float32(np.log(np.float64(1.17549435e-38)))     # the documented clamp of a denormal mel value
SEGMENT_FRAMES = (16, 32, 48, 512, 256)                          # frames_per_segment of the shape batches
_EDGE_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32)               # next to multiples of 4 (a round) and 16 (a tile)


def counts_for(frames):
    """the frame counts of one shape batch: the edges above, F - 1 and F, inside [0, F]"""
    return sorted({c for c in _EDGE_COUNTS + (frames - 1, frames) if 0 <= c <= frames})


_batches = {}


def shape_batch(frames):
    """(audio [S, F * 128] float32, counts [S]): synthetic music, one segment per count of counts_for(F) in an order that
    puts ragged counts side by side, and a last segment of white noise (no empty-energy bins) with every frame present.
    The audio goes on past every count: what lies there must not matter."""
    if frames not in _batches:
        rng = np.random.default_rng(1000 + frames)
        counts = [int(c) for c in rng.permutation(counts_for(frames))] + [frames]
        audio = F.synth_audio(len(counts), seed=frames, seg_samples=frames * HOP)
        audio[-1] = rng.uniform(-1, 1, frames * HOP).astype(np.float32)
        audio.setflags(write=False)
        _batches[frames] = (audio, counts)
    return _batches[frames]


def poisoned(audio, counts, value):
    """a copy with every sample at and beyond counts[s] * 128 of segment s overwritten"""
    out = np.array(audio, np.float32)
    for s, n in enumerate(counts):
        out[s, n * HOP:] = value
    return out


_oracle = {}


def oracle_rows(key, samples):
    """(log-mel [n, 512] float64, per-frame spectral peak [n]) of `samples` (a whole number of hops, zero-padded past
    its end as pad_end=True does), cached under `key`"""
    if key not in _oracle:
        x = np.asarray(samples, np.float32)
        assert len(x) % HOP == 0
        ref = F.compute_logmel(x, np.float64, tables="tf32")
        frames = F.frame_signal(x.astype(np.float64)) * F.hann_periodic_tf32().astype(np.float64)
        peak = np.abs(np.fft.rfft(frames, axis=-1)).max(1) if len(x) else np.zeros(0)
        ref.setflags(write=False)
        peak.setflags(write=False)
        _oracle[key] = (ref, peak)
    return _oracle[key]


def check_rows(got, ref, peak, what):
    """test_frontend_vs_oracle's bounds on rows that exist: the f32 FFT's noise floor relative to the frame's spectral
    peak in the linear domain, 1e-3 in the log where a bin carries signal, the two empty mel columns exactly the floor"""
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float32, what
    assert np.isfinite(got).all(), what
    mel_ref, mel_got = np.exp(ref), np.exp(got.astype(np.float64))
    lin = np.abs(mel_got - mel_ref)
    assert np.all(lin <= 4e-6 * peak[:, None] + 1.1e-5 * 1e-5 + 1e-12), f"{what}: linear error {lin.max()}"
    sig = mel_ref >= 1e-3 * np.maximum(peak[:, None], 1e-30)
    if sig.any():
        err = np.abs(got - ref)[sig].max()
        assert err < 1e-3, f"{what}: log error {err}"
    assert np.all(got[:, [1, 10]] == FLOOR), what


def describe_rows(got, ref, peak):
    """the figures check_rows bounds, for a test to print before it asserts"""
    mel_ref = np.exp(ref)
    lin = np.abs(np.exp(np.asarray(got, np.float64)) - mel_ref) / (4e-6 * peak[:, None] + 1.1e-5 * 1e-5 + 1e-12)
    f, b = np.unravel_index(lin.argmax(), lin.shape)
    sig = mel_ref >= 1e-3 * np.maximum(peak[:, None], 1e-30)
    return ("worst linear error %.3f of its bound (frame %d bin %d, mel / peak %.2f, value %.4f, %d of %d values over "
            "the bound), worst log error on signal bins %.2e" % (lin.max(), f, b, mel_ref[f, b] / peak[f], ref[f, b],
                                                                 int((lin > 1).sum()), lin.size, np.abs(got - ref)[sig].max()))


def check_segment(got, key, samples, n, what):
    """one segment's [F, 512] output against the oracle on its first n * 128 samples; rows >= n exactly 0.0"""
    got = np.asarray(got)
    assert np.all(got[n:] == 0.0), f"{what}: rows past the count must be exactly 0.0"
    ref, peak = oracle_rows(key, np.asarray(samples)[: n * HOP])
    assert ref.shape == (n, MEL)
    check_rows(got[:n], ref, peak, what)


def check_shape_batch(frames, out):
    audio, counts = shape_batch(frames)
    assert out.shape == (len(counts), frames, MEL)
    for s, n in enumerate(counts):
        check_segment(out[s], ("shape", frames, s), audio[s], n, f"F={frames} segment {s} n={n}")
        if n == 0:
            assert np.abs(audio[s]).max() > 0.1 and not out[s].any()


ODD_LENGTHS = (1000, 100 * HOP + 37, 1)                          # compute_spectrogram: not a multiple of the hop


def odd_length_samples(length):
    x = F.synth_audio(1, seed=length, seg_samples=max(length, FFT))[0, :length]
    if length < HOP:
        x = np.full(length, 0.5, np.float32)
    padded = np.zeros(-(-length // HOP) * HOP, np.float32)
    padded[:length] = x
    return x, padded


# ------------------------------------------------------------------------------------------------ periodic audio
# One random block of 128 samples, tiled: the hop is one period, so frame f of a segment with n frames sees the block
# 16 - j times and then 128 j zeros, j = max(0, f + 16 - n) hops of its window lying past the segment's end -- the SAME
# 2048 values for every frame of that j, in whichever segment, tile, wave and round it is computed.
PERIODIC = {64: [64, 63, 49, 48, 33, 17, 16], 512: [512, 497, 256, 17]}


def periodic_batch(frames):
    block = np.random.default_rng(7).uniform(-1, 1, HOP).astype(np.float32)
    counts = PERIODIC[frames]
    audio = np.tile(block, (len(counts), frames))
    assert audio.shape == (len(counts), frames * HOP)
    return audio, counts


def overhang_classes(frames, counts):
    """[S, F] int: j of every row that exists, -1 for rows past the count"""
    f = np.arange(frames)[None, :]
    n = np.asarray(counts)[:, None]
    return np.where(f < n, np.maximum(0, f + FFT // HOP - n), -1)


def check_periodic(frames, out):
    """EVERY row is compared bit for bit with the first row of its class; one segment against the oracle"""
    audio, counts = periodic_batch(frames)
    cls = overhang_classes(frames, counts)
    assert out.shape == cls.shape + (MEL,)
    seen = 0
    for j in range(-1, FFT // HOP):
        rows = out[cls == j]
        seen += len(rows)
        if j < 0:
            assert not rows.any()
        else:
            assert len(rows) >= 4, (j, len(rows))
            np.testing.assert_array_equal(rows, np.broadcast_to(rows[0], rows.shape), err_msg=f"F={frames} overhang {j}")
    assert seen == cls.size and set(np.unique(cls)) == set(range(-1, 16))
    check_segment(out[0], ("periodic", frames), audio[0], counts[0], f"periodic F={frames}")   # holds every class


# ------------------------------------------------------------------------------------------------ scale
SCALE_FRAMES, SCALE_COUNTS = 64, [64, 50, 64]


def scale_batch():
    """white noise under synthetic music (no non-empty mel band near zero in any frame that exists, the overhanging
    ones included); the last segment is the noise alone"""
    rng = np.random.default_rng(21)
    noise = rng.uniform(-0.5, 0.5, (3, SCALE_FRAMES * HOP)).astype(np.float32)
    audio = (0.5 * F.synth_audio(3, seed=21, seg_samples=SCALE_FRAMES * HOP) + noise).astype(np.float32)
    audio[2] = 2 * noise[2]
    return audio, SCALE_COUNTS


# ------------------------------------------------------------------------------------------------ non-finite samples
# (segment, sample, value, frame count) in one batch of 256-frame segments; the segments between them stay clean
NONFINITE_FRAMES = 256
NONFINITE = ((1, 5000, np.nan, 256), (3, 3000, np.inf, 100), (5, 12790, -np.inf, 100))
NONFINITE_COUNTS = [256, 256, 200, 100, 256, 100, 31]


def hit_frames(sample, n):
    """frames of a segment with n frames whose window [128 f, 128 f + 2048) holds `sample`"""
    return [f for f in range(n) if HOP * f <= sample < HOP * f + FFT]


def nonfinite_batches():
    """(audio with the bad samples, the same audio with zeros there)"""
    clean = np.array(F.synth_audio(len(NONFINITE_COUNTS), seed=11, seg_samples=NONFINITE_FRAMES * HOP))
    bad = clean.copy()
    for s, p, v, _ in NONFINITE:
        clean[s, p] = 0.0
        bad[s, p] = v
    return bad, clean


def check_nonfinite(out_bad, out_clean):
    assert hit_frames(5000, 256) == list(range(24, 40))
    for s, n in enumerate(NONFINITE_COUNTS):
        hit = next((hit_frames(p, cnt) for seg, p, _, cnt in NONFINITE if seg == s), [])
        assert all(cnt == NONFINITE_COUNTS[seg] for seg, _, _, cnt in NONFINITE)
        ok = np.ones(NONFINITE_FRAMES, bool)
        ok[hit] = False
        assert np.isnan(out_bad[s][~ok]).all(), f"segment {s}: every bin of a frame that saw the sample is NaN"
        np.testing.assert_array_equal(out_bad[s][ok], out_clean[s][ok], err_msg=f"segment {s}")
        assert not out_bad[s][n:].any() and np.isfinite(out_clean[s]).all()
