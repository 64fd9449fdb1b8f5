"""The log-mel frontend kernel (mt3_amd/csrc/frontend.hip) in the forms its callers launch: every segment length the
addressing depends on, frame counts on tile / wave / round edges, every (tile, wave, round) position bit for bit,
poison past the count, int16-scale and very quiet audio, non-finite samples.  The reference is the numpy oracle
(oracle/frontend.py, float64 on the product's default tables) at test_frontend_vs_oracle's bounds; the case tables are
tests/frontend_cases.py, which tests/test_frontend_forms_ref.py runs through the kernel's lane program on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from mt3_amd import spectrograms as SP  # noqa: E402
from tests import frontend_cases as fc  # noqa: E402


def run(audio, counts):
    """spectrograms.compute_spectrogram_batch (host counts, the current stream) -> CUDA [S, F, 512]"""
    return SP.compute_spectrogram_batch(torch.from_numpy(np.array(audio, np.float32)).cuda(), counts)


def run_dev(audio, counts, side_stream):
    """mt3_frontend_logmel_dev: the counts in device memory, optionally on a stream of its own"""
    a = torch.from_numpy(np.array(audio, np.float32)).cuda()
    S, frames = a.shape[0], a.shape[1] // fc.HOP
    d_counts = torch.tensor(counts, dtype=torch.int32, device="cuda")
    out = torch.full((S, frames, fc.MEL), 7.0, device="cuda")
    s = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(_lib.load().mt3_frontend_logmel_dev(SP._frontend(SP.SpectrogramConfig()), a.data_ptr(), S, frames,
                                                       d_counts.data_ptr(), out.data_ptr(), s.cuda_stream))
    s.synchronize()
    return out


# ------------------------------------------------------------------------------------------- a. shapes and counts
@pytest.mark.parametrize("frames", fc.SEGMENT_FRAMES)
def test_shapes_and_counts_vs_oracle(frames):
    audio, counts = fc.shape_batch(frames)
    fc.check_shape_batch(frames, run(audio, counts).cpu().numpy())


@pytest.mark.parametrize("length", fc.ODD_LENGTHS)
def test_lengths_that_are_no_multiple_of_the_hop(length):
    x, padded = fc.odd_length_samples(length)
    got = SP.compute_spectrogram(x)
    n = len(padded) // fc.HOP
    assert got.shape == (n, fc.MEL)
    fc.check_segment(got, ("odd", length), padded, n, f"{length} samples")


# ------------------------------------------------------------------------------------------- b. position independence
@pytest.mark.parametrize("frames", sorted(fc.PERIODIC))
def test_a_row_depends_only_on_its_window(frames):
    """Audio of period 128 = one hop: every frame with the same number of hops past the segment's end sees the same 2048
    values, so all rows of a class are bit-identical whichever workgroup, wave (own s_xchg / s_mag region) and round
    computed them -- EVERY row is in the comparison.  One repeat, the device-count entry point and a stream of its own
    give the same bits."""
    audio, counts = fc.periodic_batch(frames)
    out = run(audio, counts)
    cls = torch.from_numpy(fc.overhang_classes(frames, counts)).cuda()
    covered = 0
    for j in range(-1, 16):
        rows = out[cls == j]
        covered += rows.shape[0]
        assert rows.shape[0] >= 4
        assert torch.equal(rows, (rows[:1] if j >= 0 else torch.zeros_like(rows[:1])).expand_as(rows)), f"overhang {j}"
    assert covered == cls.numel()
    fc.check_periodic(frames, out.cpu().numpy())                # the same comparison in numpy, and the oracle
    assert torch.equal(run(audio, counts), out)
    assert torch.equal(run_dev(audio, counts, side_stream=False), out)
    assert torch.equal(run_dev(audio, counts, side_stream=True), out)


# ------------------------------------------------------------------------------------------- c. nothing past the count
@pytest.mark.parametrize("frames", fc.SEGMENT_FRAMES)
def test_samples_past_the_count_are_not_read(frames):
    audio, counts = fc.shape_batch(frames)
    assert 0 in counts and frames - 1 in counts
    zeros = run(fc.poisoned(audio, counts, 0.0), counts).cpu().numpy()
    assert np.isfinite(zeros).all()
    for value in (np.nan, 3e38):
        np.testing.assert_array_equal(run(fc.poisoned(audio, counts, value), counts).cpu().numpy(), zeros)
    np.testing.assert_array_equal(run(audio, counts).cpu().numpy(), zeros)


# ------------------------------------------------------------------------------------------- d. scale
# x * 2^k is exact in float32 and every step up to the mel value is linear or the square root of a sum of squares, so
# the mel values scale exactly unless something under- or overflows: only the log differs.
@pytest.fixture(scope="module")
def scaled_outputs():
    audio, counts = fc.scale_batch()
    outs = {}
    for k in (0, 15, -20):
        scaled = audio * np.float32(2.0 ** k)
        assert np.array_equal(scaled.astype(np.float64), audio.astype(np.float64) * 2.0 ** k)
        outs[k] = run(scaled, counts).cpu().numpy()
    return audio, counts, outs


def test_scaling_by_a_power_of_two_adds_k_ln_2(scaled_outputs):
    """out_k - out_0 = k ln 2 up to the log itself: 1 ulp for v_log_f32 and one rounding of the product with ln 2 on each
    side, 4 ulp of float32 at the larger of the two values (measured: 0.94); bins at the floor stay at the floor."""
    audio, counts, outs = scaled_outputs
    exists = np.arange(fc.SCALE_FRAMES)[None, :] < np.asarray(counts)[:, None]
    out0 = outs[0]
    empty = out0 == fc.FLOOR
    assert empty[exists].sum() == 2 * exists.sum()              # the two structurally empty columns and no other bin
    live = exists[:, :, None] & ~empty
    worst = {}
    for k in (15, -20):
        outk = outs[k]
        assert not outk[~exists].any() and np.all(outk[empty] == fc.FLOOR) and np.isfinite(outk).all()
        diff = np.abs(outk.astype(np.float64) - out0.astype(np.float64) - k * np.log(2.0))
        ulp = np.spacing(np.maximum(np.abs(outk), np.abs(out0)).astype(np.float32)).astype(np.float64)
        worst[k] = float((diff / ulp)[live].max())
    print("frontend scale: worst |out_k - out_0 - k ln 2| in float32 ulp:", worst, "lowest live value", out0[live].min())
    assert max(worst.values()) <= 4.0, worst


def test_int16_scale_vs_oracle(scaled_outputs):
    """out_{+15} against the oracle on the scaled audio at the bounds of the shape tests, which scale with the peak.

    This is a check of the LOG: on noise bands the mel value is 3 to 4 times the frame's spectral peak, so at log values of
    11 to 15 the linear bound 4e-6 * peak asks for a log within about one float32 ulp (9.5e-7).  A log2 of the whole value
    times ln 2 (v_log_f32's 1 ulp taken at a log2 near 20) was up to 1.5 ulp off and reached 1.455 of the bound here;
    safe_log_fast takes the instruction's log2 of the mantissa alone and stays where libm's logf does (0.48 of it)."""
    audio, counts, outs = scaled_outputs
    scaled = audio * np.float32(2.0 ** 15)
    for k, x in ((0, audio), (15, scaled)):
        for s, n in enumerate(counts):
            ref, peak = fc.oracle_rows(("scale", k, s), x[s][: n * fc.HOP])
            print(f"frontend scale 2^{k} segment {s}: " + fc.describe_rows(outs[k][s][:n], ref, peak))
    for s, n in enumerate(counts):
        fc.check_segment(outs[0][s], ("scale", 0, s), audio[s], n, f"2^0 segment {s}")
    for s, n in enumerate(counts):
        fc.check_segment(outs[15][s], ("scale", 15, s), scaled[s], n, f"2^15 segment {s}")


def test_mel_values_below_flt_min_are_clamped_or_floored():
    """the documented clamp of safe_log_fast: with the noise segment scaled by 2^-130 every output is finite and either
    exactly the floor log(1e-5) (the mel value came out as 0) or at most log(FLT_MIN) (a denormal read as the smallest
    normal number); which of the FFT's denormals survive on the device is not pinned"""
    audio, counts = fc.scale_batch()
    tiny = run(audio[2:] * np.float32(2.0 ** -130), counts[2:]).cpu().numpy()
    assert np.isfinite(tiny).all()
    at_floor, clamped = tiny == fc.FLOOR, tiny <= fc.LOG_FLT_MIN + np.float32(1e-4)
    print("frontend scale 2^-130: values at the floor", int(at_floor.sum()), "at or below log(FLT_MIN)", int(clamped.sum()),
          "of", tiny.size)
    assert np.all(at_floor | clamped)


# ------------------------------------------------------------------------------------------- e. non-finite samples
def test_nonfinite_samples_make_nan_rows_and_nothing_else():
    """the reference's rule (a dense mel product, then safe_log): a frame whose window holds a NaN or an Inf is NaN in
    all 512 bins, every other frame and every other segment has the bits it has with a zero in that place"""
    bad, clean = fc.nonfinite_batches()
    fc.check_nonfinite(run(bad, fc.NONFINITE_COUNTS).cpu().numpy(), run(clean, fc.NONFINITE_COUNTS).cpu().numpy())
