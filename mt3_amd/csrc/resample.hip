// Rational polyphase FIR resampler for gfx950: scipy.signal.resample_poly(x, up, down, window=w) with the default
// padtype (zeros outside x), summed in float64 and rounded to float32 once.
//
// Replaces the host resample of note_seq.audio_io.wav_data_to_samples_librosa (NB cell 2), which the package evaluates
// as mt3_amd/audio_io.resample(..., "kaiser_best"): resample_poly in float64 with resampy's kaiser_best filter.
//
//   H      = w * up                                (float64, 2*half + 1 taps: the table scipy applies)
//   n_out  = ceil(n_in * up / down)
//   y[n]   = sum_k x[k] * H[n*down + half - k*up]   (H indices outside [0, 2*half] and k outside [0, n_in) are zero)
//
// Layout:
//   * the taps are reordered once, at create time, into a phase-major table [up][taps_per_phase] (zero padded): output n
//     has phase p = (n*down + half) mod up and reads row p contiguously, tap t against input kmax - t with
//     kmax = (n*down + half) div up.  The table (452 KB at 44.1 kHz, 655 KB at 11.025 kHz) does not fit in LDS; it
//     stays in L2 / the vector L1.
//   * one lane per output, 256 consecutive outputs per workgroup (lanes walk consecutive outputs, i.e. scattered
//     phases).  The workgroup's input span -- (255*down + n_taps) / up samples, 1,058 at 44.1 kHz -- is staged in LDS
//     as f32, kSpan samples per pass; longer spans (large `down`) take several passes, each lane summing the taps whose
//     input falls in the pass.
//   * every product is f32 -> f64 times the f64 tap, accumulated by v_fma_f64 from +0.0; index arithmetic is int64
//     (n*down reaches 4.2e9 on a 10-minute 44.1 kHz file).
//   * outputs n_out <= n < out_capacity are written as 0.0 (the frontend's zero-padded [n_segments, T*hop] layout);
//     nothing at or past out_capacity is touched.
//   * the input is a sample source (pcm.h), read only by the LDS staging line: a float32 array (mt3_resampler_run) or
//     a WAV file's PCM frames, decoded and mixed down to mono as they are staged (mt3_resampler_run_pcm: the decode
//     inside wav_data_to_samples_librosa, NB cell 2, fused in).  A frame is decoded once per workgroup whose span
//     holds it, about 1.5 times at 44.1 kHz, against 353 f64 multiply-adds per output.  From LDS on both paths are
//     the same code, so the PCM path gives mt3_resampler_run's bits on read_wav's samples.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "common.h"
#include "mt3_hip.h"
#include "pcm.h"

struct mt3_resampler {
  int32_t up = 0, down = 0;
  int64_t half = 0;          // (n_taps - 1) / 2
  int32_t tpp = 0;           // taps per phase: ceil(n_taps / up)
  double* d_taps = nullptr;  // [up][tpp]
};

namespace {

constexpr int kThreads = 256;          // outputs per workgroup
constexpr int kSpan = 4096;            // input samples staged in LDS per pass (16 KB)
constexpr int64_t kMaxTaps = 1 << 20;

template <class Src>
__global__ __launch_bounds__(kThreads) void resample_poly_kernel(Src x, int64_t n_in,
                                                                 const double* __restrict__ taps, int32_t up,
                                                                 int32_t down, int64_t half, int32_t tpp,
                                                                 int64_t n_out, float* __restrict__ y, int64_t cap) {
  __shared__ float xs[kSpan];
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kThreads;
  const int64_t n = n0 + threadIdx.x;
  if (n0 >= n_out) {                                   // a tile of the zero tail (uniform over the workgroup)
    if (n < cap) y[n] = 0.f;
    return;
  }
  const int64_t n_last = (n0 + kThreads < n_out ? n0 + kThreads : n_out) - 1;
  const int64_t m = n * down + half;
  const int64_t kmax = m / up;                         // input index of tap 0
  const double* h = taps + (m - kmax * up) * tpp;      // phase row
  // inputs any live output of the tile reads, clipped to [0, n_in)
  int64_t lo = (n0 * down + half) / up - (tpp - 1), hi = (n_last * down + half) / up;
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_in - 1 ? n_in - 1 : hi;
  double acc = 0.0;
  for (int64_t c0 = lo; c0 <= hi; c0 += kSpan) {
    const int len = static_cast<int>(hi + 1 - c0 < kSpan ? hi + 1 - c0 : kSpan);
    __syncthreads();                                   // the previous pass has been read
    for (int i = threadIdx.x; i < len; i += kThreads) xs[i] = x(c0 + i);
    __syncthreads();
    if (n <= n_last) {
      // taps t with kmax - t in [c0, c0 + len) and 0 <= t < tpp
      const int64_t d = kmax - c0;
      const int64_t t_lo = d - len + 1 > 0 ? d - len + 1 : 0, t_hi = d < tpp - 1 ? d : tpp - 1;
      if (t_lo <= t_hi) {                              // then d <= tpp + len - 2 < 2^21: int indices
        const int di = static_cast<int>(d), t1 = static_cast<int>(t_hi);
#pragma unroll 4
        for (int t = static_cast<int>(t_lo); t <= t1; ++t) acc = fma(static_cast<double>(xs[di - t]), h[t], acc);
      }
    }
  }
  if (n < cap) y[n] = n <= n_last ? static_cast<float>(acc) : 0.f;
}

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// the size checks and the one launch mt3_resampler_run and mt3_resampler_run_pcm share (n_in >= 1 samples of `src`)
template <class Src>
int launch(const char* who, const mt3_resampler* r, Src src, int64_t n_in, float* d_out, int64_t out_capacity,
           void* stream) {
  const std::string w(who);
  const int64_t n_out = mt3_resample_output_length(n_in, r->up, r->down);
  if (n_out < 0) return mt3::fail(MT3_ERR_INVALID, w + ": n_in too large");
  if (out_capacity < n_out)
    return mt3::fail(MT3_ERR_INVALID, w + ": out_capacity " + std::to_string(out_capacity) + " is less than the " +
                                          std::to_string(n_out) + " output samples");
  const int64_t blocks = (out_capacity + kThreads - 1) / kThreads;
  // n*down + half must stay in int64 for every n of the grid
  if (blocks > INT32_MAX || blocks * kThreads > (INT64_MAX / 2 - r->half) / r->down)
    return mt3::fail(MT3_ERR_INVALID, w + ": out_capacity too large");
  hipLaunchKernelGGL(resample_poly_kernel<Src>, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), src, n_in, r->d_taps, r->up, r->down, r->half, r->tpp, n_out,
                     d_out, out_capacity);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

}  // namespace

extern "C" {

int64_t mt3_resample_output_length(int64_t n_in, int32_t up, int32_t down) {
  if (n_in < 0 || up < 1 || down < 1) return -1;
  // ceil(n_in * up / down) without forming n_in * up: q*up + ceil(r*up / down), r*up < 2^62
  const int64_t q = n_in / down, r = n_in % down;
  if (q > (INT64_MAX - up) / up) return -1;
  return q * up + (r * up + down - 1) / down;
}

int mt3_resampler_create(const double* h_taps, int64_t n_taps, int32_t up, int32_t down, mt3_resampler** out) {
  if (!h_taps || !out) return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_create: null argument");
  if (n_taps < 1 || n_taps % 2 == 0)
    return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_create: n_taps must be positive and odd (2*half + 1), got " +
                                          std::to_string(n_taps));
  if (n_taps > kMaxTaps)
    return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_create: " + std::to_string(n_taps) + " taps is more than 2^20");
  if (up < 1 || down < 1)
    return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_create: up and down must be >= 1");
  if (gcd64(up, down) != 1)
    return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_create: up/down must be in lowest terms (gcd(up, down) == 1)");
  auto* r = new (std::nothrow) mt3_resampler;
  if (!r) return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_create: out of host memory");
  r->up = up;
  r->down = down;
  r->half = (n_taps - 1) / 2;
  r->tpp = static_cast<int32_t>((n_taps + up - 1) / up);
  std::vector<double> table(static_cast<size_t>(up) * r->tpp, 0.0);
  for (int64_t i = 0; i < n_taps; ++i) table[static_cast<size_t>(i % up) * r->tpp + i / up] = h_taps[i];
  hipError_t e = hipMalloc(&r->d_taps, table.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(r->d_taps, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (r->d_taps) (void)hipFree(r->d_taps);
    delete r;
    return mt3::fail(MT3_ERR_HIP, std::string("mt3_resampler_create: ") + hipGetErrorString(e));
  }
  *out = r;
  return MT3_OK;
}

void mt3_resampler_destroy(mt3_resampler* r) {
  if (!r) return;
  if (r->d_taps) (void)hipFree(r->d_taps);
  delete r;
}

int mt3_resampler_run(mt3_resampler* r, const float* d_in, int64_t n_in, float* d_out, int64_t out_capacity,
                      void* stream) {
  if (!r || !d_in || !d_out) return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_run: null argument");
  if (n_in < 1) return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_run: n_in must be >= 1");
  return launch("mt3_resampler_run", r, mt3::F32Samples{d_in}, n_in, d_out, out_capacity, stream);
}

int mt3_resampler_run_pcm(mt3_resampler* r, const void* d_pcm, int64_t n_frames, int32_t channels, int32_t format,
                          float* d_out, int64_t out_capacity, void* stream) {
  const int rc = mt3::pcm_check("mt3_resampler_run_pcm", d_pcm, d_out, n_frames, channels, format);
  if (rc != MT3_OK) return rc;
  if (!r) return mt3::fail(MT3_ERR_INVALID, "mt3_resampler_run_pcm: null resampler");
  return mt3::pcm_dispatch(format, d_pcm, channels, [&](auto src) {
    return launch("mt3_resampler_run_pcm", r, src, n_frames, d_out, out_capacity, stream);
  });
}

}  // extern "C"
