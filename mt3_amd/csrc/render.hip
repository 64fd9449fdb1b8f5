// Notes -> audio for gfx950: the NoteSequences of a job rendered into float32 samples (mt3_op_render_notes).  The rule:
// include/mt3_hip.h, "rendering notes to audio".
//
// Every output sample is an independent sum over the few notes sounding at its instant, in the rule's note order, so
// there is nothing to scatter and nothing to add atomically:
//   1. render_kernel, grid (tiles, sequences): a workgroup of 256 lanes owns a tile of 1024 consecutive samples of one
//      sequence, four per lane at a stride of 256 (a wave stores 256 contiguous bytes).  It finds the notes that can
//      sound in the tile by two binary searches -- on the sorted starts for the upper end, on the running maximum of the
//      sounding instants (d_reach, monotone by construction) for the lower -- and walks that range once, in order.  The
//      note's fields are uniform over the workgroup; a note that ended before the tile is skipped by a uniform branch,
//      and inside a note lanes diverge only in the tile that holds its first or last sample.
//      Per (note, sample): t = n / rate - start in float64 (n / rate once per sample).  Per partial: one float64 product
//      and fraction, then float32: the phase in turns is folded to [-1/4, 1/4] (exact in float32) and sin(2 pi q) taken
//      from an odd polynomial of degree 9 in q -- 3.4e-9 from the sine, 2.1e-7 with float32 Horner rounding, against
//      the 1.5e-5 tolerance of the int16 file.  The polynomial rather than v_sin_f32: its error is
//      known from the coefficients alone and is the same on every device, and it costs six VALU operations.
//   2. peak_kernel (normalize only), grid (blocks, sequences): max |sample| of the lanes' strided samples, the wave by
//      shuffles, the four waves through LDS, one atomic max per workgroup on the bit pattern (non-negative floats order
//      as their bit patterns do, and a maximum does not depend on the order it is taken in).
//   3. scale_kernel (normalize only): every sample times 0.9f / peak where peak > 0.
// The per-sequence tables ride in the kernel arguments, 128 sequences per launch.  Plain vector loads and stores; no LDS
// in render_kernel, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "mt3_hip.h"

#pragma clang fp contract(off)          // the rule names every rounding; the fused steps below are written as fmaf

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerLane = 4;
constexpr int kTile = MT3_RENDER_TILE;
static_assert(kTile == kThreads * kPerLane, "a tile is four samples per lane");
constexpr int kPerLaunch = 128;                      // sequences whose tables fit one launch's arguments
constexpr int kMaxSweepBlocks = 1024;                // peak / scale blocks per sequence; longer sequences stride
constexpr int kPartials = 6;
constexpr double kGuard = 0x1p-40;

struct SeqTable {                                    // 3.5 KiB by value
  int64_t out0[kPerLaunch];                          // the sequence's first sample in d_out
  int64_t note0[kPerLaunch];
  int64_t samples[kPerLaunch];
  int32_t notes[kPerLaunch];
};

// 2^(r / 12), r = 0 .. 11, correctly rounded to float64
__device__ __forceinline__ double twelfth_root(int r) {
  constexpr double kRoot[12] = {1.0,                1.0594630943592953, 1.122462048309373,  1.189207115002721,
                                1.2599210498948732, 1.3348398541700344, 1.4142135623730951, 1.4983070768766815,
                                1.5874010519681994, 1.681792830507429,  1.7817974362806785, 1.8877486253633868};
  double v = kRoot[0];
#pragma unroll
  for (int i = 1; i < 12; ++i) v = r == i ? kRoot[i] : v;      // selects on a uniform value: no table in memory
  return v;
}

// 440 * 2^((pitch - 69) / 12) for pitch 0 .. 127
__device__ __forceinline__ double pitch_hz(int32_t pitch) {
  const int q = pitch + 3;                           // pitch - 69 + 72: not negative
  return ldexp(440.0 * twelfth_root(q % 12), q / 12 - 6);
}

// sin(2 pi p) for a phase p in [0, 1] turns
__device__ __forceinline__ float sin_turns(float p) {
  const float r = p - rintf(p);                      // [-1/2, 1/2], exact
  const float q = fabsf(r) > 0.25f ? copysignf(0.5f, r) - r : r;      // sin(pi - x) = sin x; exact
  const float z = q * q;
  float y = fmaf(z, 39.53581371073427f, -76.54965682052698f);
  y = fmaf(z, y, 81.60099819260891f);
  y = fmaf(z, y, -41.341654929343406f);
  y = fmaf(z, y, 6.283185159611163f);
  return y * q;
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x;
}

// the least n with (double)n / rate - start >= 0: ceil(start * rate), put right where a rounding moved it by one
__device__ __forceinline__ int64_t first_sounding(double start, double rate) {
  double y = ceil(start * rate);
  if (!(y >= 0.0)) y = 0.0;
  if (y > 0x1p52) y = 0x1p52;
  int64_t c = static_cast<int64_t>(y);
  if (c > 0 && static_cast<double>(c - 1) / rate - start >= 0.0) --c;
  else if (static_cast<double>(c) / rate - start < 0.0) ++c;
  return c;
}

__global__ __launch_bounds__(kThreads) void render_kernel(SeqTable tab, const double* __restrict__ start,
                                                          const double* __restrict__ end,
                                                          const double* __restrict__ reach,
                                                          const int32_t* __restrict__ pitch,
                                                          const int32_t* __restrict__ velocity,
                                                          const int32_t* __restrict__ drum, int32_t sample_rate,
                                                          float* __restrict__ out) {
  const int r = blockIdx.y;
  const int64_t N = tab.samples[r];
  const int64_t n0 = static_cast<int64_t>(blockIdx.x) * kTile;
  if (n0 >= N) return;
  const int64_t n1 = n0 + kTile < N ? n0 + kTile : N;
  const double rate = static_cast<double>(sample_rate);
  const double t_first = static_cast<double>(n0) / rate, t_last = static_cast<double>(n1 - 1) / rate;
  const double t_from = t_first * (1.0 - kGuard) - kGuard;
  const int32_t count = tab.notes[r];
  start += tab.note0[r], end += tab.note0[r], reach += tab.note0[r];
  pitch += tab.note0[r], velocity += tab.note0[r], drum += tab.note0[r];

  // [lo, hi): lo the first note whose running reach comes up to the tile, hi the first whose start is past it.  Both
  // searches stay inside [0, count] whatever the arrays hold.
  int32_t a = 0, b = count;
  while (a < b) {
    const int32_t m = a + (b - a) / 2;
    if (start[m] > t_last) b = m; else a = m + 1;
  }
  const int32_t hi = a;
  a = 0, b = hi;
  while (a < b) {
    const int32_t m = a + (b - a) / 2;
    if (reach[m] >= t_from) b = m; else a = m + 1;
  }
  const int32_t lo = a;

  double T[kPerLane];
  float acc[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    T[j] = static_cast<double>(n0 + j * kThreads + threadIdx.x) / rate;
    acc[j] = 0.f;
  }

  for (int32_t i = lo; i < hi; ++i) {
    const double s = start[i];
    const int32_t p = pitch[i], v = velocity[i];
    if (static_cast<uint32_t>(p) > 127u || v == 0) continue;
    const float g = static_cast<float>(v) / 127.f;
    if (drum[i]) {
      if (s + MT3_RENDER_DRUM_SECONDS < t_from) continue;
      const int64_t first = first_sounding(s, rate);
      const uint32_t key = static_cast<uint32_t>(p) << 20;
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        const double t = T[j] - s;
        if (t >= 0.0 && t < MT3_RENDER_DRUM_SECONDS) {
          const uint32_t m = static_cast<uint32_t>(n0 + j * kThreads + threadIdx.x - first);
          const float u = static_cast<float>(mix32(key + m) >> 8) * 0x1p-23f - 1.f;
          acc[j] += g * (u * expf(static_cast<float>(t) * (-1.f / 0.03f)));
        }
      }
      continue;
    }
    const double d = end[i] - s, lim = d + MT3_RENDER_RELEASE_SECONDS;
    if (s + lim < t_from) continue;
    const double f0 = pitch_hz(p);
    double kf[kPartials];
    int K = 0;
#pragma unroll
    for (int k = 0; k < kPartials; ++k) {
      kf[k] = static_cast<double>(k + 1) * f0;
      K += kf[k] < 0.475 * rate;
    }
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const double t = T[j] - s;
      if (t >= 0.0 && t < lim) {
        const float tf = static_cast<float>(t), past = static_cast<float>(t - d);
        const float env = fminf(tf * 250.f, 1.f) * expf(tf * (-1.f / 0.7f)) * fminf(fmaxf(1.f - past * 25.f, 0.f), 1.f);
        float tone = 0.f;
#pragma unroll
        for (int k = 0; k < kPartials; ++k) {
          if (k < K) {                               // uniform: the partials below 0.475 of the rate are the first K
            const double turns = kf[k] * t;
            const float ph = static_cast<float>(turns - floor(turns));
            tone = fmaf(sin_turns(ph), 1.f / static_cast<float>(k + 1), tone);
          }
        }
        acc[j] += (g * env) * tone;
      }
    }
  }

  float* dst = out + tab.out0[r];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int64_t n = n0 + j * kThreads + threadIdx.x;
    if (n < n1) dst[n] = acc[j];
  }
}

// grid (blocks, sequences): peaks[sequence] = max(peaks[sequence], max |sample| of this workgroup's samples)
__global__ __launch_bounds__(kThreads) void peak_kernel(SeqTable tab, const float* __restrict__ out, float* peaks) {
  __shared__ float s_max[kWaves];
  const int r = blockIdx.y;
  const int64_t N = tab.samples[r];
  const float* src = out + tab.out0[r];
  float m = 0.f;
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; n < N;
       n += static_cast<int64_t>(gridDim.x) * kThreads)
    m = fmaxf(m, fabsf(src[n]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = fmaxf(m, s_max[w]);
    if (m > 0.f) atomicMax(reinterpret_cast<unsigned int*>(peaks + r), __float_as_uint(m));
  }
}

__global__ __launch_bounds__(kThreads) void scale_kernel(SeqTable tab, float* out, const float* __restrict__ peaks) {
  const int r = blockIdx.y;
  const float peak = peaks[r];
  if (!(peak > 0.f)) return;
  const float scale = 0.9f / peak;
  const int64_t N = tab.samples[r];
  float* dst = out + tab.out0[r];
  for (int64_t n = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; n < N;
       n += static_cast<int64_t>(gridDim.x) * kThreads)
    dst[n] *= scale;
}

}  // namespace

extern "C" int mt3_op_render_notes(const double* d_start, const double* d_end, const double* d_reach,
                                   const int32_t* d_pitch, const int32_t* d_velocity, const int32_t* d_is_drum,
                                   int64_t n_notes, int32_t n_seq, const int64_t* h_note_offsets,
                                   const int64_t* h_sample_offsets, const int64_t* h_n_samples, int32_t sample_rate,
                                   int32_t normalize, float* d_out, int64_t out_capacity, float* d_peaks, void* stream) {
  const std::string who = "mt3_op_render_notes: ";
  if (n_seq < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_seq must not be negative");
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (sample_rate < 1 || sample_rate > MT3_RENDER_MAX_SAMPLE_RATE)
    return mt3::fail(MT3_ERR_INVALID, who + "sample_rate must be 1 .. 384000");
  if (out_capacity < 0) return mt3::fail(MT3_ERR_INVALID, who + "out_capacity must not be negative");
  if (n_seq == 0) return MT3_OK;
  if (!h_note_offsets || !h_sample_offsets || !h_n_samples) return mt3::fail(MT3_ERR_INVALID, who + "null table");
  if (n_notes > 0 && (!d_start || !d_end || !d_reach || !d_pitch || !d_velocity || !d_is_drum))
    return mt3::fail(MT3_ERR_INVALID, who + "null note array");
  if (h_note_offsets[0] < 0 || h_note_offsets[n_seq] > n_notes)
    return mt3::fail(MT3_ERR_INVALID, who + "h_note_offsets must lie inside [0, n_notes]");
  int64_t span1 = 0, total = 0;
  for (int32_t i = 0; i < n_seq; ++i) {
    if (h_note_offsets[i + 1] < h_note_offsets[i]) return mt3::fail(MT3_ERR_INVALID, who + "h_note_offsets must not decrease");
    if (h_note_offsets[i + 1] - h_note_offsets[i] > INT32_MAX)
      return mt3::fail(MT3_ERR_INVALID, who + "more than 2^31 - 1 notes in one sequence");
    if (h_n_samples[i] < 0) return mt3::fail(MT3_ERR_INVALID, who + "h_n_samples: negative length");
    if (h_n_samples[i] > MT3_RENDER_MAX_SAMPLES) return mt3::fail(MT3_ERR_INVALID, who + "h_n_samples: more than 2^40 samples");
    if (h_sample_offsets[i] < 0 || h_sample_offsets[i] > INT64_MAX / 8)
      return mt3::fail(MT3_ERR_INVALID, who + "h_sample_offsets: sample offset negative or too large");
    if (h_sample_offsets[i] < span1)
      return mt3::fail(MT3_ERR_INVALID, who + "h_sample_offsets: sequences overlap or are out of order");
    span1 = h_sample_offsets[i] + h_n_samples[i];
    total += h_n_samples[i];
  }
  if (span1 > out_capacity) return mt3::fail(MT3_ERR_INVALID, who + "the sequences end past out_capacity");
  if (total == 0) return MT3_OK;
  if (!d_out) return mt3::fail(MT3_ERR_INVALID, who + "null d_out");
  if (normalize && !d_peaks) return mt3::fail(MT3_ERR_INVALID, who + "null d_peaks with normalize set");

  hipStream_t s = static_cast<hipStream_t>(stream);
  if (normalize) MT3_HIP_CHECK(hipMemsetAsync(d_peaks, 0, static_cast<size_t>(n_seq) * sizeof(float), s));
  for (int32_t r0 = 0; r0 < n_seq; r0 += kPerLaunch) {
    const int n = n_seq - r0 < kPerLaunch ? n_seq - r0 : kPerLaunch;
    SeqTable t{};
    int64_t longest = 0;
    for (int j = 0; j < n; ++j) {
      t.out0[j] = h_sample_offsets[r0 + j];
      t.note0[j] = h_note_offsets[r0 + j];
      t.samples[j] = h_n_samples[r0 + j];
      t.notes[j] = static_cast<int32_t>(h_note_offsets[r0 + j + 1] - h_note_offsets[r0 + j]);
      if (t.samples[j] > longest) longest = t.samples[j];
    }
    if (longest == 0) continue;
    const uint32_t tiles = static_cast<uint32_t>((longest + kTile - 1) / kTile);
    hipLaunchKernelGGL(render_kernel, dim3(tiles, static_cast<uint32_t>(n)), dim3(kThreads), 0, s, t, d_start, d_end,
                       d_reach, d_pitch, d_velocity, d_is_drum, sample_rate, d_out);
    MT3_HIP_CHECK(hipGetLastError());
    if (normalize) {
      int64_t blocks = (longest + kThreads - 1) / kThreads;
      if (blocks > kMaxSweepBlocks) blocks = kMaxSweepBlocks;
      const dim3 grid(static_cast<uint32_t>(blocks), static_cast<uint32_t>(n));
      hipLaunchKernelGGL(peak_kernel, grid, dim3(kThreads), 0, s, t, d_out, d_peaks + r0);
      MT3_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(scale_kernel, grid, dim3(kThreads), 0, s, t, d_out, d_peaks + r0);
      MT3_HIP_CHECK(hipGetLastError());
    }
  }
  return MT3_OK;
}
