// Piano rolls and frame counts for gfx950: the notes of a job -> float32 rolls [128, F] (mt3_op_pianoroll), pairs of
// rolls -> (TP, FP, FN) (mt3_op_frame_counts).  The rule: include/mt3_hip.h, "piano rolls and frame counts".
//
// A roll is the sum over its notes of velocity * [f0 <= column < f1].  Written note by note that costs the note's length;
// here a note costs two adds whatever its length, and the lengths are paid once per row:
//   1. the span of the job's rolls is zeroed by a memset on the stream and taken as int32;
//   2. edges_kernel, one lane per note: f0 = int(start * fps), f1 = int(end * fps) in float64 (one product each, the
//      0.05 s rule applied first), then two return-less int32 vector atomics, +velocity at (pitch, f0) and -velocity at
//      (pitch, f1); the second is skipped when f1 == F, where the row ends.  A note of another roll never meets these
//      cells, and integer adds commute, so the cells do not depend on the order the atomics arrive in;
//   3. scan_kernel, one workgroup of 256 lanes per (roll, pitch row): an inclusive add-scan of the row in place, in tiles
//      of 1024 columns, four consecutive columns per lane (one 16-byte load and store where the row's base is 16-byte
//      aligned, four 4-byte ones otherwise and in the row's last, partial group of four): the lane's running sums, the
//      wave's scan of the lane totals by shuffles, the four wave totals through LDS (two sets, used in turn, so one
//      barrier per tile is enough), the tiles before in a register.  The cell is read as int32 and written back as the
//      float32 of the sum at the same address -- every sum is an integer below 2^24 (mt3_hip.h), so the float is exact.
//      A row is read once and written once: 8 bytes per cell, bound by memory.
// The per-roll tables (first note, number of notes, first cell, width) ride in the kernel arguments, 128 rolls per
// launch, so the call copies nothing: blockIdx.y is the roll, its table entry a uniform load.
//
// counts_kernel, grid (column blocks, pairs): a workgroup strides over blocks of 256 columns and walks the 128 rows of
// each, so a wave reads 256 contiguous bytes per roll and row; a column at or past a roll's own width reads as 0.  Each
// wave counts its three conditions with __ballot + __popcll (scalar work beside the loads), the four waves meet in LDS,
// and lanes 0..2 make one 64-bit atomic add each.  Counts are integers: the result does not depend on the order either.
// Plain vector loads, stores and atomics only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "device.h"
#include "mt3_hip.h"

#pragma clang fp contract(off)          // int(x * fps) is ONE rounded product, as Python evaluates it

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerLane = 4;
constexpr int kTile = kThreads * kPerLane;
constexpr int kPitches = MT3_PIANOROLL_PITCHES;
constexpr int kPerLaunch = 128;                      // rolls (pairs) whose tables fit one launch's arguments
constexpr int kMaxCountBlocks = 1024;                // column blocks per pair; wider pairs stride
constexpr int32_t kMaxThreshold = 1 << 24;

struct RollTable {                                   // 3 KiB by value
  int64_t cell0[kPerLaunch];                         // the roll's first cell in d_out, in floats
  int64_t note0[kPerLaunch];
  int32_t notes[kPerLaunch];
  int32_t width[kPerLaunch];
};

struct PairTable {                                   // 3 KiB by value
  int64_t ref0[kPerLaunch], est0[kPerLaunch];
  int32_t ref_w[kPerLaunch], est_w[kPerLaunch];
};

// int(x * fps) cut to [0, F]; NaN and negative products: 0
__device__ __forceinline__ int32_t frame_of(double t, double fps, int32_t F) {
  const double y = t * fps;
  if (!(y >= 0.0)) return 0;
  if (y >= static_cast<double>(F)) return F;
  return static_cast<int32_t>(y);
}

__global__ __launch_bounds__(kThreads) void edges_kernel(RollTable t, const double* __restrict__ start,
                                                         const double* __restrict__ end,
                                                         const int32_t* __restrict__ pitch,
                                                         const int32_t* __restrict__ velocity,
                                                         const int32_t* __restrict__ drum, double fps, int32_t is_drum,
                                                         int32_t* out) {
  const int r = blockIdx.y;
  const int32_t F = t.width[r];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (F == 0 || i >= t.notes[r]) return;
  const int64_t g = t.note0[r] + i;
  const int32_t p = pitch[g];
  if (static_cast<uint32_t>(p) >= static_cast<uint32_t>(kPitches)) return;
  if (!is_drum && drum[g]) return;
  const double s = start[g];
  double e = end[g];
  if (is_drum || e - s < MT3_PIANOROLL_MIN_NOTE_SECONDS) e = s + MT3_PIANOROLL_MIN_NOTE_SECONDS;
  const int32_t f0 = frame_of(s, fps, F), f1 = frame_of(e, fps, F);
  if (f1 <= f0) return;                              // f0 < f1 <= F from here on
  const int32_t v = velocity[g];
  int32_t* row = out + t.cell0[r] + static_cast<int64_t>(p) * F;
  (void)__hip_atomic_fetch_add(row + f0, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (f1 < F) (void)__hip_atomic_fetch_add(row + f1, -v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (128 pitch rows, rolls): the row's int32 edges -> the float32 of their running sums, in place
__global__ __launch_bounds__(kThreads) void scan_kernel(RollTable t, int32_t* out) {
  __shared__ int s_sum[2][kWaves];
  const int r = blockIdx.y;
  const int32_t F = t.width[r];
  if (F == 0) return;
  const int tid = threadIdx.x;
  int32_t* row = out + t.cell0[r] + static_cast<int64_t>(blockIdx.x) * F;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  int carry = 0, set = 0;                            // uniform over the workgroup
  for (int64_t base = 0; base < F; base += kTile, set ^= 1) {
    const int64_t at = base + tid * kPerLane;
    const bool whole = vec && at + kPerLane <= F;
    int x[kPerLane];
    if (whole) {
      const int4 v = *reinterpret_cast<const int4*>(row + at);
      x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) x[j] = at + j < F ? row[at + j] : 0;
    }
    x[1] += x[0], x[2] += x[1], x[3] += x[2];
    int before, total;                               // the set of the tile before may still be read: this one is the other
    mt3k::block_scan_add<kWaves>(x[3], s_sum[set], &before, &total);
    before += carry;
    carry += total;
    if (whole) {
      int4 v;
      v.x = __float_as_int(static_cast<float>(x[0] + before));
      v.y = __float_as_int(static_cast<float>(x[1] + before));
      v.z = __float_as_int(static_cast<float>(x[2] + before));
      v.w = __float_as_int(static_cast<float>(x[3] + before));
      *reinterpret_cast<int4*>(row + at) = v;
    } else {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j)
        if (at + j < F) row[at + j] = __float_as_int(static_cast<float>(x[j] + before));
    }
  }
}

// grid (column blocks, pairs): counts [pair][3] += (TP, FP, FN) of this workgroup's columns
__global__ __launch_bounds__(kThreads) void counts_kernel(PairTable t, const float* __restrict__ rolls, float threshold,
                                                          unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_cnt[kWaves][3];
  const int pr = blockIdx.y;
  const int32_t Fr = t.ref_w[pr], Fe = t.est_w[pr], F = max(Fr, Fe);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* ref = rolls + t.ref0[pr];
  const float* est = rolls + t.est0[pr];
  unsigned long long tp = 0, fp = 0, fn = 0;         // uniform over the wave
  for (int64_t c0 = static_cast<int64_t>(blockIdx.x) * kThreads; c0 < F; c0 += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int64_t c = c0 + tid;                      // every lane of the wave stays in the loop for the ballots
    const bool in_r = c < Fr, in_e = c < Fe;
#pragma unroll 4
    for (int p = 0; p < kPitches; ++p) {
      const float rv = in_r ? ref[static_cast<int64_t>(p) * Fr + c] : 0.f;
      const float ev = in_e ? est[static_cast<int64_t>(p) * Fe + c] : 0.f;
      const bool r_on = rv > threshold, e_on = ev > 0.f;
      tp += __popcll(__ballot(r_on && e_on));
      fp += __popcll(__ballot(!r_on && e_on));
      fn += __popcll(__ballot(r_on && !e_on));
    }
  }
  if (lane == 0) s_cnt[wave][0] = tp, s_cnt[wave][1] = fp, s_cnt[wave][2] = fn;
  __syncthreads();
  if (tid < 3) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += s_cnt[w][tid];
    if (sum) atomicAdd(&counts[static_cast<size_t>(pr) * 3 + tid], sum);
  }
}

constexpr int64_t kMaxCells = INT64_MAX / 8;         // every cell index times 4 bytes stays inside int64

// the cells [first, last) of a roll of `width` columns at column offset `col`; false where the arithmetic would leave int64
bool roll_cells(int64_t col, int32_t width, int64_t* first, int64_t* last) {
  if (col < 0 || width < 0 || col > kMaxCells / kPitches - width) return false;
  *first = col * kPitches;
  *last = (col + width) * kPitches;
  return true;
}

}  // namespace

extern "C" int mt3_op_pianoroll(const double* d_start, const double* d_end, const int32_t* d_pitch,
                                const int32_t* d_velocity, const int32_t* d_is_drum, int64_t n_notes, int32_t n_rolls,
                                const int64_t* h_note_offsets, const int64_t* h_col_offsets, const int32_t* h_widths,
                                double fps, int32_t is_drum, float* d_out, int64_t out_capacity, void* stream) {
  const std::string who = "mt3_op_pianoroll: ";
  if (n_rolls < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_rolls must not be negative");
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (!std::isfinite(fps) || !(fps > 0.0)) return mt3::fail(MT3_ERR_INVALID, who + "fps must be finite and positive");
  if (out_capacity < 0) return mt3::fail(MT3_ERR_INVALID, who + "out_capacity must not be negative");
  if (n_rolls == 0) return MT3_OK;
  if (!h_note_offsets || !h_col_offsets || !h_widths) return mt3::fail(MT3_ERR_INVALID, who + "null table");
  if (n_notes > 0 && (!d_start || !d_end || !d_pitch || !d_velocity || !d_is_drum))
    return mt3::fail(MT3_ERR_INVALID, who + "null note array");
  if (h_note_offsets[0] < 0 || h_note_offsets[n_rolls] > n_notes)
    return mt3::fail(MT3_ERR_INVALID, who + "h_note_offsets must lie inside [0, n_notes]");
  int64_t span0 = 0, span1 = 0;
  for (int32_t i = 0; i < n_rolls; ++i) {
    const int64_t cnt = h_note_offsets[i + 1] - h_note_offsets[i];
    if (h_note_offsets[i + 1] < h_note_offsets[i]) return mt3::fail(MT3_ERR_INVALID, who + "h_note_offsets must not decrease");
    if (cnt > INT32_MAX) return mt3::fail(MT3_ERR_INVALID, who + "more than 2^31 - 1 notes in one roll");
    if (h_widths[i] < 0) return mt3::fail(MT3_ERR_INVALID, who + "negative width");
    int64_t first, last;
    if (!roll_cells(h_col_offsets[i], h_widths[i], &first, &last))
      return mt3::fail(MT3_ERR_INVALID, who + "column offset negative or too large");
    if (i == 0) span0 = first;
    if (first < span1) return mt3::fail(MT3_ERR_INVALID, who + "h_col_offsets: rolls overlap or are out of order");
    span1 = last;
  }
  if (span1 > out_capacity) return mt3::fail(MT3_ERR_INVALID, who + "the rolls end past out_capacity");
  if (span1 == span0) return MT3_OK;
  if (!d_out) return mt3::fail(MT3_ERR_INVALID, who + "null d_out");

  hipStream_t s = static_cast<hipStream_t>(stream);
  int32_t* out = reinterpret_cast<int32_t*>(d_out);
  MT3_HIP_CHECK(hipMemsetAsync(out + span0, 0, static_cast<size_t>(span1 - span0) * sizeof(int32_t), s));
  for (int32_t r0 = 0; r0 < n_rolls; r0 += kPerLaunch) {
    const int n = n_rolls - r0 < kPerLaunch ? n_rolls - r0 : kPerLaunch;
    RollTable t{};
    int32_t most = 0, widest = 0;
    for (int j = 0; j < n; ++j) {
      t.cell0[j] = h_col_offsets[r0 + j] * kPitches;
      t.note0[j] = h_note_offsets[r0 + j];
      t.notes[j] = static_cast<int32_t>(h_note_offsets[r0 + j + 1] - h_note_offsets[r0 + j]);
      t.width[j] = h_widths[r0 + j];
      if (t.width[j] > 0 && t.notes[j] > most) most = t.notes[j];
      if (t.width[j] > widest) widest = t.width[j];
    }
    if (widest == 0) continue;
    if (most > 0) {
      const uint32_t blocks = static_cast<uint32_t>((static_cast<int64_t>(most) + kThreads - 1) / kThreads);
      hipLaunchKernelGGL(edges_kernel, dim3(blocks, static_cast<uint32_t>(n)), dim3(kThreads), 0, s, t, d_start, d_end,
                         d_pitch, d_velocity, d_is_drum, fps, is_drum, out);
      MT3_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(scan_kernel, dim3(kPitches, static_cast<uint32_t>(n)), dim3(kThreads), 0, s, t, out);
      MT3_HIP_CHECK(hipGetLastError());
    }                                                // no notes in the piece: its rolls are the memset's zeros, +0.0f
  }
  return MT3_OK;
}

extern "C" int mt3_op_frame_counts(const float* d_rolls, int64_t rolls_capacity, int32_t n_pairs,
                                   const int64_t* h_ref_col_offsets, const int32_t* h_ref_widths,
                                   const int64_t* h_est_col_offsets, const int32_t* h_est_widths,
                                   int32_t velocity_threshold, uint64_t* d_counts, void* stream) {
  const std::string who = "mt3_op_frame_counts: ";
  if (n_pairs < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_pairs must not be negative");
  if (rolls_capacity < 0) return mt3::fail(MT3_ERR_INVALID, who + "rolls_capacity must not be negative");
  if (velocity_threshold > kMaxThreshold || velocity_threshold < -kMaxThreshold)
    return mt3::fail(MT3_ERR_INVALID, who + "velocity_threshold must be within +-2^24");
  if (n_pairs == 0) return MT3_OK;
  if (!h_ref_col_offsets || !h_ref_widths || !h_est_col_offsets || !h_est_widths)
    return mt3::fail(MT3_ERR_INVALID, who + "null table");
  if (!d_counts) return mt3::fail(MT3_ERR_INVALID, who + "null d_counts");
  bool any = false;
  for (int32_t i = 0; i < n_pairs; ++i) {
    int64_t first, last;
    if (!roll_cells(h_ref_col_offsets[i], h_ref_widths[i], &first, &last) || last > rolls_capacity)
      return mt3::fail(MT3_ERR_INVALID, who + "a reference roll: negative width or column offset, or past rolls_capacity");
    if (!roll_cells(h_est_col_offsets[i], h_est_widths[i], &first, &last) || last > rolls_capacity)
      return mt3::fail(MT3_ERR_INVALID, who + "an estimated roll: negative width or column offset, or past rolls_capacity");
    any = any || h_ref_widths[i] > 0 || h_est_widths[i] > 0;
  }
  if (any && !d_rolls) return mt3::fail(MT3_ERR_INVALID, who + "null d_rolls");

  hipStream_t s = static_cast<hipStream_t>(stream);
  MT3_HIP_CHECK(hipMemsetAsync(d_counts, 0, static_cast<size_t>(n_pairs) * 3 * sizeof(uint64_t), s));
  for (int32_t p0 = 0; p0 < n_pairs; p0 += kPerLaunch) {
    const int n = n_pairs - p0 < kPerLaunch ? n_pairs - p0 : kPerLaunch;
    PairTable t{};
    int32_t widest = 0;
    for (int j = 0; j < n; ++j) {
      t.ref0[j] = h_ref_col_offsets[p0 + j] * kPitches;
      t.est0[j] = h_est_col_offsets[p0 + j] * kPitches;
      t.ref_w[j] = h_ref_widths[p0 + j];
      t.est_w[j] = h_est_widths[p0 + j];
      if (t.ref_w[j] > widest) widest = t.ref_w[j];
      if (t.est_w[j] > widest) widest = t.est_w[j];
    }
    if (widest == 0) continue;
    int64_t blocks = (static_cast<int64_t>(widest) + kThreads - 1) / kThreads;
    if (blocks > kMaxCountBlocks) blocks = kMaxCountBlocks;
    hipLaunchKernelGGL(counts_kernel, dim3(static_cast<uint32_t>(blocks), static_cast<uint32_t>(n)), dim3(kThreads), 0, s, t,
                       d_rolls, static_cast<float>(velocity_threshold),
                       reinterpret_cast<unsigned long long*>(d_counts) + static_cast<size_t>(p0) * 3);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}
