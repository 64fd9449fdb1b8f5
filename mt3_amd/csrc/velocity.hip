// Note velocities for gfx950 from the float32 log-mel the frontend has already written on the device: a level per note
// (mt3_op_note_levels), then per (file, group) an anchor by rank and a velocity per note by a threshold table
// (mt3_op_level_velocities).  The rule: include/mt3_hip.h, "note velocities"; its statement in numpy:
// mt3_amd/velocity.py, levels_reference / velocities_reference.
//
// Levels: a note's window frames are spread over a group of 8 lanes (lane j takes frames frame + j, frame + j + 8, ...),
// 32 notes per workgroup of 256 lanes.  A lane gathers its frame's bins from one log-mel row -- float32 values widened to
// float64 and added left to right in table order, then ONE division by the count -- and keeps the largest sum that is
// not NaN; the 8 lanes then reduce that maximum with three xor moves inside the wave.  Every lane of a wave reaches the
// moves: a lane without a note or without a frame carries NaN, which the maximum skips.  No atomics.
//
// Velocities: one workgroup of 256 lanes per (file, group) over the group's contiguous notes.  The member of ascending
// rank r is found by a radix select on the order-preserving 64-bit image of the level, 8 passes of 8 bits from the top:
// a pass counts, with integer LDS atomics, the measured levels that share the prefix found so far into 256 bins (strided
// loop: a group of any size), a workgroup sum-scan over the bins finds the one that holds rank r, and r becomes the
// rank inside it.  The first pass's total is the measured count n, which gives r = floor(quantile * (n - 1)).  The
// counts are integers, so the order of the atomics does not show.  Then every note: d = level - anchor, and the number
// of thresholds <= d by binary search in the ascending table.
//
// 64 files per launch (their table rides in the kernel arguments), the launches one after the other on the stream.
// Plain vector loads and stores only; global memory sees no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "device.h"
#include "mt3_hip.h"

namespace {

constexpr int kLanes = 256;                          // lanes of a workgroup, both kernels
constexpr int kWaves = kLanes / 64;
constexpr int kGroup = 8;                            // lanes that share a note's window
constexpr int kNotesPerGroup = kLanes / kGroup;      // notes per workgroup of the levels kernel
constexpr int kPerLaunch = 64;                       // files whose table fits one launch's arguments
constexpr int kKeys = MT3_VELOCITY_KEYS;             // rows of the bin table: 128 pitches and the drum row
constexpr int kThresholds = MT3_VELOCITY_THRESHOLDS;

struct VelocityTable {                               // 64 * 28 bytes by value
  int64_t first[kPerLaunch], row0[kPerLaunch];
  int32_t n_notes[kPerLaunch], n_pitched[kPerLaunch], n_frames[kPerLaunch];
};
static_assert(sizeof(VelocityTable) <= 2048, "the table of one launch stays within 2 KiB of kernel arguments");

// the larger of two sums, NaN skipped: np.fmax
__device__ __forceinline__ double fmax_skip(double a, double b) { return (b == b && (a != a || b > a)) ? b : a; }

// the order-preserving image of a double that is not NaN: a < b  <=>  image(a) < image(b) (-0.0 just below +0.0)
__device__ __forceinline__ uint64_t image_of(double v) {
  const uint64_t u = static_cast<uint64_t>(__double_as_longlong(v));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double(static_cast<long long>(u));
}

// notes [note0, note0 + n_here) of the job, the files t.* among them: 32 notes per workgroup
__global__ __launch_bounds__(kLanes) void note_levels_kernel(
    VelocityTable t, int n_files, int64_t note0, int64_t n_here, const float* __restrict__ d_logmel, int n_mel,
    const int32_t* __restrict__ d_frame, const int32_t* __restrict__ d_key, const int32_t* __restrict__ d_bin_first,
    const int32_t* __restrict__ d_bins, int n_bins, int window, double* __restrict__ d_level) {
  const int j = threadIdx.x & (kGroup - 1);
  const int64_t local = static_cast<int64_t>(blockIdx.x) * kNotesPerGroup + (threadIdx.x / kGroup);
  const bool has_note = local < n_here;
  const int64_t i = note0 + local;
  double best = NAN;
  bool in_file = false;
  if (has_note) {
    // the note's file: the last one of the launch whose first note is not after it (files lie in order, back to back
    // or with gaps; a note in a gap belongs to no file and is not written)
    int lo = 0, hi = n_files;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (t.first[mid] <= i) lo = mid; else hi = mid;
    }
    in_file = i >= t.first[lo] && i - t.first[lo] < t.n_notes[lo];
    const int64_t n_frames = in_file ? t.n_frames[lo] : 0;
    const int64_t frame = d_frame[i];
    const int32_t key = d_key[i];
    int32_t b0 = 0, b1 = 0;
    if (key >= 0 && key < kKeys) b0 = d_bin_first[key], b1 = d_bin_first[key + 1];
    if (b0 < 0 || b1 > n_bins || b1 < b0) b1 = b0 = 0;                  // a table that is not the checked one: no bins
    if (frame >= 0 && frame < n_frames && b1 > b0) {
      const double count = static_cast<double>(b1 - b0);
      const int64_t end = frame + window < n_frames ? frame + window : n_frames;
      for (int64_t g = frame + j; g < end; g += kGroup) {
        const float* row = d_logmel + (t.row0[lo] + g) * n_mel;         // a row of the file's own: g < n_frames
        double s = 0.0;
        for (int32_t b = b0; b < b1; ++b) {
          const uint32_t bin = static_cast<uint32_t>(d_bins[b]);
          s += bin < static_cast<uint32_t>(n_mel) ? static_cast<double>(row[bin]) : static_cast<double>(NAN);
        }
        best = fmax_skip(best, s / count);
      }
    }
  }
  // the 8 lanes of a note are 8 neighbours of one wave
#pragma unroll
  for (int o = 1; o < kGroup; o <<= 1) best = fmax_skip(best, __shfl_xor(best, o));
  if (in_file && j == 0) d_level[i] = best;
}

// workgroup b: group (b & 1) of file (b >> 1) of the launch
__global__ __launch_bounds__(kLanes) void level_velocities_kernel(
    VelocityTable t, const double* __restrict__ d_level, double quantile, const double* __restrict__ d_th,
    const int32_t* __restrict__ d_velocity_in, int32_t* __restrict__ d_velocity, double* __restrict__ d_anchor,
    int32_t* __restrict__ d_measured) {
  __shared__ int s_hist[kLanes];
  __shared__ int s_scan[kWaves];
  __shared__ int s_pick[2];                          // the bin that holds the rank, and the members before it
  __shared__ double s_th[kThresholds];
  const int tid = threadIdx.x;
  const int f = blockIdx.x >> 1, group = blockIdx.x & 1;
  const int64_t a = t.first[f] + (group ? t.n_pitched[f] : 0);
  const int64_t n = group ? t.n_notes[f] - t.n_pitched[f] : t.n_pitched[f];
  if (tid < kThresholds) s_th[tid] = d_th[tid];

  uint64_t prefix = 0;                               // the top bits of the anchor's image found so far; uniform
  int64_t rank = 0;
  int measured = 0;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    s_hist[tid] = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += kLanes) {
      const double v = d_level[a + i];
      if (v != v) continue;
      const uint64_t k = image_of(v);
      if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1);
    }
    __syncthreads();
    const int mine = s_hist[tid];
    int before, total;
    mt3k::block_scan_add<kWaves>(mine, s_scan, &before, &total);
    if (pass == 0) {
      measured = total;
      if (measured == 0) break;                      // uniform: every lane holds the same total
      rank = static_cast<int64_t>(floor(quantile * static_cast<double>(measured - 1)));
      rank = rank < 0 ? 0 : rank > measured - 1 ? measured - 1 : rank;
    }
    if (before <= rank && rank < static_cast<int64_t>(before) + mine) s_pick[0] = tid, s_pick[1] = before;   // one lane
    __syncthreads();
    prefix = (prefix << 8) | static_cast<uint64_t>(s_pick[0]);
    rank -= s_pick[1];
    // s_hist, s_scan and s_pick are written again only after the next pass's first barrier
  }

  const double anchor = measured ? value_of(prefix) : static_cast<double>(NAN);
  if (tid == 0) d_anchor[blockIdx.x] = anchor, d_measured[blockIdx.x] = measured;
  __syncthreads();                                   // s_th is whole (also when the loop broke before its barriers)
  for (int64_t i = tid; i < n; i += kLanes) {
    const double v = d_level[a + i];
    int32_t out = d_velocity_in[a + i];
    if (v == v) {
      const double d = v - anchor;
      int lo = 0, hi = kThresholds;                  // the thresholds <= d: th ascends
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d >= s_th[mid]) lo = mid + 1; else hi = mid;
      }
      out = 1 + lo;
    }
    d_velocity[a + i] = out;
  }
}

// what both ops check of the file table, before any device work
int check_files(const std::string& who, const mt3_velocity_file* h_files, int32_t n_files, int64_t n_notes) {
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (n_files > 0 && !h_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table");
  int64_t end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_velocity_file& f = h_files[i];
    if (f.first < 0 || f.n_notes < 0 || f.first > n_notes || f.n_notes > n_notes - f.first)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's note range must lie inside [0, n_notes]");
    if (f.first < end) return mt3::fail(MT3_ERR_INVALID, who + "note ranges overlap or are out of order");
    end = f.first + f.n_notes;
    if (f.n_pitched < 0 || f.n_pitched > f.n_notes)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's n_pitched must lie in 0 .. n_notes");
  }
  return MT3_OK;
}

VelocityTable table_of(const mt3_velocity_file* h_files, int n) {
  VelocityTable t{};
  for (int i = 0; i < n; ++i) {
    const mt3_velocity_file& f = h_files[i];
    t.first[i] = f.first, t.row0[i] = f.row0, t.n_notes[i] = f.n_notes, t.n_pitched[i] = f.n_pitched;
    t.n_frames[i] = f.n_frames;
  }
  return t;
}

}  // namespace

extern "C" int mt3_op_note_levels(const float* d_logmel, int64_t n_rows, int32_t n_mel, const mt3_velocity_file* h_files,
                                  int32_t n_files, const int32_t* d_frame, const int32_t* d_key, int64_t n_notes,
                                  const int32_t* h_bin_first, const int32_t* h_bins, const int32_t* d_bin_first,
                                  const int32_t* d_bins, int32_t n_bins, int32_t window, double* d_level, void* stream) {
  const std::string who = "mt3_op_note_levels: ";
  if (window < 1 || window > MT3_VELOCITY_MAX_WINDOW)
    return mt3::fail(MT3_ERR_INVALID, who + "window must be 1 .. 64 frames");
  if (n_mel < 1 || n_mel > MT3_VELOCITY_MAX_MEL) return mt3::fail(MT3_ERR_INVALID, who + "n_mel must be 1 .. 4096");
  if (n_rows < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_rows must not be negative");
  if (n_bins < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_bins must not be negative");
  if (const int rc = check_files(who, h_files, n_files, n_notes)) return rc;
  if (n_files == 0) return MT3_OK;
  if (!h_bin_first || !d_bin_first) return mt3::fail(MT3_ERR_INVALID, who + "null bin_first (host or device)");
  if (n_bins > 0 && (!h_bins || !d_bins)) return mt3::fail(MT3_ERR_INVALID, who + "null bins (host or device)");
  if (h_bin_first[0] != 0 || h_bin_first[MT3_VELOCITY_KEYS] != n_bins)
    return mt3::fail(MT3_ERR_INVALID, who + "bin_first must rise from 0 to n_bins");
  for (int k = 0; k < MT3_VELOCITY_KEYS; ++k)
    if (h_bin_first[k + 1] < h_bin_first[k]) return mt3::fail(MT3_ERR_INVALID, who + "bin_first must rise from 0 to n_bins");
  for (int32_t b = 0; b < n_bins; ++b)
    if (h_bins[b] < 0 || h_bins[b] >= n_mel) return mt3::fail(MT3_ERR_INVALID, who + "a bin of the table is >= n_mel");
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_velocity_file& f = h_files[i];
    if (f.row0 < 0 || f.n_frames < 0 || f.row0 > n_rows || f.n_frames > n_rows - f.row0)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's rows must lie inside the log-mel's [0, n_rows]");
  }
  if (n_rows > 0 && !d_logmel) return mt3::fail(MT3_ERR_INVALID, who + "null log-mel");
  if (n_notes > 0 && (!d_frame || !d_key)) return mt3::fail(MT3_ERR_INVALID, who + "null note column (frame or key)");
  if (n_notes > 0 && !d_level) return mt3::fail(MT3_ERR_INVALID, who + "null level");

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t p0 = 0; p0 < n_files; p0 += kPerLaunch) {
    const int n = n_files - p0 < kPerLaunch ? n_files - p0 : kPerLaunch;
    const int64_t note0 = h_files[p0].first;
    const int64_t n_here = h_files[p0 + n - 1].first + h_files[p0 + n - 1].n_notes - note0;
    if (n_here == 0) continue;
    const int64_t groups = (n_here + kNotesPerGroup - 1) / kNotesPerGroup;
    if (groups > INT32_MAX) return mt3::fail(MT3_ERR_INVALID, who + "too many notes for one launch");
    hipLaunchKernelGGL(note_levels_kernel, dim3(static_cast<uint32_t>(groups)), dim3(kLanes), 0, s,
                       table_of(h_files + p0, n), n, note0, n_here, d_logmel, static_cast<int>(n_mel), d_frame, d_key,
                       d_bin_first, d_bins, static_cast<int>(n_bins), static_cast<int>(window), d_level);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}

extern "C" int mt3_op_level_velocities(const double* d_level, int64_t n_notes, const mt3_velocity_file* h_files,
                                       int32_t n_files, double quantile, const double* d_th,
                                       const int32_t* d_velocity_in, int32_t* d_velocity, double* d_anchor,
                                       int32_t* d_measured, void* stream) {
  const std::string who = "mt3_op_level_velocities: ";
  if (!(quantile >= 0.0 && quantile <= 1.0)) return mt3::fail(MT3_ERR_INVALID, who + "quantile must lie in [0, 1]");
  if (const int rc = check_files(who, h_files, n_files, n_notes)) return rc;
  if (n_files == 0) return MT3_OK;
  if (n_notes > 0 && (!d_level || !d_velocity_in || !d_velocity))
    return mt3::fail(MT3_ERR_INVALID, who + "null note column (level, velocity_in or velocity)");
  if (!d_th) return mt3::fail(MT3_ERR_INVALID, who + "null thresholds");
  if (!d_anchor || !d_measured) return mt3::fail(MT3_ERR_INVALID, who + "null output (anchor or measured)");

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t p0 = 0; p0 < n_files; p0 += kPerLaunch) {
    const int n = n_files - p0 < kPerLaunch ? n_files - p0 : kPerLaunch;
    hipLaunchKernelGGL(level_velocities_kernel, dim3(static_cast<uint32_t>(2 * n)), dim3(kLanes), 0, s,
                       table_of(h_files + p0, n), d_level, quantile, d_th, d_velocity_in, d_velocity, d_anchor + 2 * p0,
                       d_measured + 2 * p0);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}
