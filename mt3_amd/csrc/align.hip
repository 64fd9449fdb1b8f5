// Shift paths for gfx950: the best time shift per segment of every file of a job (mt3_op_align_paths).  The rule:
// include/mt3_hip.h, "shift paths"; its numpy statement: mt3_amd/alignment.py, best_paths_reference.
//
// One workgroup of 64 lanes (one wave) per file, 64 files per launch (their table and the grid ride in the kernel
// arguments).  Lane j owns shift j: it keeps g_j, reads the row D[s-1][.] and the grid from LDS (every lane reads the
// same word: a broadcast), takes the minimum over k in increasing order -- the lowest k wins on equal values -- and
// writes D[s][j] into the other half of the double-buffered row, one barrier per segment.  The stored k of every
// (segment, shift) goes to the caller's scratch, one byte each, so a file may have any number of segments.  Lane 0 then
// finds the path's end and reads the path back: S dependent one-byte loads.  The kernel is small by nature (a file of
// ten minutes is 293 segments; 293 * 64 * 64 float64 steps per file); it exists so that the score table of a job goes
// from the scoring call to the path without leaving the device.  Plain vector loads and stores only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "mt3_hip.h"

#pragma clang fp contract(off)          // every difference, product and sum of the rule is rounded on its own

namespace {

constexpr int kLanes = MT3_ALIGN_MAX_SHIFTS;         // 64: one wave
constexpr int kPerLaunch = 64;                       // files whose table fits one launch's arguments

struct AlignTable {                                  // 512 + 512 bytes by value
  int32_t first[kPerLaunch], segments[kPerLaunch];
  double grid[kLanes];
};
static_assert(sizeof(AlignTable) <= 1024, "the tables of one launch stay within 1 KiB");

__global__ __launch_bounds__(kLanes) void align_kernel(AlignTable t, const float* __restrict__ scores, int K, double lambda,
                                                       double max_jump, uint8_t* __restrict__ back,
                                                       int32_t* __restrict__ path, double* __restrict__ total) {
  __shared__ double D[2][kLanes];
  __shared__ double g[kLanes];
  const int p = blockIdx.x, j = threadIdx.x;
  const int64_t first = t.first[p];
  const int S = t.segments[p];
  const bool mine = j < K;
  const float* sc = scores + first * K;
  uint8_t* bk = back + first * K;
  const double gj = t.grid[mine ? j : 0];
  g[j] = gj;
  float c = mine ? sc[j] : 0.f;
  D[0][j] = -static_cast<double>(c);
  __syncthreads();
  for (int s = 1; s < S; ++s) {
    const double* prev = D[(s - 1) & 1];
    if (mine) {
      c = sc[static_cast<int64_t>(s) * K + j];
      double best = 0.0;
      int arg = -1;
      for (int k = 0; k < K; ++k) {
        const double jump = fabs(gj - g[k]);
        if (!(jump <= max_jump)) continue;           // k = j always passes: jump 0
        const double v = prev[k] + lambda * jump;
        if (arg < 0 || v < best) best = v, arg = k;
      }
      D[s & 1][j] = -static_cast<double>(c) + best;
      bk[static_cast<int64_t>(s) * K + j] = static_cast<uint8_t>(arg);
    }
    __syncthreads();                                 // the row is complete, and the one before it is free again
  }
  if (j == 0) {
    const double* last = D[(S - 1) & 1];
    int at = 0;
    for (int k = 1; k < K; ++k)
      if (last[k] < last[at]) at = k;
    total[p] = last[at];
    for (int s = S - 1; s > 0; --s) {
      path[first + s] = at;
      at = bk[static_cast<int64_t>(s) * K + at];
      at = at < K ? at : K - 1;                      // (a stored k is always < K; no load may leave the table whatever it reads)
    }
    path[first] = at;
  }
}

}  // namespace

extern "C" int mt3_op_align_paths(const float* d_scores, int32_t total_segments, int32_t K, const int32_t* h_files,
                                  int32_t n_files, const double* h_grid, double smoothness, double max_jump,
                                  uint8_t* d_backptr, int32_t* d_path, double* d_total, void* stream) {
  const std::string who = "mt3_op_align_paths: ";
  if (K < 1 || K > kLanes) return mt3::fail(MT3_ERR_INVALID, who + "K must be 1 .. " + std::to_string(kLanes));
  if (total_segments < 0) return mt3::fail(MT3_ERR_INVALID, who + "total_segments must not be negative");
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (!h_grid) return mt3::fail(MT3_ERR_INVALID, who + "null grid");
  for (int32_t j = 0; j < K; ++j) {
    if (!std::isfinite(h_grid[j])) return mt3::fail(MT3_ERR_INVALID, who + "the grid must be finite");
    if (j && !(h_grid[j] > h_grid[j - 1])) return mt3::fail(MT3_ERR_INVALID, who + "the grid must be strictly increasing");
  }
  if (!(smoothness >= 0.0) || !std::isfinite(smoothness))
    return mt3::fail(MT3_ERR_INVALID, who + "smoothness must be finite and not negative");
  if (!(max_jump >= 0.0)) return mt3::fail(MT3_ERR_INVALID, who + "max_jump must not be negative (INFINITY: unlimited)");
  if (n_files == 0) return MT3_OK;
  if (!h_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table");
  if (!d_scores || !d_backptr || !d_path || !d_total)
    return mt3::fail(MT3_ERR_INVALID, who + "null scores, back-pointer scratch, path or totals");
  int64_t end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const int64_t first = h_files[2 * i], n = h_files[2 * i + 1];
    if (n < 1) return mt3::fail(MT3_ERR_INVALID, who + "a file must have at least 1 segment");
    if (first < 0 || first + n > total_segments)
      return mt3::fail(MT3_ERR_INVALID, who + "a segment range must lie inside [0, total_segments]");
    if (first < end) return mt3::fail(MT3_ERR_INVALID, who + "segment ranges overlap or are out of order");
    end = first + n;
  }

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t p0 = 0; p0 < n_files; p0 += kPerLaunch) {
    const int n = n_files - p0 < kPerLaunch ? n_files - p0 : kPerLaunch;
    AlignTable t{};
    for (int i = 0; i < n; ++i) t.first[i] = h_files[2 * (p0 + i)], t.segments[i] = h_files[2 * (p0 + i) + 1];
    for (int j = 0; j < K; ++j) t.grid[j] = h_grid[j];
    hipLaunchKernelGGL(align_kernel, dim3(static_cast<uint32_t>(n)), dim3(kLanes), 0, s, t, d_scores, K, smoothness,
                       max_jump, d_backptr, d_path, d_total + p0);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}
