// Beat tracking for gfx950: the beats of every file of a job from its onset frames (mt3_op_track_beats), and the notes of a
// job moved onto the beats' grid (mt3_op_snap_notes).  The rules: include/mt3_hip.h, "beats"; their numpy statements:
// mt3_amd/beats.py, track_reference and snap_reference.
//
// mt3_op_track_beats: one workgroup of 256 lanes (4 waves) per file, 32 files per launch (their table rides in the kernel
// arguments).  Everything is integer arithmetic, so no order of the sums matters; the two tables (tempo prior, penalties)
// come from the host.
//   1. counts: one atomicAdd per note into the file's count row (zeroed by the op's memset before the launch); a frame
//      outside [0, F) is skipped, so no column content writes outside the row.
//   2. envelope E[t] = n[t-1] + 2 n[t] + n[t+1] (n clamped to 255) into the file's second row, and its maximum.
//   3. autocorrelation: E goes through LDS in tiles of kTile frames plus a halo of LAG_MAX; wave w owns the 44 lags
//      LAG_MIN + 44 w .. + 43 in 44 int64 registers per lane, lane j takes the frames j, j + 64, ... of the tile (the 64
//      lanes read 64 consecutive words: no bank conflict), and the lanes' sums meet in LDS by 64-bit integer atomics.
//      Lane 0 then takes the lowest lag of maximal A * W.
//   4. the path: every predecessor of frame t lies at least lo frames back, so the file is walked in blocks of lo frames
//      whose frames do not depend on each other, one barrier per block.  A frame gets a group of G lanes (G = the largest
//      power of two with lo * G <= 256; 2 .. 16), lane q of the group takes the lags lo + q, lo + q + G, ... in ascending
//      order and the group's lanes are folded by xor-shuffles -- higher value first, then the lower lag.  The last
//      kRing = 512 values of C live in an LDS ring: a block reads t - hi .. t - lo and writes t, and lo + hi - 1 <= 499 <
//      512 keeps the two apart.  pen sits beside it.  The back pointers (uint16: hi <= 400) go to global scratch.
//   5. lane 0 finds the path's end among the ring's last p values and reads the path back: dependent two-byte loads, like
//      the read-back of align.hip.  A stored step is always in lo .. t; the walk stops at anything else.
// Plain vector loads and stores and integer atomics only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "mt3_hip.h"

#pragma clang fp contract(off)          // mt3_op_snap_notes: every float64 operation of the rule is rounded on its own

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerLaunch = 32;                        // files whose table fits one launch's arguments
constexpr int kLagMin = MT3_BEATS_LAG_MIN, kLagMax = MT3_BEATS_LAG_MAX;
constexpr int kLags = kLagMax - kLagMin + 1;          // 176
constexpr int kLagsPerWave = kLags / kWaves;          // 44
constexpr int kTile = MT3_BEATS_TILE;                 // frames of E per autocorrelation tile
constexpr int kRing = 512;                            // > lo + hi - 1 for every period
constexpr int kPenStride = MT3_BEATS_PEN_STRIDE;      // 301
static_assert(kLags % kWaves == 0, "every wave owns the same number of lags");
static_assert(kTile % 64 == 0, "a lane's frames are 64 apart");
static_assert((kLagMax + 1) / 2 + 2 * kLagMax - 1 < kRing, "a block's writes stay clear of its reads in the ring");
static_assert(2 * kLagMax - (kLagMax + 1) / 2 + 1 == kPenStride, "pen rows hold lo .. hi of the longest period");

struct BeatsTable {                                   // 32 * 32 bytes by value
  int64_t first[kPerLaunch], frame0[kPerLaunch], beat0[kPerLaunch];
  int32_t n_notes[kPerLaunch], n_frames[kPerLaunch];
};
static_assert(sizeof(BeatsTable) <= 1024, "the table of one launch stays within 1 KiB");

__global__ __launch_bounds__(kThreads) void track_kernel(
    BeatsTable tab, const int32_t* __restrict__ d_frames, const int64_t* __restrict__ d_prior,
    const int64_t* __restrict__ d_pen, int32_t* d_rows, int64_t total_frames, uint16_t* d_back,
    int32_t* __restrict__ d_period, int32_t* __restrict__ d_n_beats, int32_t* __restrict__ d_beats,
    int64_t* __restrict__ d_score) {
  __shared__ int32_t s_e[kTile + kLagMax];
  __shared__ unsigned long long s_a[kLags];
  __shared__ int64_t s_ring[kRing];
  __shared__ int64_t s_pen[kPenStride];
  __shared__ int32_t s_max[kWaves];
  __shared__ int32_t s_period;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int file = blockIdx.x;
  const int32_t F = tab.n_frames[file];
  const int32_t n_notes = tab.n_notes[file];
  const int32_t* frames = d_frames + tab.first[file];
  int32_t* count = d_rows + tab.frame0[file];                  // [F] onsets per frame
  int32_t* env = d_rows + total_frames + tab.frame0[file];     // [F] E
  uint16_t* back = d_back + tab.frame0[file];                  // [F]
  int32_t* beats = d_beats + tab.beat0[file];                  // [F / 13 + 2]

  // ---- 1: onsets per frame
  for (int32_t i = tid; i < n_notes; i += kThreads) {
    const int32_t f = frames[i];
    if (f >= 0 && f < F) atomicAdd(&count[f], 1);
  }
  __syncthreads();

  // ---- 2: the envelope and its peak
  int32_t mine = 0;
  for (int32_t t = tid; t < F; t += kThreads) {
    const int32_t a = t > 0 ? min(count[t - 1], 255) : 0;
    const int32_t b = min(count[t], 255);
    const int32_t c = t + 1 < F ? min(count[t + 1], 255) : 0;
    const int32_t e = a + 2 * b + c;
    env[t] = e;
    mine = max(mine, e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine = max(mine, __shfl_xor(mine, o));
  if (lane == 0) s_max[wave] = mine;
  if (tid < kLags) s_a[tid] = 0;
  __syncthreads();                                             // env is written; s_max and s_a are set
  int32_t peak = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) peak = max(peak, s_max[w]);
  if (peak == 0) {                                             // no onset inside the file (F == 0 among them): uniform
    if (tid == 0) d_period[file] = 0, d_n_beats[file] = 0, d_score[file] = 0;
    return;
  }

  // ---- 3: A[l] = sum over t of E[t] * E[t + l], and the period
  {
    unsigned long long acc[kLagsPerWave];
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j) acc[j] = 0;
    const int lag0 = kLagMin + wave * kLagsPerWave;
    for (int32_t t0 = 0; t0 < F; t0 += kTile) {
      for (int i = tid; i < kTile + kLagMax; i += kThreads) s_e[i] = t0 + i < F ? env[t0 + i] : 0;
      __syncthreads();
      for (int t = lane; t < kTile; t += 64) {
        const uint32_t e = static_cast<uint32_t>(s_e[t]);
#pragma unroll
        for (int j = 0; j < kLagsPerWave; ++j)
          acc[j] += static_cast<unsigned long long>(e) * static_cast<uint32_t>(s_e[t + lag0 + j]);
      }
      __syncthreads();                                         // the tile is free again
    }
#pragma unroll
    for (int j = 0; j < kLagsPerWave; ++j)
      if (acc[j]) atomicAdd(&s_a[wave * kLagsPerWave + j], acc[j]);
    __syncthreads();
    if (tid == 0) {
      int64_t best = 0;
      int32_t arg = 0;
      for (int l = 0; l < kLags; ++l) {
        const int64_t v = static_cast<int64_t>(s_a[l]) * d_prior[l];
        if (v > best) best = v, arg = kLagMin + l;             // strictly greater: the lowest lag of the maximal ones
      }
      s_period = arg;
    }
    __syncthreads();
  }
  const int32_t p = s_period;
  if (p == 0) {                                                // every product is 0: uniform
    if (tid == 0) d_period[file] = 0, d_n_beats[file] = 0, d_score[file] = 0;
    return;
  }

  // ---- 4: the path
  const int32_t lo = (p + 1) / 2, hi = 2 * p;
  for (int i = tid; i <= hi - lo; i += kThreads) s_pen[i] = d_pen[static_cast<int64_t>(p - kLagMin) * kPenStride + i];
  int G = 2;                                                   // lanes per frame: lo * G <= 256, lo <= 100
  while (G < 16 && lo * G * 2 <= kThreads) G *= 2;
  const int j = tid / G, q = tid % G;
  const bool in_block = j < lo;
  __syncthreads();                                             // s_pen is written
  for (int32_t b = 0; b < F; b += lo) {
    const int32_t t = b + j;
    const bool live = in_block && t < F;
    int64_t best = INT64_MIN;
    int32_t arg = 0;
    int32_t e = 0;
    if (live) {
      if (q == 0) e = env[t];
      const int32_t last = min(hi, t);
      for (int32_t l = lo + q; l <= last; l += G) {
        const int64_t v = s_ring[(t - l) & (kRing - 1)] - s_pen[l - lo];
        if (v > best) best = v, arg = l;                       // ascending l: the lowest of the lane's maximal ones
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {                     // the group's lanes lie side by side inside one wave
      const int64_t v = __shfl_xor(best, o);
      const int32_t a = __shfl_xor(arg, o);
      if (v > best || (v == best && a != 0 && a < arg)) best = v, arg = a;
    }
    if (live && q == 0) {
      const int64_t s = static_cast<int64_t>((static_cast<uint32_t>(e) << 16) / static_cast<uint32_t>(peak));
      const bool taken = arg != 0 && best > 0;
      s_ring[t & (kRing - 1)] = s + (taken ? best : 0);
      back[t] = static_cast<uint16_t>(taken ? arg : 0);
    }
    __syncthreads();                                           // the block's C is in the ring, its steps are in `back`
  }

  // ---- 5: the path's end and the beats
  if (tid == 0) {
    int32_t at = max(F - p, 0);
    int64_t score = s_ring[at & (kRing - 1)];
    for (int32_t t = at + 1; t < F; ++t)
      if (s_ring[t & (kRing - 1)] > score) score = s_ring[t & (kRing - 1)], at = t;
    const int32_t room = F / ((kLagMin + 1) / 2) + 2;
    int32_t n = 1;
    for (int32_t t = at; n < room;) {                          // how many beats
      const int32_t l = back[t];
      if (l < lo || l > t) break;                              // 0 ends the path; nothing else is ever stored
      t -= l, ++n;
    }
    int32_t t = at;
    for (int32_t k = n - 1; k >= 0; --k) {
      beats[k] = t;
      t -= back[t];
    }
    d_period[file] = p, d_n_beats[file] = n, d_score[file] = score;
  }
}

struct SnapTable {                                    // 32 * 24 bytes by value
  int64_t first[kPerLaunch], beat0[kPerLaunch];
  int32_t n_notes[kPerLaunch], n_beats[kPerLaunch];
};

struct Step {
  int32_t i;
  double k;
};

__device__ __forceinline__ double beat_time(const int32_t* frames, int32_t i) {
  return static_cast<double>(frames[i]) / static_cast<double>(MT3_BEATS_FPS);
}

// the last beat at or before t, kept within 0 .. n - 2, and the nearest grid step of its interval (the lower on a tie)
__device__ __forceinline__ Step snap_step(const int32_t* frames, int32_t n, double t, double sub) {
  int32_t a = 0, b = n;                               // the first beat > t
  while (a < b) {
    const int32_t m = (a + b) >> 1;
    if (beat_time(frames, m) <= t) a = m + 1; else b = m;
  }
  const int32_t i = min(max(a - 1, 0), n - 2);
  const double b0 = beat_time(frames, i), b1 = beat_time(frames, i + 1);
  return {i, ceil(((t - b0) / (b1 - b0)) * sub - 0.5)};
}

__device__ __forceinline__ double snap_point(const int32_t* frames, Step s, double sub) {
  const double b0 = beat_time(frames, s.i), b1 = beat_time(frames, s.i + 1);
  return s.k == sub ? b1 : b0 + (s.k / sub) * (b1 - b0);
}

__global__ __launch_bounds__(kThreads) void snap_kernel(SnapTable tab, const double* __restrict__ d_start,
                                                        const double* __restrict__ d_end,
                                                        const int32_t* __restrict__ d_beat_frames, double sub,
                                                        double* __restrict__ d_out_start, double* __restrict__ d_out_end) {
  const int file = blockIdx.x;
  const int64_t first = tab.first[file];
  const int32_t n = tab.n_notes[file], n_beats = tab.n_beats[file];
  const int32_t* frames = d_beat_frames + tab.beat0[file];
  for (int32_t i = threadIdx.x; i < n; i += kThreads) {
    double start = d_start[first + i], end = d_end[first + i];
    if (n_beats >= 2) {
      const Step s = snap_step(frames, n_beats, start, sub);
      start = snap_point(frames, s, sub);
      end = snap_point(frames, snap_step(frames, n_beats, end, sub), sub);
      if (end <= start) end = snap_point(frames, Step{s.i, s.k + 1.0}, sub);
    }
    d_out_start[first + i] = start;
    d_out_end[first + i] = end;
  }
}

}  // namespace

extern "C" int mt3_op_track_beats(const int32_t* d_frames, int64_t n_notes, const mt3_beats_file* h_files, int32_t n_files,
                                  const int64_t* d_prior, int32_t n_prior, const int64_t* d_penalties, int32_t n_penalties,
                                  int32_t* d_rows, uint16_t* d_back, int64_t total_frames, int32_t* d_period,
                                  int32_t* d_n_beats, int32_t* d_beats, int64_t total_beats, int64_t* d_score,
                                  void* stream) {
  const std::string who = "mt3_op_track_beats: ";
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (total_frames < 0 || total_beats < 0)
    return mt3::fail(MT3_ERR_INVALID, who + "total_frames and total_beats must not be negative");
  if (n_prior != kLags)
    return mt3::fail(MT3_ERR_INVALID, who + "the prior table holds " + std::to_string(kLags) + " lags");
  if (n_penalties != kLags * kPenStride)
    return mt3::fail(MT3_ERR_INVALID, who + "the penalty table holds " + std::to_string(kLags) + " rows of " +
                                          std::to_string(kPenStride));
  if (n_files == 0) return MT3_OK;
  if (!h_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table");
  if (!d_prior || !d_penalties) return mt3::fail(MT3_ERR_INVALID, who + "null prior or penalty table");
  if (!d_period || !d_n_beats || !d_score) return mt3::fail(MT3_ERR_INVALID, who + "null period, n_beats or score");
  if (n_notes > 0 && !d_frames) return mt3::fail(MT3_ERR_INVALID, who + "null onset frames");
  if (total_frames > 0 && (!d_rows || !d_back)) return mt3::fail(MT3_ERR_INVALID, who + "null scratch rows or back pointers");
  if (!d_beats) return mt3::fail(MT3_ERR_INVALID, who + "null beats");
  int64_t note_end = 0, frame_end = 0, beat_end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_beats_file& f = h_files[i];
    if (f.n_frames < 0 || f.n_frames >= MT3_BEATS_MAX_FRAMES)
      return mt3::fail(MT3_ERR_INVALID, who + "n_frames must be 0 .. 2^20 - 1");
    if (f.first < 0 || f.n_notes < 0 || f.first > n_notes || f.n_notes > n_notes - f.first)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's note range must lie inside [0, n_notes]");
    if (f.frame0 < 0 || f.frame0 > total_frames || f.n_frames > total_frames - f.frame0)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's frame range must lie inside [0, total_frames]");
    const int64_t room = MT3_BEATS_CAPACITY(f.n_frames);
    if (f.beat0 < 0 || f.beat0 > total_beats || room > total_beats - f.beat0)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's beat range (n_frames / 13 + 2) must lie inside [0, total_beats]");
    if (f.first < note_end) return mt3::fail(MT3_ERR_INVALID, who + "note ranges overlap or are out of order");
    if (f.frame0 < frame_end) return mt3::fail(MT3_ERR_INVALID, who + "frame ranges overlap or are out of order");
    if (f.beat0 < beat_end) return mt3::fail(MT3_ERR_INVALID, who + "beat ranges overlap or are out of order");
    note_end = f.first + f.n_notes, frame_end = f.frame0 + f.n_frames, beat_end = f.beat0 + room;
  }

  hipStream_t s = static_cast<hipStream_t>(stream);
  if (total_frames > 0) MT3_HIP_CHECK(hipMemsetAsync(d_rows, 0, static_cast<size_t>(total_frames) * sizeof(int32_t), s));
  for (int32_t p0 = 0; p0 < n_files; p0 += kPerLaunch) {
    const int n = n_files - p0 < kPerLaunch ? n_files - p0 : kPerLaunch;
    BeatsTable t{};
    for (int i = 0; i < n; ++i) {
      const mt3_beats_file& f = h_files[p0 + i];
      t.first[i] = f.first, t.frame0[i] = f.frame0, t.beat0[i] = f.beat0, t.n_notes[i] = f.n_notes, t.n_frames[i] = f.n_frames;
    }
    hipLaunchKernelGGL(track_kernel, dim3(static_cast<uint32_t>(n)), dim3(kThreads), 0, s, t, d_frames, d_prior, d_penalties,
                       d_rows, total_frames, d_back, d_period + p0, d_n_beats + p0, d_beats, d_score + p0);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}

extern "C" int mt3_op_snap_notes(const double* d_start, const double* d_end, int64_t n_notes, const int32_t* d_beat_frames,
                                 int64_t n_beat_frames, const mt3_snap_file* h_files, int32_t n_files, int32_t subdivisions,
                                 double* d_out_start, double* d_out_end, void* stream) {
  const std::string who = "mt3_op_snap_notes: ";
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (n_beat_frames < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_beat_frames must not be negative");
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (subdivisions < 1 || subdivisions > MT3_BEATS_MAX_SUBDIVISIONS)
    return mt3::fail(MT3_ERR_INVALID, who + "subdivisions must be 1 .. " + std::to_string(MT3_BEATS_MAX_SUBDIVISIONS));
  if (n_files == 0) return MT3_OK;
  if (!h_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table");
  if (n_notes > 0 && (!d_start || !d_end || !d_out_start || !d_out_end))
    return mt3::fail(MT3_ERR_INVALID, who + "null start, end or output column");
  if (n_beat_frames > 0 && !d_beat_frames) return mt3::fail(MT3_ERR_INVALID, who + "null beat frames");
  int64_t note_end = 0, beat_end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_snap_file& f = h_files[i];
    if (f.first < 0 || f.n_notes < 0 || f.first > n_notes || f.n_notes > n_notes - f.first)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's note range must lie inside [0, n_notes]");
    if (f.beat0 < 0 || f.n_beats < 0 || f.beat0 > n_beat_frames || f.n_beats > n_beat_frames - f.beat0)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's beat range must lie inside [0, n_beat_frames]");
    if (f.first < note_end) return mt3::fail(MT3_ERR_INVALID, who + "note ranges overlap or are out of order");
    if (f.beat0 < beat_end) return mt3::fail(MT3_ERR_INVALID, who + "beat ranges overlap or are out of order");
    note_end = f.first + f.n_notes, beat_end = f.beat0 + f.n_beats;
  }
  if (n_notes == 0) return MT3_OK;

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t p0 = 0; p0 < n_files; p0 += kPerLaunch) {
    const int n = n_files - p0 < kPerLaunch ? n_files - p0 : kPerLaunch;
    SnapTable t{};
    for (int i = 0; i < n; ++i) {
      const mt3_snap_file& f = h_files[p0 + i];
      t.first[i] = f.first, t.beat0[i] = f.beat0, t.n_notes[i] = f.n_notes, t.n_beats[i] = f.n_beats;
    }
    hipLaunchKernelGGL(snap_kernel, dim3(static_cast<uint32_t>(n)), dim3(kThreads), 0, s, t, d_start, d_end, d_beat_frames,
                       static_cast<double>(subdivisions), d_out_start, d_out_end);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}
