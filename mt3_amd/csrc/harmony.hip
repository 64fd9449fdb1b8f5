// Harmony and meter for gfx950: the key, the chord of every beat, the bar length and the downbeat phase of every file of a
// job from its notes and its beat frames (mt3_op_analyze_harmony).  The rule: include/mt3_hip.h, "harmony"; its numpy
// statement: mt3_amd/harmony.py, analyze_reference.
//
// One workgroup of 256 lanes (4 waves) per file, all files in ONE launch (the file table is read from the device), no
// workgroup waits for another.  Everything is integer arithmetic, so no order of the sums matters.
//   key    every lane adds its notes' lengths to D[12] in LDS (64-bit integer atomics); 24 lanes take a key each.
//   tiles  the beats go through LDS kTile = 32 intervals at a time -- the roll of a ten-minute file (1,200 x 128 words)
//          does not fit, one tile (32 x 129 words, the rows padded by one word against bank conflicts) does.  Per tile:
//     1. the tile's kTile + 1 interval edges into LDS; the roll, the onset counts and the struck flags cleared
//     2. roll: a lane per note (the file's notes in passes of 256).  A note outside the tile's frames is dropped after two
//        compares; one inside finds its first interval by binary search in the edges and adds its overlap to every
//        interval it reaches (LDS integer atomics).  No carry leaves a tile, so there is no scan across tiles.
//     3. H[i][c] (a lane per interval and class, 11 reads) and the lowest loud pitch (a lane per interval, ascending)
//     4. Q[i][k] (a lane per interval and state; the quotient floored by hand for a negative E), and, over the notes once
//        more, the onsets within the window of each beat of the tile and whether one of them is the lowest loud pitch
//     5. wave 0 walks the tile's beats: lane k < 25 holds V[k] in a register across tiles; one step is a butterfly of five
//        xor moves (the higher value, then the lower index), a compare and a byte of `back` to the workspace.  Wave 1
//        stores the tile's onset counts and struck flags (16 bits per beat) beside it.
//   path   lane 0 follows `back` from the last beat: dependent one-byte loads, like the read-back of beats.hip.
//   meter  every lane folds its beats' accents into the nine sums (m = 2, 3, 4; every phase) in registers; xor moves
//          across the wave, then one LDS atomic per wave and sum; lane 0 takes the best (m, phase).
// Plain vector loads and stores and integer atomics only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "common.h"
#include "mt3_hip.h"

namespace {

constexpr int kThreads = MT3_HARMONY_NOTE_TILE;       // 256
constexpr int kTile = MT3_HARMONY_BEAT_TILE;          // intervals per tile
constexpr int kStates = MT3_HARMONY_STATES;           // 25
constexpr int kKeys = MT3_HARMONY_KEYS;               // 24
constexpr int kRow = 129;                             // words per interval of the roll: 128 pitches and one of padding
constexpr int kWindow = MT3_HARMONY_ONSET_WINDOW;
static_assert(kThreads % 64 == 0 && kThreads >= 128, "wave 0 walks the path while wave 1 stores the accents");
static_assert(kTile < 64 && kTile + 1 <= kThreads, "a lane per edge, and a lane of one wave per interval");
static_assert(kStates <= 32, "a lane of wave 0 per state; the lanes past the states hold the lowest value");
static_assert(MT3_HARMONY_WORKSPACE_BYTES_PER_BEAT == 2 + kStates, "16 bits of accents and 25 back pointers per beat");

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the higher value, then the lower index, over the 64 lanes
__device__ __forceinline__ void wave_argmax(int32_t& v, int32_t& at) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int32_t ov = __shfl_xor(v, o), oat = __shfl_xor(at, o);
    if (ov > v || (ov == v && oat < at)) v = ov, at = oat;
  }
}

__global__ __launch_bounds__(kThreads) void harmony_kernel(
    const mt3_harmony_file* __restrict__ d_files, const int32_t* __restrict__ d_start, const int32_t* __restrict__ d_end,
    const int32_t* __restrict__ d_key, const int32_t* __restrict__ d_beats, const int32_t* __restrict__ d_profiles,
    int32_t change_penalty, int32_t onset_weight, int32_t change_weight, int32_t bass_weight, uint16_t* d_accents,
    int8_t* d_back, int64_t* __restrict__ d_key_scores, int32_t* __restrict__ d_info, int8_t* d_chords) {
  __shared__ int32_t s_r[kTile * kRow];
  __shared__ int32_t s_h[kTile * 12];
  __shared__ int32_t s_q[kTile * kStates];
  __shared__ int32_t s_edge[kTile + 1];
  __shared__ int32_t s_low[kTile], s_on[kTile], s_struck[kTile];
  __shared__ unsigned long long s_d[12];
  __shared__ long long s_score[kKeys];
  __shared__ unsigned long long s_m[9];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int file = blockIdx.x;
  const mt3_harmony_file f = d_files[file];
  const int32_t n_notes = f.n_notes, B = f.n_beats;
  const int32_t* start = d_start + f.first;
  const int32_t* end = d_end + f.first;
  const int32_t* key = d_key + f.first;
  const int32_t* beats = d_beats + f.beat0;
  uint16_t* accents = d_accents + f.beat0;                     // [B]
  int8_t* back = d_back + f.beat0 * kStates;                   // [B][25]
  int8_t* chords = d_chords + f.beat0;                         // [B]
  int32_t* info = d_info + static_cast<int64_t>(file) * 4;

  // ---- the key
  if (tid < 12) s_d[tid] = 0;
  if (tid < 9) s_m[tid] = 0;
  __syncthreads();
  for (int32_t n = tid; n < n_notes; n += kThreads) {
    const int32_t s = start[n], e = end[n], k = key[n];
    if (s < 0 || e <= s || k < 0 || k >= 128) continue;            // a drum's key is >= 256
    atomicAdd(&s_d[k % 12], static_cast<unsigned long long>(e - s));
  }
  __syncthreads();
  if (tid < kKeys) {
    long long score = 0;
#pragma unroll
    for (int c = 0; c < 12; ++c) score += static_cast<long long>(d_profiles[tid * 12 + c]) * static_cast<long long>(s_d[c]);
    s_score[tid] = score;
    d_key_scores[static_cast<int64_t>(file) * kKeys + tid] = score;
  }
  __syncthreads();
  if (tid == 0) {
    bool any = false;
    for (int c = 0; c < 12; ++c) any |= s_d[c] != 0;
    int32_t at = 0;
    for (int k = 1; k < kKeys; ++k)
      if (s_score[k] > s_score[at]) at = k;                    // strictly greater: the lowest of the maximal ones
    info[0] = any ? at : -1;
  }
  if (B < 2) {                                                 // uniform: no chords and no meter
    if (tid == 0) info[1] = 0, info[2] = 0, info[3] = -1;
    return;
  }

  // ---- the tiles: roll, emissions, accents and the path's forward pass
  const int32_t last_edge = 2 * beats[B - 1] - beats[B - 2];
  int32_t V = INT32_MIN;                                       // wave 0, lane k < 25: V[k] of the beat before
  for (int32_t t0 = 0; t0 < B; t0 += kTile) {
    const int32_t nt = min(kTile, B - t0);
    if (tid <= nt) s_edge[tid] = t0 + tid < B ? beats[t0 + tid] : last_edge;
    for (int i = tid; i < kTile * kRow; i += kThreads) s_r[i] = 0;
    if (tid < kTile) s_on[tid] = 0, s_struck[tid] = 0;
    __syncthreads();

    // 2: the roll of the tile
    const int32_t lo = s_edge[0], hi = s_edge[nt];
    for (int32_t n = tid; n < n_notes; n += kThreads) {
      const int32_t s = start[n], e = end[n];
      if (s < 0 || e <= s || e <= lo || s >= hi) continue;
      const int32_t k = key[n];
      if (k < 0 || k >= 128) continue;                         // drums, and nothing outside a row of the roll
      int32_t a = 0, b = nt - 1;                               // the first interval that ends after s; s < hi: it exists
      while (a < b) {
        const int32_t m = (a + b) >> 1;
        if (s_edge[m + 1] > s) b = m; else a = m + 1;
      }
      for (int32_t j = a; j < nt && s_edge[j] < e; ++j)
        atomicAdd(&s_r[j * kRow + k], min(e, s_edge[j + 1]) - max(s, s_edge[j]));
    }
    __syncthreads();

    // 3: classes and the lowest loud pitch
    for (int x = tid; x < nt * 12; x += kThreads) {
      const int j = x / 12, c = x % 12;
      int32_t sum = 0;
      for (int p = c; p < 128; p += 12) sum += s_r[j * kRow + p];
      s_h[x] = sum;
    }
    if (tid < nt) {
      const long long len = s_edge[tid + 1] - s_edge[tid];
      int32_t low = -1;
      for (int p = 0; p < 128; ++p)
        if (4ll * s_r[tid * kRow + p] >= len) {
          low = p;
          break;
        }
      s_low[tid] = low;
    }
    __syncthreads();

    // 4: emissions, and the onsets at the tile's beats
    for (int x = tid; x < nt * kStates; x += kThreads) {
      const int j = x / kStates, k = x % kStates;
      int32_t q = 0;
      if (k > 0) {
        const int r = (k - 1) >> 1, minor = (k - 1) & 1;
        const int32_t* h = s_h + j * 12;
        long long tot = 0;
#pragma unroll
        for (int c = 0; c < 12; ++c) tot += h[c];
        const int third = r + 4 - minor, fifth = r + 7;
        const long long tones =
            static_cast<long long>(h[r]) + h[third >= 12 ? third - 12 : third] + h[fifth >= 12 ? fifth - 12 : fifth];
        long long E = 3 * tones - tot;                         // +2 on the chord's tones, -1 on the rest
        const int32_t low = s_low[j];
        if (low >= 0 && low % 12 == r) E += h[r];
        const long long num = E * 256, den = tot > 0 ? tot : 1;
        long long quot = num / den;
        if (num < 0 && quot * den != num) --quot;              // floor, not truncation
        q = static_cast<int32_t>(quot);
      }
      s_q[x] = q;
    }
    const int32_t first_beat = s_edge[0] - kWindow, last_beat = s_edge[nt - 1] + kWindow;
    for (int32_t n = tid; n < n_notes; n += kThreads) {
      const int32_t s = start[n];
      if (s < first_beat || s > last_beat || s < 0 || end[n] <= s) continue;
      const int32_t k = key[n];
      int32_t a = 0, b = nt;                                   // the first beat of the tile at or after s - window
      while (a < b) {
        const int32_t m = (a + b) >> 1;
        if (s_edge[m] >= s - kWindow) b = m; else a = m + 1;
      }
      for (int32_t j = a; j < nt && s_edge[j] <= s + kWindow; ++j) {
        atomicAdd(&s_on[j], 1);
        if (k == s_low[j]) atomicOr(&s_struck[j], 1);          // a drum's key is >= 256, a low of -1 is no key
      }
    }
    __syncthreads();

    // 5: the path through the tile (wave 0), the tile's accents (wave 1)
    if (wave == 0) {
      for (int32_t j = 0; j < nt; ++j) {
        const int32_t i = t0 + j;
        const int32_t q = lane < kStates ? s_q[j * kStates + lane] : 0;
        if (i == 0) {
          if (lane < kStates) V = q;
          continue;
        }
        int32_t best = V, at = lane;
        wave_argmax(best, at);
        const int32_t move = best - change_penalty;
        if (lane < kStates) {
          const bool stay = V >= move;                         // staying wins on equal values
          back[static_cast<int64_t>(i) * kStates + lane] = static_cast<int8_t>(stay ? lane : at);
          V = q + (stay ? V : move);
        }
      }
    } else if (wave == 1 && lane < nt) {
      accents[t0 + lane] = static_cast<uint16_t>(min(s_on[lane], 255) | (s_struck[lane] << 8));
    }
    __syncthreads();                                           // the tile's LDS is free; its `back` and accents are stored
  }

  // ---- the path's end and the chords
  if (wave == 0) {
    int32_t best = V, at = lane;
    wave_argmax(best, at);
    if (lane == 0) {
      int32_t k = at;
      for (int32_t i = B - 1; i >= 0; --i) {
        chords[i] = static_cast<int8_t>(k);
        if (i > 0) {
          k = back[static_cast<int64_t>(i) * kStates + k];
          if (k < 0 || k >= kStates) k = 0;                    // (nothing else is ever stored)
        }
      }
      info[1] = best;
    }
  }
  __syncthreads();                                             // the chords are stored

  // ---- the meter
  long long sums[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};             // m = 2: 0 .. 1, m = 3: 2 .. 4, m = 4: 5 .. 8
  for (int32_t i = tid; i < B; i += kThreads) {
    const int32_t x = accents[i];
    const int32_t change = i > 0 && chords[i] != chords[i - 1] ? 1 : 0;
    const long long a = onset_weight * (x & 255) + change_weight * change + bass_weight * (x >> 8);
    const int32_t f2 = i & 1, f3 = i % 3, f4 = i & 3;
#pragma unroll
    for (int p = 0; p < 2; ++p) sums[p] += f2 == p ? a : 0;
#pragma unroll
    for (int p = 0; p < 3; ++p) sums[2 + p] += f3 == p ? a : 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) sums[5 + p] += f4 == p ? a : 0;
  }
#pragma unroll
  for (int x = 0; x < 9; ++x) {
    const long long v = wave_sum(sums[x]);
    if (lane == 0 && v) atomicAdd(&s_m[x], static_cast<unsigned long long>(v));
  }
  __syncthreads();
  if (tid == 0) {
    const long long total = static_cast<long long>(s_m[0] + s_m[1]);
    long long best = 0;
    int32_t bar = 0, phase = -1;
    int at = 0;
    for (int m = 2; m <= 4; ++m) {
      for (int p = 0; p < m; ++p, ++at) {
        if (B < 2 * m) continue;
        const long long num = static_cast<long long>(s_m[at]);
        const long long cnt = (B - p + m - 1) / m;
        const long long score = (num << 16) / cnt - ((total - num) << 16) / (B - cnt);
        if (score > best) best = score, bar = m, phase = p;    // strictly greater: the lowest m, then the lowest phase
      }
    }
    info[2] = bar, info[3] = phase;
  }
}

}  // namespace

extern "C" int mt3_op_analyze_harmony(const int32_t* d_start, const int32_t* d_end, const int32_t* d_key,
                                      const int32_t* h_key, int64_t n_notes, const int32_t* d_beats,
                                      const int32_t* h_beats, int64_t n_beats,
                                      const mt3_harmony_file* h_files, const mt3_harmony_file* d_files, int32_t n_files,
                                      const int32_t* d_profiles, int32_t n_profiles, int32_t change_penalty,
                                      int32_t onset_weight, int32_t change_weight, int32_t bass_weight, void* d_workspace,
                                      int64_t workspace_bytes, int64_t* d_key_scores, int32_t* d_info, int8_t* d_chords,
                                      void* stream) {
  const std::string who = "mt3_op_analyze_harmony: ";
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (n_beats < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_beats must not be negative");
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (n_profiles != kKeys * 12)
    return mt3::fail(MT3_ERR_INVALID, who + "the profile table holds " + std::to_string(kKeys) + " rows of 12");
  if (change_penalty < 0 || change_penalty > MT3_HARMONY_MAX_CHANGE_PENALTY)
    return mt3::fail(MT3_ERR_INVALID, who + "change_penalty must be 0 .. 2^20");
  if (onset_weight < 0 || onset_weight > MT3_HARMONY_MAX_WEIGHT || change_weight < 0 ||
      change_weight > MT3_HARMONY_MAX_WEIGHT || bass_weight < 0 || bass_weight > MT3_HARMONY_MAX_WEIGHT)
    return mt3::fail(MT3_ERR_INVALID, who + "onset_weight, change_weight and bass_weight must be 0 .. " +
                                          std::to_string(MT3_HARMONY_MAX_WEIGHT));
  if (n_files == 0) return MT3_OK;
  if (!h_files || !d_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table");
  if (!d_profiles) return mt3::fail(MT3_ERR_INVALID, who + "null profile table");
  if (!d_key_scores || !d_info) return mt3::fail(MT3_ERR_INVALID, who + "null key_scores or info");
  if (n_notes > 0 && (!d_start || !d_end || !d_key || !h_key)) return mt3::fail(MT3_ERR_INVALID, who + "null note column");
  if (n_beats > 0 && (!d_beats || !h_beats)) return mt3::fail(MT3_ERR_INVALID, who + "null beat frames");
  if (n_beats > 0 && !d_chords) return mt3::fail(MT3_ERR_INVALID, who + "null chords");
  if (n_beats > 0 && !d_workspace) return mt3::fail(MT3_ERR_INVALID, who + "null workspace");
  if (workspace_bytes < MT3_HARMONY_WORKSPACE_BYTES_PER_BEAT * n_beats)
    return mt3::fail(MT3_ERR_INVALID, who + "the workspace holds " + std::to_string(MT3_HARMONY_WORKSPACE_BYTES_PER_BEAT) +
                                          " bytes per beat");
  if (reinterpret_cast<uintptr_t>(d_workspace) % 2)
    return mt3::fail(MT3_ERR_INVALID, who + "the workspace must be 2-byte aligned");
  int64_t note_end = 0, beat_end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_harmony_file& f = h_files[i];
    if (f.first < 0 || f.n_notes < 0 || f.first > n_notes || f.n_notes > n_notes - f.first)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's note range must lie inside [0, n_notes]");
    if (f.beat0 < 0 || f.n_beats < 0 || f.beat0 > n_beats || f.n_beats > n_beats - f.beat0)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's beat range must lie inside [0, n_beats]");
    if (f.first < note_end) return mt3::fail(MT3_ERR_INVALID, who + "note ranges overlap or are out of order");
    if (f.beat0 < beat_end) return mt3::fail(MT3_ERR_INVALID, who + "beat ranges overlap or are out of order");
    note_end = f.first + f.n_notes, beat_end = f.beat0 + f.n_beats;
    for (int64_t n = f.first; n < note_end; ++n)
      if (h_key[n] < 0 || (h_key[n] & ~0x100) > 127)
        return mt3::fail(MT3_ERR_INVALID, who + "a key is pitch + 256 * is_drum with a pitch of 0 .. 127");
    int64_t longest = 0;
    for (int64_t b = f.beat0; b < beat_end; ++b) {
      if (h_beats[b] < 0 || h_beats[b] >= MT3_BEATS_MAX_FRAMES || (b > f.beat0 && h_beats[b] <= h_beats[b - 1]))
        return mt3::fail(MT3_ERR_INVALID, who + "a file's beat frames must ascend strictly inside 0 .. 2^20 - 1");
      if (b > f.beat0 && h_beats[b] - h_beats[b - 1] > longest) longest = h_beats[b] - h_beats[b - 1];
    }
    if (f.n_notes * longest >= (int64_t{1} << 31))
      return mt3::fail(MT3_ERR_INVALID, who + "a file's notes times its longest beat interval must stay below 2^31");
  }

  uint8_t* workspace = static_cast<uint8_t*>(d_workspace);
  hipLaunchKernelGGL(harmony_kernel, dim3(static_cast<uint32_t>(n_files)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), d_files, d_start, d_end, d_key, d_beats, d_profiles, change_penalty, onset_weight, change_weight,
                     bass_weight, reinterpret_cast<uint16_t*>(workspace), reinterpret_cast<int8_t*>(workspace + 2 * n_beats),
                     d_key_scores, d_info, d_chords);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}
