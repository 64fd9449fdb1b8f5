// Note preparation for gfx950: known notes as the reference prepares them before tokenizing -- the sustain pedal applied
// to every note's end (note_seq.apply_sustain_control_changes) or overlapping notes trimmed (mt3 trim_overlapping_notes)
// (mt3_op_prepare_notes).  The rule: include/mt3_hip.h, "note preparation"; its event-by-event statement on the host:
// mt3_amd/note_sequences.py, apply_sustain_control_changes / trim_overlapping_notes.
//
// One workgroup of 256 lanes per file, 64 files per launch (their table rides in the kernel arguments).  The file's notes
// lie sorted by (key, start, pos), so the notes of one key are a run and a note's successor is inside its run; the pedal
// events lie sorted by (instrument, time, ON before OFF), so the pedal's state at a time is one binary search:
//   0. (sustain) tiles of 256 pedal events walked from the END: an exclusive block_scan_max over the reversed lane order,
//      carried from tile to tile -> for every event the index of the next OFF at or after it, into scratch;
//   1. tiles of 256 notes walked from the END, one note per lane: flag = the pedal is down at the note's start (sustain) or
//      1 (trim); the same reversed scan over "position if flagged" -> the nearest flagged successor j, which decides only
//      when it has the note's key (runs are contiguous); then the case analysis -> the new end and a keep flag, into
//      scratch at the note's ORIGINAL position;
//   2. tiles over the original order: block_scan_add of the keep flags, carried, compacts the survivors' ends and
//      positions into the output columns.
// Every new end is a member value (a note start, a pedal time, t_last): nothing is computed, so nothing rounds.  Indices
// come from the scans and from binary searches over [0, n): unsorted columns give other notes, never an index outside the
// file; a `pos` outside the file is not written.  Scratch words written in one pass are read in the next by other lanes
// of the same workgroup, after a __syncthreads.  Plain vector loads and stores only, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "device.h"
#include "mt3_hip.h"

namespace {

constexpr int kTile = MT3_NOTE_PREP_TILE;            // notes per tile = lanes of the workgroup
constexpr int kWaves = kTile / 64;
constexpr int kPerLaunch = 64;                       // files whose table fits one launch's arguments

struct PrepTable {                                   // 64 * 40 bytes by value
  int64_t first[kPerLaunch], pedal_first[kPerLaunch];
  double t_last[kPerLaunch], total_time[kPerLaunch];
  int32_t n_notes[kPerLaunch], n_pedal[kPerLaunch];
};
static_assert(sizeof(PrepTable) <= 2560, "the table of one launch stays within 2.5 KiB of kernel arguments");

// the first pedal event after (instrument g, time t) in the order (instrument, time): in [0, np] whatever the columns hold
__device__ __forceinline__ int32_t pedal_after(const double* time, const int32_t* inst_state, int32_t np, int32_t g,
                                               double t) {
  int32_t lo = 0, hi = np;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    const int32_t gi = inst_state[mid] >> 1;
    if (gi > g || (gi == g && time[mid] > t)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// ped(g, t): the event before `after` is g's and an ON
__device__ __forceinline__ bool pedal_down(const int32_t* inst_state, int32_t after, int32_t g) {
  return after > 0 && inst_state[after - 1] == g * 2;
}

__global__ __launch_bounds__(kTile) void note_prep_kernel(
    PrepTable t, int mode, const double* __restrict__ d_start, const double* __restrict__ d_end,
    const int32_t* __restrict__ d_key, const int32_t* __restrict__ d_pos, int64_t n_job,
    const double* __restrict__ d_pedal_time, const int32_t* __restrict__ d_pedal_inst_state,
    double* __restrict__ d_out_end, int32_t* __restrict__ d_out_src, int32_t* __restrict__ d_counts,
    double* __restrict__ d_total_time, int32_t* d_scratch) {
  __shared__ int s_scan[kWaves];
  __shared__ double s_rel[kTile];
  __shared__ int s_took_last[kTile];
  const int tid = threadIdx.x;
  const int64_t first = t.first[blockIdx.x];
  const int32_t n = t.n_notes[blockIdx.x];
  const int32_t np = mode == MT3_NOTE_PREP_SUSTAIN ? t.n_pedal[blockIdx.x] : 0;
  const double t_last = t.t_last[blockIdx.x];
  const double* start = d_start + first;
  const double* end = d_end + first;
  const int32_t* key = d_key + first;
  const int32_t* pos = d_pos + first;
  const double* pedal_time = d_pedal_time + t.pedal_first[blockIdx.x];
  const int32_t* pedal_is = d_pedal_inst_state + t.pedal_first[blockIdx.x];
  double* new_end = reinterpret_cast<double*>(d_scratch) + first;      // [n] per ORIGINAL position
  int32_t* keep_of = d_scratch + 2 * n_job + first;                    // [n] per ORIGINAL position
  int32_t* next_off = d_scratch + 3 * n_job + t.pedal_first[blockIdx.x];   // [np] per pedal event

  // ---- 0: for every pedal event the next OFF at or after it (np: none), walking from the end
  int32_t carry = 0;                                   // np - (the nearest OFF so far), 0: none; uniform
  for (int32_t t0 = np > 0 ? (np - 1) / kTile * kTile : -1; t0 >= 0; t0 -= kTile) {
    const int64_t k = static_cast<int64_t>(t0) + (kTile - 1 - tid);      // lanes before this one hold later events
    const int mine = k < np && (pedal_is[k] & 1) ? static_cast<int>(np - k) : 0;
    int before, total;
    mt3k::block_scan_max<kWaves>(mine, s_scan, &before, &total);
    if (k < np) next_off[k] = np - max(max(before, carry), mine);      // in [k, np]
    carry = max(carry, total);
    __syncthreads();                                   // s_scan is free again; after the last tile: scratch is written
  }

  // ---- 1: the successor that decides, the new end and the keep flag of every note
  double my_rel = -INFINITY;                           // the largest release this lane's notes were held to
  int my_took_last = 0;
  carry = 0;                                           // n - (the nearest flagged note so far), 0: none; uniform
  for (int32_t t0 = n > 0 ? (n - 1) / kTile * kTile : -1; t0 >= 0; t0 -= kTile) {
    const int64_t i = static_cast<int64_t>(t0) + (kTile - 1 - tid);
    double s = 0, e = 0;
    int32_t k = 0, g = 0;
    int flag = 0;
    if (i < n) {
      s = start[i], e = end[i], k = key[i], g = k >> 7;
      flag = mode == MT3_NOTE_PREP_SUSTAIN ? pedal_down(pedal_is, pedal_after(pedal_time, pedal_is, np, g, s), g) : 1;
    }
    int before, total;
    mt3k::block_scan_max<kWaves>(flag ? static_cast<int>(n - i) : 0, s_scan, &before, &total);
    const int32_t nearest = max(before, carry);        // of the notes after i alone
    carry = max(carry, total);
    if (i < n) {
      const int32_t j = n - nearest;                   // nearest > 0: i < j < n
      const bool has_j = nearest > 0 && key[j] == k;
      const double sj = has_j ? start[j] : 0.0;
      double to = e;
      int keep = 1;
      if (mode == MT3_NOTE_PREP_SUSTAIN) {
        const int32_t after = pedal_after(pedal_time, pedal_is, np, g, e);
        const bool down = pedal_down(pedal_is, after, g);
        const int32_t off = after < np ? next_off[after] : np;          // <= np
        const bool has_rel = off < np && (pedal_is[off] >> 1) == g;
        const double rel = has_rel ? pedal_time[off] : 0.0;
        if (has_j && (down ? (!has_rel || sj < rel) : sj <= e)) {
          to = sj, keep = sj != s;
        } else if (down) {
          to = has_rel ? rel : t_last;
          if (has_rel) my_rel = fmax(my_rel, rel); else my_took_last = 1;
        }
      } else {
        if (has_j && e > sj) to = sj;
        keep = s < to;
      }
      const int32_t p = pos[i];
      if (p >= 0 && p < n) new_end[p] = to, keep_of[p] = keep;
    }
    __syncthreads();
  }

  // ---- the file's total_time: t_last when a note was held to the end, else the largest of the old one and the releases
  s_rel[tid] = my_rel, s_took_last[tid] = my_took_last;
  __syncthreads();
  if (tid == 0) {
    double total = t.total_time[blockIdx.x];
    int took_last = 0;
    for (int l = 0; l < kTile; ++l) total = fmax(total, s_rel[l]), took_last |= s_took_last[l];
    d_total_time[blockIdx.x] = took_last ? t_last : total;
  }

  // ---- 2: the survivors, compacted in the original order
  int32_t kept_so_far = 0;                             // uniform
  for (int64_t t0 = 0; t0 < n; t0 += kTile) {
    const int64_t p = t0 + tid;
    const int keep = p < n && keep_of[p] != 0;
    int before, total;
    mt3k::block_scan_add<kWaves>(keep, s_scan, &before, &total);
    if (keep) {
      const int64_t at = first + kept_so_far + before; // kept_so_far + before < the file's kept notes <= n
      d_out_end[at] = new_end[p];
      d_out_src[at] = static_cast<int32_t>(p);
    }
    kept_so_far += total;
    __syncthreads();
  }
  if (tid == 0) d_counts[blockIdx.x] = kept_so_far;
}

}  // namespace

extern "C" int mt3_op_prepare_notes(int32_t mode, const double* d_start, const double* d_end, const int32_t* d_key,
                                    const int32_t* d_pos, int64_t n_notes, const double* d_pedal_time,
                                    const int32_t* d_pedal_inst_state, int64_t n_pedal, const mt3_note_prep_file* h_files,
                                    int32_t n_files, double* d_out_end, int32_t* d_out_src, int32_t* d_counts,
                                    double* d_total_time, int32_t* d_scratch, int64_t scratch_words, void* stream) {
  const std::string who = "mt3_op_prepare_notes: ";
  if (mode != MT3_NOTE_PREP_SUSTAIN && mode != MT3_NOTE_PREP_TRIM)
    return mt3::fail(MT3_ERR_INVALID, who + "unknown mode: MT3_NOTE_PREP_SUSTAIN or MT3_NOTE_PREP_TRIM");
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (n_pedal < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_pedal must not be negative");
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (n_files == 0) return MT3_OK;
  if (!h_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table");
  if (n_notes > 0 && (!d_start || !d_end || !d_key || !d_pos))
    return mt3::fail(MT3_ERR_INVALID, who + "null note column (start, end, key or pos)");
  const bool sustain = mode == MT3_NOTE_PREP_SUSTAIN;
  if (sustain && n_pedal > 0 && (!d_pedal_time || !d_pedal_inst_state))
    return mt3::fail(MT3_ERR_INVALID, who + "null pedal column (time or inst_state)");
  if (n_notes > 0 && (!d_out_end || !d_out_src)) return mt3::fail(MT3_ERR_INVALID, who + "null output column (end or src)");
  if (!d_counts) return mt3::fail(MT3_ERR_INVALID, who + "null counts");
  if (!d_total_time) return mt3::fail(MT3_ERR_INVALID, who + "null total_time");
  const int64_t pedal_words = sustain ? n_pedal : 0;
  if ((n_notes > 0 || pedal_words > 0) && !d_scratch) return mt3::fail(MT3_ERR_INVALID, who + "null scratch");
  if (reinterpret_cast<uintptr_t>(d_scratch) % 8)
    return mt3::fail(MT3_ERR_INVALID, who + "scratch must be 8-byte aligned: it starts with float64 words");
  if (n_notes > INT64_MAX / 8 || n_pedal > INT64_MAX / 8 || scratch_words < MT3_NOTE_PREP_SCRATCH_WORDS(n_notes, pedal_words))
    return mt3::fail(MT3_ERR_INVALID, who + "scratch too small: 3 * n_notes + n_pedal int32 words are needed");
  int64_t end = 0, pedal_end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_note_prep_file& f = h_files[i];
    if (f.first < 0 || f.n_notes < 0 || f.first > n_notes || f.n_notes > n_notes - f.first)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's note range must lie inside [0, n_notes]");
    if (f.first < end) return mt3::fail(MT3_ERR_INVALID, who + "note ranges overlap or are out of order");
    end = f.first + f.n_notes;
    if (!std::isfinite(f.t_last) || !std::isfinite(f.total_time))
      return mt3::fail(MT3_ERR_INVALID, who + "t_last and total_time must be finite");
    if (!sustain) continue;
    if (f.pedal_first < 0 || f.n_pedal < 0 || f.pedal_first > n_pedal || f.n_pedal > n_pedal - f.pedal_first)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's pedal range must lie inside [0, n_pedal]");
    if (f.pedal_first < pedal_end) return mt3::fail(MT3_ERR_INVALID, who + "pedal ranges overlap or are out of order");
    pedal_end = f.pedal_first + f.n_pedal;
  }

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t p0 = 0; p0 < n_files; p0 += kPerLaunch) {
    const int n = n_files - p0 < kPerLaunch ? n_files - p0 : kPerLaunch;
    PrepTable t{};
    for (int i = 0; i < n; ++i) {
      const mt3_note_prep_file& f = h_files[p0 + i];
      t.first[i] = f.first, t.n_notes[i] = f.n_notes, t.t_last[i] = f.t_last, t.total_time[i] = f.total_time;
      t.pedal_first[i] = sustain ? f.pedal_first : 0, t.n_pedal[i] = sustain ? f.n_pedal : 0;
    }
    hipLaunchKernelGGL(note_prep_kernel, dim3(static_cast<uint32_t>(n)), dim3(kTile), 0, s, t, static_cast<int>(mode),
                       d_start, d_end, d_key, d_pos, n_notes, d_pedal_time, d_pedal_inst_state, d_out_end, d_out_src,
                       d_counts + p0, d_total_time + p0, d_scratch);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}
