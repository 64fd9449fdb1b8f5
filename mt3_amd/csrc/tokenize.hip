// The target tokenizer for gfx950: the notes of a job -> the id rows the model is trained on (mt3_op_tokenize_notes; the
// rule: include/mt3_hip.h, mt3t_*; the same rule serially on the host: mt3_notes_tokenize in symbolic.cpp).
//
// One workgroup of 256 lanes owns a FILE and walks its rows (one per segment) in order.  What a row needs from the rows
// before it is the held table at its tie section's start, so the table stays in LDS -- one bit per (program, pitch),
// 2 KiB -- and each row only advances it by the events between the previous start and its own:
//   1. the row's ranges: three binary searches over the file's steps (mt3t_tie_begin, mt3t_lower_bound), done by every
//      lane on the same addresses, so the result is uniform without a broadcast;
//   2. advance: the events [done, b) in tiles of 256, one per lane.  A pitched event is a write to its pair; the LAST
//      writer decides: atomicMax of (lane + 1) << 1 | set into an LDS table of one word per pair (64 KiB), and after a
//      barrier the lane that reads its own key back applies its effect to the held bits (atomicOr / atomicAnd: two winners
//      may share a word, never a bit) and puts the word back to 0.  Tiles are taken in order (mt3_op_tie_prompts' shape);
//   3. tie section: lane p < 128 owns program row p.  Whether the row opens with a program id is a compare with the last
//      program WRITTEN before it -- an exclusive max-scan of (p + 1) << 8 | mapped program over the non-empty rows whose
//      map entry is not -1; an exclusive add-scan of the rows' id counts gives each its place.  The scan's total is the
//      program the segment's first event is compared with: the seam between tie section and events;
//   4. events: tiles of 256, one per lane.  Shift ids and the velocity id depend on the event before only, which the lane
//      reads from memory; the program id needs the last pitched event with a mapped program, drums lying between: the
//      same max-scan, carried from tile to tile and started from the tie section's total.  An add-scan of the per-event
//      id counts (shift ids + 0 / 1 program + 0 / 1 velocity + 1) places them; every lane writes its own ids, note_of and
//      is_onset, each position of the row exactly once;
//   5. EOS or the cut, the padding, length and truncated.
// Every loop is bounded by its arguments: rows of the file, events / 256 tiles, at most `stride` shift ids per event, 32
// rounds per binary search.  No lane waits for another outside __syncthreads, whose conditions are uniform.  Plain vector
// loads and stores and LDS atomics only; no floating point.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "common.h"
#include "device.h"
#include "mt3_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPairs = MT3_TOKENIZE_PROGRAMS * MT3_TOKENIZE_PITCHES;
constexpr int kRowWords = MT3_TOKENIZE_PITCHES / 32;
constexpr int kWords = kPairs / 32;
static_assert(MT3_TOKENIZE_PROGRAMS <= kThreads, "a lane per program row");

__global__ __launch_bounds__(kThreads) void tokenize_kernel(
    mt3_tokenize_rule r, const int32_t* __restrict__ d_step, const int32_t* __restrict__ d_pitch,
    const int32_t* __restrict__ d_program, const int32_t* __restrict__ d_velbin, const int32_t* __restrict__ d_is_drum,
    const int32_t* __restrict__ d_note, int64_t n_events, const mt3_tokenize_file* __restrict__ files,
    const mt3_tokenize_row* __restrict__ rows, int32_t n_rows_job, int32_t stride, int32_t* __restrict__ d_ids,
    int32_t* __restrict__ d_lengths, int32_t* __restrict__ d_truncated, int32_t* __restrict__ d_note_of,
    uint8_t* __restrict__ d_is_onset) {
  __shared__ int s_last[kPairs];             // per (program, pitch): the key of its last writer in the tile, 0 = none
  __shared__ uint32_t s_held[kWords];
  __shared__ int s_max[kWaves], s_add[kWaves];

  const int tid = threadIdx.x;
  const bool ties = r.spec == MT3_SPEC_TIES;
  const mt3_tokenize_file file = files[blockIdx.x];
  // ---- the file's ranges, checked: everything below indexes inside [ev0, ev0 + n_ev) and [row_lo, row_hi)
  int64_t ev0 = file.event0;
  int32_t n_ev = file.n_events;
  if (ev0 < 0 || n_ev < 0 || ev0 > n_events || n_ev > n_events - ev0) ev0 = 0, n_ev = 0;
  if (file.row0 < 0 || file.n_rows < 0 || file.row0 > n_rows_job || file.n_rows > n_rows_job - file.row0) return;
  const int32_t row_lo = file.row0, row_hi = file.row0 + file.n_rows;
  const int32_t* step = d_step + ev0;
  const int32_t* pitch = d_pitch + ev0;
  const int32_t* program = d_program + ev0;
  const int32_t* velbin = d_velbin + ev0;
  const int32_t* is_drum = d_is_drum + ev0;
  const int32_t* note = d_note + ev0;

  if (ties) {
    for (int i = tid; i < kPairs; i += kThreads) s_last[i] = 0;
    for (int i = tid; i < kWords; i += kThreads) s_held[i] = 0u;
  }
  __syncthreads();

  int32_t done = 0;                          // the events replayed into s_held so far; uniform
  for (int32_t row = row_lo; row < row_hi; ++row) {
    const mt3_tokenize_row seg = rows[row];
    if (seg.file != static_cast<int32_t>(blockIdx.x)) continue;          // uniform: another file's row
    int32_t* ids = d_ids + static_cast<size_t>(row) * stride;
    int32_t* note_of = d_note_of + static_cast<size_t>(row) * stride;
    uint8_t* is_onset = d_is_onset + static_cast<size_t>(row) * stride;
    const int32_t e_lo = mt3t_lower_bound(step, n_ev, seg.step_lo);
    const int32_t e_hi = seg.step_hi > seg.step_lo ? max(e_lo, mt3t_lower_bound(step, n_ev, seg.step_hi)) : e_lo;
    int64_t base = 0;                        // ids of the row so far; uniform
    int last_program = -1;                   // the last program written in the row so far; uniform

    if (ties) {
      // ---- 2: advance the held table to the tie section's start
      const int32_t b = mt3t_tie_begin(step, n_ev, seg.step_lo);
      for (int32_t t0 = done; t0 < b; t0 += kThreads) {
        const int32_t e = t0 + tid;
        int key = 0, pair = 0;
        if (e < b && !is_drum[e]) {
          pair = mt3t_index(program[e]) * MT3_TOKENIZE_PITCHES + mt3t_index(pitch[e]);
          key = ((tid + 1) << 1) | (mt3t_velbin(&r, velbin[e]) ? 1 : 0);
          atomicMax(&s_last[pair], key);
        }
        __syncthreads();
        if (key && s_last[pair] == key) {
          if (key & 1)
            atomicOr(&s_held[pair >> 5], 1u << (pair & 31));
          else
            atomicAnd(&s_held[pair >> 5], ~(1u << (pair & 31)));
          s_last[pair] = 0;
        }
        __syncthreads();
      }
      done = max(done, b);
      // ---- 3: the tie section
      int mine = 0, mapped = -1;
      if (tid < MT3_TOKENIZE_PROGRAMS) {
#pragma unroll
        for (int w = 0; w < kRowWords; ++w) mine += __popc(s_held[tid * kRowWords + w]);
        mapped = r.program_map[tid];
      }
      int seen, seen_all, off, total;
      mt3k::block_scan_max<kWaves>(mine && mapped >= 0 ? ((tid + 1) << 8) | mapped : 0, s_max, &seen, &seen_all);
      const int opens = mine && mapped >= 0 && (seen ? (seen & 0xff) : -1) != mapped;
      mt3k::block_scan_add<kWaves>(mine + opens, s_add, &off, &total);
      if (mine) {
        int64_t at = off;
        if (opens) mt3t_put(stride, &at, r.program_first + mapped, -1, 0, ids, note_of, is_onset);
        for (int w = 0; w < kRowWords; ++w) {
          uint32_t bits = s_held[tid * kRowWords + w];
          while (bits && at < stride) {      // at most 32 rounds
            const int q = __ffs(bits) - 1;
            bits &= bits - 1;
            mt3t_put(stride, &at, r.pitch_first + w * 32 + q, -1, 0, ids, note_of, is_onset);
          }
        }
      }
      if (tid == 0) {
        int64_t at = total;
        mt3t_put(stride, &at, r.tie_id, -1, 0, ids, note_of, is_onset);
      }
      base = static_cast<int64_t>(total) + 1;
      if (seen_all) last_program = seen_all & 0xff;
      __syncthreads();                       // s_max / s_add are free again; s_held is read before the next advance
    }

    // ---- 4: the segment's events
    for (int32_t t0 = e_lo; t0 < e_hi; t0 += kThreads) {
      const int32_t e = t0 + tid;
      const bool active = e < e_hi;
      int64_t d = 0;
      int n_shift = 0, mapped = -1, v = 0, drum = 0, has_velocity = 0;
      if (active) {
        d = static_cast<int64_t>(step[e]) - seg.step_lo;
        const int64_t prev = e > e_lo ? static_cast<int64_t>(step[e - 1]) - seg.step_lo : 0;
        const int64_t want = mt3t_shift_count(&r, d, prev);
        n_shift = static_cast<int>(want < stride ? want : stride);        // more than `stride` of them end past the cut anyway
        v = mt3t_velbin(&r, velbin[e]);
        drum = ties && is_drum[e];
        if (ties && !drum) mapped = r.program_map[mt3t_index(program[e])];
        has_velocity = e == e_lo || v != mt3t_velbin(&r, velbin[e - 1]);
      }
      int seen, seen_all, off, total;
      mt3k::block_scan_max<kWaves>(mapped >= 0 ? ((tid + 1) << 8) | mapped : 0, s_max, &seen, &seen_all);
      const int has_program = mapped >= 0 && (seen ? (seen & 0xff) : last_program) != mapped;
      mt3k::block_scan_add<kWaves>(active ? n_shift + has_program + has_velocity + 1 : 0, s_add, &off, &total);
      if (active) {
        int64_t at = base + off;
        for (int k = 0; k < n_shift && at < stride; ++k)
          mt3t_put(stride, &at, r.shift_first + mt3t_shift_value(&r, d, k), -1, 0, ids, note_of, is_onset);
        at = base + off + n_shift;
        if (has_program) mt3t_put(stride, &at, r.program_first + mapped, -1, 0, ids, note_of, is_onset);
        if (has_velocity) mt3t_put(stride, &at, r.velocity_first + v, -1, 0, ids, note_of, is_onset);
        mt3t_put(stride, &at, (drum ? r.drum_first : r.pitch_first) + mt3t_index(pitch[e]), note[e], v != 0, ids, note_of,
                 is_onset);
      }
      base += total;
      if (seen_all) last_program = seen_all & 0xff;
      __syncthreads();                       // s_max / s_add are free again
    }

    // ---- 5: EOS or the cut, and the padding
    if (tid == 0) {
      d_lengths[row] = base < stride ? static_cast<int32_t>(base) + 1 : stride;
      d_truncated[row] = base < stride ? 0 : 1;
    }
    for (int64_t i = base + tid; i < stride; i += kThreads) {
      ids[i] = i == base ? 1 : 0;
      note_of[i] = -1;
      is_onset[i] = 0;
    }
  }
}

}  // namespace

extern "C" int mt3_op_tokenize_notes(const mt3_tokenize_rule* r, const int32_t* d_step, const int32_t* d_pitch,
                                     const int32_t* d_program, const int32_t* d_velbin, const int32_t* d_is_drum,
                                     const int32_t* d_note, int64_t n_events, const mt3_tokenize_file* d_files,
                                     int32_t n_files, const mt3_tokenize_row* d_rows, int32_t rows, int32_t stride,
                                     int32_t* d_ids, int32_t* d_lengths, int32_t* d_truncated, int32_t* d_note_of,
                                     uint8_t* d_is_onset, void* stream) {
  const std::string who = "mt3_op_tokenize_notes: ";
  if (const char* bad = mt3t_bad_rule(r, stride)) return mt3::fail(MT3_ERR_INVALID, who + bad);
  if (n_events < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_events must not be negative");
  if (n_files < 1) return mt3::fail(MT3_ERR_INVALID, who + "n_files must be at least 1");
  if (rows < 1) return mt3::fail(MT3_ERR_INVALID, who + "rows must be at least 1");
  if (n_events > 0 && (!d_step || !d_pitch || !d_program || !d_velbin || !d_is_drum || !d_note))
    return mt3::fail(MT3_ERR_INVALID, who + "null event array");
  if (!d_files || !d_rows) return mt3::fail(MT3_ERR_INVALID, who + "null table");
  if (!d_ids || !d_lengths || !d_truncated || !d_note_of || !d_is_onset) return mt3::fail(MT3_ERR_INVALID, who + "null output");
  hipLaunchKernelGGL(tokenize_kernel, dim3(static_cast<uint32_t>(n_files)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), *r, d_step, d_pitch, d_program, d_velbin, d_is_drum, d_note, n_events,
                     d_files, d_rows, rows, stride, d_ids, d_lengths, d_truncated, d_note_of, d_is_onset);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}
