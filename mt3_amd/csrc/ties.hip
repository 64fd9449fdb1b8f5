// Tied decoding for gfx950: emitted id rows -> the tie-section prompts of the file's next segments (mt3_op_tie_prompts;
// the rule: include/mt3_hip.h, mt3n_replay + mt3n_tie_section).
//
// The serial replay is a chain of up to 1024 dependent read-modify-writes of a 2 KiB table.  Here one workgroup of 256
// lanes owns a row and goes through it in tiles of 1024 ids, four consecutive ids per lane:
//   1. the tile's first id <= 1 and its first tie_id: a min over the lane's four ids, over the wave (shuffles), over the
//      four waves (LDS);
//   2. the last program id and the last velocity id at or before every position: an inclusive max-scan of the keys
//      (position + 1) << 8 | program value and (position + 1) << 1 | velocity-is-zero, 0 for every other id -- the larger
//      key is the later token and carries that token's value; a position whose key is still 0 takes the value carried in
//      from the tiles before (initially program 0, velocity non-zero: the note decoder's initial values);
//   3. every pitch id before the row's end is a write to its (program, pitch): a set inside the tie section or at non-zero
//      velocity, a clear otherwise (mt3n_pitch_effect).  The LAST writer decides: atomicMax of (position + 1) << 1 | set
//      into an LDS table of one word per pair (64 KiB at 128 x 128); after a barrier the lane that reads its own key back
//      is the pair's last writer in this tile -- it applies its effect to the held bits (LDS atomicOr / atomicAnd: two
//      winners may share a word, never a bit) and puts the pair's word back to 0 for the next tile.
// Tiles are taken in order and a tile's winners are applied before the next tile starts, so the held bits after the last
// tile are the serial replay's.  Steps 1 and 2 share their barrier; positions are tile-local, so no key overflows whatever
// the row's length.
// The section: lane r < program_count counts the bits of program row r; an exclusive add-scan of (count << 8 | row is
// non-empty) gives each row the index of its first pair and the number of non-empty rows before it, and the lane writes its
// row's pairs (at most 128) where they belong.  The lane that owns the last kept pair writes tie_id; the rest of the
// 2 * cap + 1 ids is zeroed by all lanes.
// Plain vector loads and stores and LDS atomics only; a row is read once (4 KiB at 1024 ids), the kernel is bound by its
// barriers, not by memory.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <string>

#include "common.h"
#include "device.h"
#include "mt3_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerLane = 4;
constexpr int kTile = kThreads * kPerLane;
constexpr int kMaxPairs = MT3_NOTE_MAX_PROGRAMS * MT3_NOTE_MAX_PITCHES;
constexpr int kMaxWords = MT3_NOTE_MAX_PROGRAMS * MT3_NOTE_ROW_WORDS;

__device__ __forceinline__ int wave_min(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o));
  return x;
}

__global__ __launch_bounds__(kThreads) void tie_prompts_kernel(mt3_note_grammar n, const int32_t* __restrict__ ids,
                                                               int32_t stride, int32_t cap, int32_t flags,
                                                               int32_t* __restrict__ prompts, int32_t* __restrict__ count,
                                                               uint32_t* __restrict__ held_out) {
  __shared__ int s_last[kMaxPairs];          // per (program, pitch): the key of its last writer in the tile, 0 = none
  __shared__ uint32_t s_held[kMaxWords];
  __shared__ int s_end[kWaves], s_tie[kWaves], s_prog[kWaves], s_vel[kWaves], s_sum[kWaves];
  __shared__ long long s_tie_at;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = n.g.pitch_count, R = n.g.program_count, RW = mt3n_row_words(&n), W = R * RW;
  const int32_t* row = ids + static_cast<size_t>(blockIdx.x) * stride;
  const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(ids) & 15) == 0;

  for (int i = tid; i < R * P; i += kThreads) s_last[i] = 0;
  for (int i = tid; i < W; i += kThreads) s_held[i] = 0u;
  __syncthreads();

  int carry_prog = 0, carry_zero = 0, tie_seen = 0;          // uniform over the workgroup
  for (int64_t base = 0; base < stride; base += kTile) {
    // ---- the lane's four ids; past the row's end: 0, which ends the row
    int tok[kPerLane];
    const int64_t at = base + tid * kPerLane;
    if (vec && at + kPerLane <= stride) {
      const int4 v = *reinterpret_cast<const int4*>(row + at);
      tok[0] = v.x, tok[1] = v.y, tok[2] = v.z, tok[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) tok[j] = at + j < stride ? row[at + j] : 0;
    }
    // ---- 1 + 2: the lane's part
    int end = kTile, tie = kTile, kp[kPerLane], kv[kPerLane], run_p = 0, run_v = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int l = tid * kPerLane + j;
      if (tok[j] <= 1) end = min(end, l);
      if (tok[j] == n.g.tie_id) tie = min(tie, l);
      const uint32_t pv = static_cast<uint32_t>(tok[j] - n.g.program_first);
      const uint32_t vv = static_cast<uint32_t>(tok[j] - n.velocity_first);
      if (pv < static_cast<uint32_t>(R)) run_p = ((l + 1) << 8) | static_cast<int>(pv);
      if (vv < static_cast<uint32_t>(n.velocity_count)) run_v = ((l + 1) << 1) | (vv == 0 ? 1 : 0);
      kp[j] = run_p, kv[j] = run_v;          // keys grow with the position: the running value IS the running max
    }
    // ---- the wave's part, then the four waves through LDS
    const int w_end = wave_min(end), w_tie = wave_min(tie);
    const int inc_p = mt3k::wave_scan_max(run_p, lane), inc_v = mt3k::wave_scan_max(run_v, lane);
    int before_p = __shfl_up(inc_p, 1), before_v = __shfl_up(inc_v, 1);          // the lanes before this one
    if (lane == 0) before_p = 0, before_v = 0;
    if (lane == 63) s_prog[wave] = inc_p, s_vel[wave] = inc_v;
    if (lane == 0) s_end[wave] = w_end, s_tie[wave] = w_tie;
    __syncthreads();
    int t_end = kTile, t_tie = kTile, tile_p = 0, tile_v = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      t_end = min(t_end, s_end[w]);
      t_tie = min(t_tie, s_tie[w]);
      if (w < wave) before_p = max(before_p, s_prog[w]), before_v = max(before_v, s_vel[w]);
      tile_p = max(tile_p, s_prog[w]), tile_v = max(tile_v, s_vel[w]);
    }
    // ---- 3: the pitch ids before the row's end
    int key[kPerLane], pair[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int l = tid * kPerLane + j;
      const uint32_t p = static_cast<uint32_t>(tok[j] - n.g.pitch_first);
      key[j] = 0;
      if (l < t_end && p < static_cast<uint32_t>(P)) {
        const int seen_p = max(before_p, kp[j]), seen_v = max(before_v, kv[j]);
        const int prog = seen_p ? (seen_p & 0xff) : carry_prog;
        const int zero = seen_v ? (seen_v & 1) : carry_zero;
        const int in_tie = !tie_seen && l < t_tie;
        key[j] = ((l + 1) << 1) | ((in_tie || !zero) ? 1 : 0);
        pair[j] = prog * P + static_cast<int>(p);
        atomicMax(&s_last[pair[j]], key[j]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      if (key[j] && s_last[pair[j]] == key[j]) {
        const int prog = pair[j] / P, p = pair[j] - prog * P;
        uint32_t* w = &s_held[prog * RW + (p >> 5)];
        if (key[j] & 1)
          atomicOr(w, 1u << (p & 31));
        else
          atomicAnd(w, ~(1u << (p & 31)));
        s_last[pair[j]] = 0;
      }
    }
    __syncthreads();
    if (t_end < kTile) break;                                  // the row ends in this tile
    if (tile_p) carry_prog = tile_p & 0xff;
    if (tile_v) carry_zero = tile_v & 1;
    tie_seen |= t_tie < kTile;
  }

  // ---- the section
  int mine = 0;
  if (tid < R)
    for (int w = 0; w < RW; ++w) mine += __popc(s_held[tid * RW + w]);
  const int packed = (mine << 8) | (mine ? 1 : 0);
  if (tid == 0) s_tie_at = 0;                                  // nothing kept: the bare tie_id
  int excl, total;
  mt3k::block_scan_add<kWaves>(packed, s_sum, &excl, &total);  // (its barrier publishes s_tie_at too)
  const int pairs = total >> 8, kept = min(pairs, cap);
  const bool drop = (flags & MT3_TIE_DROP_REDUNDANT_PROGRAMS) != 0;
  int32_t* out = prompts + static_cast<size_t>(blockIdx.x) * (2 * static_cast<size_t>(cap) + 1);
  if (mine) {
    int k = excl >> 8;                                         // the index of the row's first pair
    const int m = excl & 0xff;                                 // non-empty rows before this one
    const int prog_id = n.g.program_first + tid;
    if (drop && k < cap) out[k + m] = prog_id;
    for (int w = 0; w < RW; ++w) {
      uint32_t bits = s_held[tid * RW + w];
      while (bits && k < cap) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        const int64_t o = drop ? static_cast<int64_t>(k) + m + 1 : 2 * static_cast<int64_t>(k) + 1;
        if (!drop) out[o - 1] = prog_id;
        out[o] = n.g.pitch_first + w * 32 + b;
        if (k == kept - 1) s_tie_at = o + 1;
        ++k;
      }
    }
  }
  __syncthreads();
  const int64_t tie_at = s_tie_at, len = 2 * static_cast<int64_t>(cap) + 1;
  if (tid == 0) {
    out[tie_at] = n.g.tie_id;
    count[blockIdx.x] = pairs;
  }
  for (int64_t i = tie_at + 1 + tid; i < len; i += kThreads) out[i] = 0;
  if (held_out)
    for (int i = tid; i < W; i += kThreads) held_out[static_cast<size_t>(blockIdx.x) * W + i] = s_held[i];
}

const char* bad_args(const mt3_note_grammar* n, int32_t cap, int32_t flags) {
  if (!n) return "null descriptor";
  if (mt3_note_grammar_check(n, INT32_MAX) != MT3_OK) return nullptr;          // the message is mt3_last_error()'s
  if (cap < 0 || cap > (1 << 30) - 1) return "cap must be in [0, 2^30)";
  if (flags & ~MT3_TIE_DROP_REDUNDANT_PROGRAMS) return "unknown flags";
  return "";
}

int refuse(const char* who, const mt3_note_grammar* n, int32_t cap, int32_t flags) {
  const char* bad = bad_args(n, cap, flags);
  if (bad && !*bad) return MT3_OK;
  const std::string why = bad ? std::string(bad) : std::string(mt3_last_error());
  return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": " + why);
}

}  // namespace

extern "C" int32_t mt3_note_grammar_tie_prompt(const mt3_note_grammar* n, const int32_t* h_row, int32_t len, int32_t cap,
                                               int32_t flags, int32_t* h_prompt, uint32_t* h_held) {
  const char* who = "mt3_note_grammar_tie_prompt";
  if (const int rc = refuse(who, n, cap, flags)) return rc;
  if (len < 1) return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": len must be at least 1");
  if (!h_row || !h_prompt) return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": null argument");
  uint32_t held[kMaxWords];
  mt3n_replay(n, h_row, len, held);
  if (h_held)
    for (int w = 0; w < mt3n_table_words(n); ++w) h_held[w] = held[w];
  return mt3n_tie_section(n, held, cap, flags, h_prompt);
}

extern "C" int mt3_op_tie_prompts(const mt3_note_grammar* n, const int32_t* d_ids, int32_t rows, int32_t ids_stride,
                                  int32_t cap, int32_t flags, int32_t* d_prompts, int32_t* d_count, uint32_t* d_held,
                                  void* stream) {
  const char* who = "mt3_op_tie_prompts";
  if (const int rc = refuse(who, n, cap, flags)) return rc;
  if (rows < 1) return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": rows must be at least 1");
  if (ids_stride < 1) return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": ids_stride must be at least 1");
  if (!d_ids || !d_prompts || !d_count) return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": null argument");
  hipLaunchKernelGGL(tie_prompts_kernel, dim3(static_cast<uint32_t>(rows)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), *n, d_ids, ids_stride, cap, flags, d_prompts, d_count, d_held);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}
