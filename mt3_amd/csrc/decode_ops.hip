// Small bandwidth/latency kernels around the decode loop (gfx950).
//
//   rmsnorm_kernel      T5 LayerNorm (mt3/layers.py:604-621) as a standalone pass -- used once per
//                       encode for `encoder_norm` (network.py:192); every other norm is fused into
//                       the GEMM that consumes it (gemm.hip NORM).
//   embed_kernel        Embed (one-hot matmul in the reference, layers.py:530-533 -> a row gather)
//                       + FixedEmbed decode slice pos[t] (layers.py:589-596).
//   argmax_step_kernel  greedy pick of the step (lowest id on ties), EOS bookkeeping, writes
//                       ids[b][t]; rows that already emitted EOS get 0 (pad).  BEAM1 variant: one step
//                       of t5x beam_search with num_decodes=1 (top-2 of log_softmax, live/finished sets).
//                       Positions are PER-ROW device counters (no cross-row sync), so ONE captured
//                       hipGraph serves every step; the block also writes the next step's embedding row.
//   beam_step_kernel    one step of t5x beam_search with num_decodes = k (mt3_engine_decode_beams): one wave per live
//                       beam, the k * 2k candidates merged in LDS, the slot -> cache-row map rewritten; with
//                       beam_reorder_kernel (K/V copies of forked rows) and beam_finalize_kernel (history backtrack).
//                       Both token kernels read up to two per-segment tables (SegTable in kernels.h): the MASKED
//                       instantiations count the logit of a token the slot's mask row disallows as -inf, the PROMPT
//                       instantiations emit the prompt row's token while the slot is inside it.  The GRAMMAR
//                       instantiations (TokenGrammar in kernels.h) keep one packed state per slot and count the ids the
//                       event grammar disallows in that state as -inf as well.
//   ids_to_tokens_kernel GenericTokenVocabulary._decode_tf (mt3/vocabularies.py:241-271), bit-exact.
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.h"
#include "device.h"
#include "kernels.h"

namespace mt3k {

template <typename CT>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                       CT* __restrict__ out_ct, float* __restrict__ out_f32,
                                                       int rows, int dim) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);          // one wave per row
  if (row >= rows) return;
  const float* xr = x + static_cast<size_t>(row) * dim;
  float ss = 0.f;
  for (int i = lane * 4; i < dim; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  const float rs = rsqrtf(ss / static_cast<float>(dim) + 1e-6f);
  for (int i = lane * 4; i < dim; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    const float4 sc = *reinterpret_cast<const float4*>(scale + i);
    const float y0 = v.x * rs * sc.x, y1 = v.y * rs * sc.y, y2 = v.z * rs * sc.z, y3 = v.w * rs * sc.w;
    if (out_f32) *reinterpret_cast<float4*>(out_f32 + static_cast<size_t>(row) * dim + i) = make_float4(y0, y1, y2, y3);
    if (out_ct) {
      CT* o = out_ct + static_cast<size_t>(row) * dim + i;
      o[0] = to_ct<CT>(y0);
      o[1] = to_ct<CT>(y1);
      o[2] = to_ct<CT>(y2);
      o[3] = to_ct<CT>(y3);
    }
  }
}

int launch_rmsnorm(int dtype, const float* x, const float* scale, void* out_ct, float* out_f32, int rows, int dim,
                   hipStream_t s) {
  if (!x || !scale || rows <= 0 || dim % 4 != 0) return mt3::fail(MT3_ERR_INVALID, "rmsnorm: bad arguments");
  const dim3 grid((rows + 3) / 4), block(256);
  if (dtype == MT3_BF16)
    hipLaunchKernelGGL((rmsnorm_kernel<__bf16>), grid, block, 0, s, x, scale, static_cast<__bf16*>(out_ct), out_f32,
                       rows, dim);
  else
    hipLaunchKernelGGL((rmsnorm_kernel<float>), grid, block, 0, s, x, scale, static_cast<float*>(out_ct), out_f32,
                       rows, dim);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// one float4 of a decoder-input row: the f32 value, for the split residual form the exact sum of squares of its
// 16-column group (4 consecutive lanes = one quad own one group), and for the bf16 path also its compute-type copy
// (y_ct == nullptr with y_ss != nullptr: the f32 engine, whose compute-type rows ARE the f32 rows)
__device__ __forceinline__ void put_row_piece(float4 v, float* y, void* y_ct, float* y_ss, size_t row, int dim, int i) {
  *reinterpret_cast<float4*>(y + row * dim + i) = v;
  if (y_ss) {
    float t = __builtin_fmaf(v.w, v.w, __builtin_fmaf(v.z, v.z, __builtin_fmaf(v.y, v.y, v.x * v.x)));
    t = quad_sum(t);
    if ((threadIdx.x & 3) == 0) y_ss[row * (dim >> 4) + (i >> 4)] = t;
  }
  if (y_ct) {
    uint2 pk;
    pk.x = pack_bf16x2(v.x, v.y);
    pk.y = pack_bf16x2(v.z, v.w);
    *reinterpret_cast<uint2*>(static_cast<__bf16*>(y_ct) + row * dim + i) = pk;
  }
}

// the split form of residual rows that did not come out of a RESID epilogue (the encoder's input projection):
// f32 rows -> bf16 copy + exact per-16-column sums of squares; one float4 per thread, a quad per 16-column group
__global__ __launch_bounds__(256) void residual_split_kernel(const float* __restrict__ x, void* __restrict__ x_ct,
                                                              float* __restrict__ x_ss, size_t n4, int dim) {
  const size_t i4 = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool in = i4 < n4;
  const float4 v = in ? reinterpret_cast<const float4*>(x)[i4] : make_float4(0.f, 0.f, 0.f, 0.f);
  float t = __builtin_fmaf(v.w, v.w, __builtin_fmaf(v.z, v.z, __builtin_fmaf(v.y, v.y, v.x * v.x)));
  t = quad_sum(t);
  if (!in) return;
  if ((threadIdx.x & 3) == 0) x_ss[i4 >> 2] = t;         // [row][dim/16] == flat index / 16
  uint2 pk;
  pk.x = pack_bf16x2(v.x, v.y);
  pk.y = pack_bf16x2(v.z, v.w);
  reinterpret_cast<uint2*>(x_ct)[i4] = pk;
}

int launch_residual_split(const float* x, void* x_ct, float* x_ss, int rows, int dim, hipStream_t s) {
  if (!x || !x_ct || !x_ss || rows <= 0 || dim % 16) return mt3::fail(MT3_ERR_INVALID, "residual_split: bad arguments");
  const size_t n4 = static_cast<size_t>(rows) * dim / 4;
  hipLaunchKernelGGL(residual_split_kernel, dim3(static_cast<unsigned>((n4 + 255) / 256)), dim3(256), 0, s, x, x_ct,
                     x_ss, n4, dim);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// q_out[b] = ew[tok] + pw[t]: the first decoder layer's unnormalised q | k | v | cross-q of the row (RowProj)
__device__ __forceinline__ void put_row_projection(const RowProj& rp, int b, int tok, int t, int tid, int nthreads) {
  const float* e = rp.ew + static_cast<size_t>(tok) * rp.q_n;
  const float* p = rp.pw + static_cast<size_t>(t) * rp.q_n;
  float* o = rp.q_out + static_cast<size_t>(b) * rp.q_n;
  for (int i = tid * 4; i < rp.q_n; i += nthreads * 4) {
    const float4 a = *reinterpret_cast<const float4*>(e + i), c = *reinterpret_cast<const float4*>(p + i);
    *reinterpret_cast<float4*>(o + i) = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
  }
}

// The one writer of a decoder input row (InputRow): slot's row = table[tok] + pos[min(t, max_pos - 1)] in every form
// present -- f32, bf16 copy, per-16-column sums of squares, layer 0's projection by table lookup -- by the `nthreads`
// threads tid = 0 .. nthreads - 1 of a block (or of a wave: nthreads = 64, tid = lane).  The result does not depend on
// nthreads: each 16-column sum of squares is formed by ONE quad (tid & 3 == threadIdx.x & 3 for every caller) with
// put_row_piece's fmaf chain and quad_sum, and with dim % 16 == 0 a quad is wholly inside or wholly outside the row.
__device__ __forceinline__ void put_input_row(const InputRow& r, int slot, int tok, int t, int tid, int nthreads) {
  if (t >= r.max_pos) t = r.max_pos - 1;
  const float* e = r.table + static_cast<size_t>(tok) * r.dim;
  const float* p = r.pos + static_cast<size_t>(t) * r.dim;
  for (int i = tid * 4; i < r.dim; i += nthreads * 4) {
    const float4 a = *reinterpret_cast<const float4*>(e + i), c = *reinterpret_cast<const float4*>(p + i);
    put_row_piece(make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w), r.y, r.y_ct, r.y_ss, slot, r.dim, i);
  }
  if (r.rp.q_out) put_row_projection(r.rp, slot, tok, t, tid, nthreads);
}

// the one host-side check of an InputRow: MT3_OK, or the failure of launcher `who` (r.y == nullptr: a kernel that
// writes no row, which then cannot write a projection either)
static int bad_input_row(const InputRow& r, const char* who) {
  const char* bad = nullptr;
  if (r.rp.q_out && (!r.y || !r.rp.ew || !r.rp.pw || r.rp.q_n % 4))
    bad = ": row projection needs the row output and its tables";
  else if (r.y && (!r.table || !r.pos || r.max_pos < 1 || r.dim <= 0 || r.dim % 4))
    bad = ": the input row needs its tables and dim % 4 == 0";
  else if (r.y && (r.y_ct || r.y_ss) && (!r.y_ss || r.dim % 16))
    bad = ": the split form needs y_ss and dim % 16 == 0";
  return bad ? mt3::fail(MT3_ERR_INVALID, std::string(who) + bad) : MT3_OK;
}

__global__ __launch_bounds__(128) void embed_kernel(InputRow in, const int* __restrict__ tok, const int* __restrict__ step) {
  put_input_row(in, blockIdx.x, tok[blockIdx.x], step[blockIdx.x], threadIdx.x, 128);
}

int launch_embed(const InputRow& in, const int* tok, const int* step, int B, hipStream_t s) {
  if (!in.y || !tok || !step) return mt3::fail(MT3_ERR_INVALID, "embed: bad arguments");
  if (const int rc = bad_input_row(in, "embed")) return rc;
  hipLaunchKernelGGL(embed_kernel, dim3(B), dim3(128), 0, s, in, tok, step);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// order of candidates: larger logit first, lower id on ties (lax.top_k / argmax convention)
__device__ inline bool cand_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

struct Top2 {
  float v1, v2;
  int i1, i2;
  __device__ inline void insert(float v, int i) {
    if (cand_better(v, i, v1, i1)) {
      v2 = v1;
      i2 = i1;
      v1 = v;
      i1 = i;
    } else if (cand_better(v, i, v2, i2)) {
      v2 = v;
      i2 = i;
    }
  }
};

// the segment slot `slot` decodes: what the EOS schedule, the masks and the prompts are indexed by.  slot_seg: the in-flight
// map (nullptr: `direct`, the row the slot decodes / the beam kernel's block)
__device__ __forceinline__ int slot_segment(const int* slot_seg, int slot, int direct) {
  return slot_seg ? slot_seg[slot] : direct;
}
// the row of segment `seg` in a per-segment table (SegTable, kernels.h), nullptr = none; never indexes with a negative
// segment or row index
template <typename T>
__device__ __forceinline__ const T* seg_table_row(const SegTable<T>& tb, int seg) {
  if (seg < 0) return nullptr;
  const int r = tb.seg_row ? tb.seg_row[seg] : 0;
  return r < 0 ? nullptr : tb.rows + static_cast<size_t>(r) * tb.stride;
}

// Constrained decoding (TokenMask): what a logit mask ahead of t5x `beam_search` does -- a disallowed token's logit is
// -inf wherever the token rule reads it.  (t5x is not at hand: written from memory, as the beam rule is.)
constexpr float kMaskedLogit = -__builtin_inff();
__device__ __forceinline__ bool mask_allows(uint32_t word, int i) { return (word >> (i & 31)) & 1u; }
// row[i] as the token rule reads it in the loops that walk the row in memory (vocab > 2048)
// (GRAMMAR: also -inf where the event grammar `g` disallows id i in the slot's state `gs`)
template <bool MASKED, bool GRAMMAR = false>
__device__ __forceinline__ float rule_logit(const float* row, const uint32_t* mrow, int i,
                                            const mt3_token_grammar* g = nullptr, int gs = 0) {
  if (MASKED && mrow && !mask_allows(mrow[i >> 5], i)) return kMaskedLogit;
  if (GRAMMAR && !mt3g_allowed(g, gs, i)) return kMaskedLogit;
  return row[i];
}

// Note-consistent decoding (TokenNotes; the rule: include/mt3_hip.h, mt3n_*).  What the NOTES instantiations read of a slot
// before the pick: the `note` int and the copy of the current program's row, both at addresses that need only the slot index.
struct NoteView {
  int note;
  uint32_t row[MT3_NOTE_ROW_WORDS];
};
__device__ __forceinline__ NoteView load_note_view(const SlotState& st, size_t slot) {
  NoteView v;
  v.note = st.note[slot];
#pragma unroll
  for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x) v.row[x] = st.nrow[slot * MT3_NOTE_ROW_WORDS + x];
  return v;
}
// row[i] under the mask, the grammar and the note rule (the loops that walk the row in memory)
template <bool MASKED>
__device__ __forceinline__ float rule_logit_notes(const float* row, const uint32_t* mrow, int i, const mt3_note_grammar* n,
                                                  int gs, const NoteView& nv) {
  if (MASKED && mrow && !mask_allows(mrow[i >> 5], i)) return kMaskedLogit;
  if (!mt3g_allowed(&n->g, gs, i) || !mt3n_allowed_extra(n, gs, nv.note, nv.row, i)) return kMaskedLogit;
  return row[i];
}
// The note state of slot `dst` after it emits `tok` from the state (gs, nv) its PARENT held before the step.  fork: dst is
// not the parent's slot (a k-beam fork: the caller has copied the parent's table over with the pitch's bit applied on the
// way, and dst's `note` and row copy are written in full); otherwise only what changes is written.  new_row: the row of the
// new program where the caller has read it already (from the parent's table), else it is read from dst's own.  Called by
// the one thread that owns dst's bookkeeping: plain vector read-modify-writes; the pitch's word comes from the row copy, so
// only a program change reads the table.
__device__ __forceinline__ void note_commit(const mt3_note_grammar& n, const SlotState& st, size_t dst, int gs,
                                            const NoteView& nv, int tok, const uint32_t* new_row, bool fork) {
  const int W = mt3n_row_words(&n);
  const int nn = mt3n_note_advance(&n, nv.note, tok);
  int pitch = 0;
  const int eff = mt3n_pitch_effect(&n, gs, nv.note, tok, &pitch);
  uint32_t* tab = st.held + dst * st.held_words;
  uint32_t* nrow = st.nrow + dst * MT3_NOTE_ROW_WORDS;
  uint32_t r[MT3_NOTE_ROW_WORDS];
#pragma unroll
  for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x) r[x] = nv.row[x];
  const bool new_prog = ((nn ^ nv.note) & static_cast<int>(MT3_NOTE_PROGRAM)) != 0;
  if (eff) {
    const int w = pitch >> 5;
    const uint32_t bit = 1u << (pitch & 31), v = eff == 1 ? (nv.row[w] | bit) : (nv.row[w] & ~bit);
#pragma unroll
    for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x)
      if (x == w) r[x] = v;
    if (!fork) {
      tab[(static_cast<uint32_t>(nv.note) & MT3_NOTE_PROGRAM) * W + w] = v;
      nrow[w] = v;
    }
  } else if (new_prog) {
#pragma unroll
    for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x)
      r[x] = x < W ? (new_row ? new_row[x] : tab[(static_cast<uint32_t>(nn) & MT3_NOTE_PROGRAM) * W + x]) : 0u;
  }
  if (fork || (new_prog && !eff)) {
#pragma unroll
    for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x) nrow[x] = r[x];
  }
  if (fork || nn != nv.note) st.note[dst] = nn;
}

// Prompted decoding (TokenPrompt): the prompt token of segment `seg` at position t, 0 = the slot is past its prompt or has
// none; never reads a position at or past the stride
__device__ __forceinline__ int prompt_token(const TokenPrompt& tp, int seg, int t) {
  if (t >= tp.stride) return 0;
  const int* row = seg_table_row(tp, seg);
  return row ? row[t] : 0;
}

// BEAM1 = false: greedy pick (the product default).
// BEAM1 = true : one step of t5x `beam_search` with num_decodes = 1: the two best
//   candidates of log_softmax are taken; the LIVE hypothesis follows the best non-EOS one; an EOS candidate
//   finishes `live prefix + EOS` with score (live_logp + logp_eos) / brevity_penalty(t + 1), kept if it
//   beats the best finished score of the row; the row is done once that score exceeds
//   live_logp / brevity_penalty(max_len + 1), after which no later finish can win.  beam_f holds
//   [live_logp | best_score] per row, beam_len the prefix length of the best finished hypothesis (-1: none);
//   beam_cfg[0] = brevity_penalty(max_len + 1) of this call, beam_cfg[1 + n] = brevity_penalty(n) =
//   ((5 + n) / 6) ^ alpha, tabulated on the host.
// MASKED = true : a.tm restricts the pick of every slot to its segment's allowed tokens (exactly 0 in the exp-sum, never a
//   candidate); the logits in memory, scaled or not, stay the model's own.  MASKED = false compiles from the statements
//   the kernel had before masks existed.
// PROMPT = true : a slot at a position inside its segment's prompt (a.tp) emits the prompt's token P[t] whatever the
//   logits say -- the synthetic EOS schedule and the mask included -- and its next input row is written from P[t]; the
//   beam-1 state (live log-prob, finished score and length) is left alone and the stop test is not evaluated, so the slot
//   never finishes there but by max_len.  The branch is block-uniform.  PROMPT = false compiles from the statements the
//   kernel had before prompts existed.
// GRAMMAR = true: the pick of every slot is restricted to the ids the event grammar a.gr allows in the slot's state
//   st.gram[b] (the intersection with the mask; where the mask is applied), and the state is advanced by the token the slot
//   emits, free, forced by the prompt or by the EOS schedule.  A fourth flag, but only on the <MASKED, PROMPT> forms: a
//   grammar step without masks or prompts passes empty tables (no mask row: no word is loaded; stride 0: no prompt token).
//   GRAMMAR = false compiles from the statements the kernel had before the grammar existed.
// NOTES = true  : on top of GRAMMAR only (a.gr.g == a.nt.n.g): the pick is further restricted by the note rule in the slot's
//   note state (st.note[b] and the row copy st.nrow[b], requested with the grammar state: their addresses need only the
//   block index), and thread 0 advances that state by the token the slot emits.  NOTES = false compiles from the
//   statements the kernel had before the note rule existed.
template <bool BEAM1, bool MASKED, bool PROMPT, bool GRAMMAR = false, bool NOTES = false>
__global__ __launch_bounds__(256) void argmax_step_kernel(ArgmaxStepArgs a) {
  const SlotState& st = a.st;
  const StepRetire& rt = a.rt;
  const LogitScale& ls = a.ls;
  const int vocab = a.vocab;
  __shared__ float s_v[8], s_sum[4];
  __shared__ int s_i[8];
  __shared__ int s_tok, s_t;
  __shared__ float s_rs;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // row retirement: a finished slot is not touched again (its ids stay at the 0 they were initialised to, its
  // position counter stops: nothing reads it any more)
  if (rt.retire && st.done[b]) return;
  const int out_row = rt.slot_row ? rt.slot_row[b] : b;        // row of `ids` / `eos_at` this slot decodes
  float* __restrict__ row = a.logits + static_cast<size_t>(b) * vocab;
  // Round 6: the whole row in registers (vocab <= 2048: eight values per thread), requested in ONE batch before anything
  // that has to be waited for.  The loops this replaces walked the row three times, one element per thread and trip, each
  // trip a dependent load (the compiler waited for every load before the next): a dozen memory round trips in a kernel
  // that every decode step ends with (rocprofv3: 14.3 us per group step).  Same values, same insertion order, same bits.
  constexpr int kPer = 8;
  const bool in_regs = vocab <= 256 * kPer;
  float xv[kPer];
  if (in_regs) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = tid + u * 256;
      xv[u] = row[i < vocab ? i : vocab - 1];
    }
  }
  // MASKED: the mask word of each of those logits, requested in the same batch -- nothing has been waited for yet, so the
  // words ride behind the logits and cost no round trip of their own
  const uint32_t* mrow = nullptr;
  uint32_t mw[kPer];
  if (MASKED) {
    mrow = seg_table_row(a.tm, slot_segment(rt.slot_seg, b, out_row));
    if (in_regs) {
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int i = tid + u * 256;
        mw[u] = mrow ? mrow[(i < vocab ? i : vocab - 1) >> 5] : 0xffffffffu;
      }
    }
  }
  // PROMPT: the slot's prompt token at its own position, one dword per block requested in the same batch (0: not inside a
  // prompt); only thread 0 reads it
  int ptok = 0;
  if (PROMPT) ptok = prompt_token(a.tp, slot_segment(rt.slot_seg, b, out_row), st.step[b]);
  // GRAMMAR: the slot's packed state, one dword per block whose address needs nothing but the block index: requested in the
  // same batch, waited for only where the ids are tested below
  int gs = 0;
  if (GRAMMAR) gs = st.gram[b];
  NoteView nv{};
  if (NOTES) nv = load_note_view(st, b);
  // thread 0 issues its state loads up front so that their latency hides behind the reductions
  int was_done = 0, t = 0, blen = -1, eos_len = 0x7fffffff;
  float live = 0.f, best = 0.f, bp_max = 1.f, bp_t = 1.f;
  if (tid == 0) {
    was_done = st.done[b];
    t = st.step[b];
    if (rt.eos_at) eos_len = rt.eos_at[slot_segment(rt.slot_seg, b, out_row)];
    if (BEAM1) {
      live = a.beam.f[b];
      best = a.beam.f[a.beam.rows + b];
      blen = a.beam.len[b];
      bp_max = a.beam.cfg[0];
      bp_t = a.beam.cfg[1 + t + 1];
    }
  }
  if (ls.ss) {
    // folded logits projection: the row arrives unnormalised; 1/rms of the final residual row from its partial sums
    // (<= 64 of them: one wave), then the scaled logits replace the raw ones (callers read them: first-step /
    // per-step logits) -- arg-max would not need the scale, the beam's log-softmax and the parity outputs do
    if (wave == 0) {
      float p = lane < ls.n_ss ? ls.ss[static_cast<size_t>(b) * ls.n_ss + lane] : 0.f;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
      if (lane == 0) s_rs = rsqrtf(p / static_cast<float>(ls.dim) + 1e-6f);
    }
    __syncthreads();
    const float rs = s_rs;
    if (in_regs) {
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int i = tid + u * 256;
        xv[u] *= rs;
        if (i < vocab) row[i] = xv[u];
      }
    } else {
      for (int i = tid; i < vocab; i += 256) row[i] *= rs;
      // (each thread re-reads below exactly the elements it just wrote: no barrier needed)
    }
  }
  if (MASKED && in_regs) {                 // after the scale and its write-back: memory keeps the model's logits
#pragma unroll
    for (int u = 0; u < kPer; ++u)
      if (!mask_allows(mw[u], tid)) xv[u] = kMaskedLogit;      // (i & 31 == tid & 31: i = tid + 256 u)
  }
  if (GRAMMAR && in_regs) {                // a handful of integer compares on the id each thread already knows
#pragma unroll
    for (int u = 0; u < kPer; ++u)
      if (!mt3g_allowed(&a.gr.g, gs, tid + u * 256)) xv[u] = kMaskedLogit;
  }
  if (NOTES && in_regs) {
#pragma unroll
    for (int u = 0; u < kPer; ++u)
      if (!mt3n_allowed_extra(&a.nt.n, gs, nv.note, nv.row, tid + u * 256)) xv[u] = kMaskedLogit;
  }
  Top2 t2{-3.0e38f, -3.0e38f, 0x7fffffff, 0x7fffffff};
  float acc = 0.f;
  if (in_regs) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {                               // ascending i per thread
      const int i = tid + u * 256;
      if (i < vocab) t2.insert(xv[u], i);
    }
    if (BEAM1) {
      // sum of exp(x - thread max) over this thread's elements; rescaled to the wave max below
#pragma unroll
      for (int u = 0; u < kPer; ++u)
        if (tid + u * 256 < vocab) acc += __expf(xv[u] - t2.v1);
    }
  } else if (NOTES) {
    for (int i = tid; i < vocab; i += 256) t2.insert(rule_logit_notes<MASKED>(row, mrow, i, &a.nt.n, gs, nv), i);
    if (BEAM1) {
      for (int i = tid; i < vocab; i += 256) acc += __expf(rule_logit_notes<MASKED>(row, mrow, i, &a.nt.n, gs, nv) - t2.v1);
    }
  } else {
    for (int i = tid; i < vocab; i += 256)                                                   // ascending i per thread
      t2.insert(rule_logit<MASKED, GRAMMAR>(row, mrow, i, &a.gr.g, gs), i);
    if (BEAM1) {
      for (int i = tid; i < vocab; i += 256) acc += __expf(rule_logit<MASKED, GRAMMAR>(row, mrow, i, &a.gr.g, gs) - t2.v1);
    }
  }
  const float own_max = t2.v1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov1 = __shfl_xor(t2.v1, o), ov2 = __shfl_xor(t2.v2, o);
    const int oi1 = __shfl_xor(t2.i1, o), oi2 = __shfl_xor(t2.i2, o);
    t2.insert(ov1, oi1);
    if (BEAM1) t2.insert(ov2, oi2);
  }
  if (BEAM1) {
    acc *= __expf(own_max - t2.v1);                     // every lane now holds the wave max in t2.v1
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  }
  if (lane == 0) {
    s_v[wave] = t2.v1;
    s_i[wave] = t2.i1;
    s_v[4 + wave] = t2.v2;
    s_i[4 + wave] = t2.i2;
    s_sum[wave] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    float m = t2.v1;                                    // wave 0's max; the block max after the merge
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      t2.insert(s_v[w], s_i[w]);
      if (BEAM1) t2.insert(s_v[4 + w], s_i[4 + w]);
    }
    int tok;
    bool finished = false;                // this step finishes the slot
    if (PROMPT && ptok != 0) {
      // inside the prompt: the token is given, nothing is scored, no EOS candidate is made and the stop test is skipped
      tok = was_done ? 0 : ptok;
      if (BEAM1 && !was_done) a.beam.len_row[out_row] = blen;
    } else if (!BEAM1) {
      if (a.forced) was_done = 0;           // teacher forcing: every step reports its own arg-max, no EOS bookkeeping
      tok = was_done ? 0 : (t + 1 >= eos_len ? 1 : t2.i1);      // synthetic EOS schedule: a point mass on EOS
      finished = !was_done && tok == 1 && !a.forced;   // EOS
    } else {
      tok = 0;
      if (!was_done) {
        m = t2.v1;
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) sum += s_sum[w] * __expf(s_v[w] - m);
        const float lse = m + __logf(sum);
        float lp1 = t2.v1 - lse, lp2 = t2.v2 - lse;
        int eos_slot = t2.i1 == 1 ? 1 : (t2.i2 == 1 ? 2 : 0);
        if (t + 1 >= eos_len) {           // synthetic EOS schedule: EOS with probability 1, everything else impossible
          eos_slot = 1;
          lp1 = 0.f;
          lp2 = -1.0e30f;
        }
        if (eos_slot) {
          const float score = (live + (eos_slot == 1 ? lp1 : lp2)) / bp_t;
          if (blen < 0 || score > best) {
            best = score;
            blen = t;
          }
        }
        tok = eos_slot == 1 ? t2.i2 : t2.i1;
        live += eos_slot == 1 ? lp2 : lp1;
        a.beam.f[b] = live;
        a.beam.f[a.beam.rows + b] = best;
        a.beam.len[b] = blen;
        a.beam.len_row[out_row] = blen;
        finished = blen >= 0 && best > live / bp_max;
      }
    }
    // in-flight batching: a slot that has written max_len ids is finished as well (the row ran out of positions)
    if (!was_done && rt.max_len > 0 && t + 1 >= rt.max_len) finished = true;
    if (finished) {
      st.done[b] = 1;
      atomicAdd(st.n_done, 1);
    }
    a.ids[static_cast<size_t>(out_row) * a.ids_stride + t] = tok;
    if (GRAMMAR && !was_done) st.gram[b] = mt3g_advance(&a.gr.g, gs, tok);   // a finished slot keeps its last state
    if (NOTES && !was_done) note_commit(a.nt.n, st, b, gs, nv, tok, nullptr, false);
    // teacher forcing (Transformer.decode on given decoder_input_tokens, network.py:303-361): the NEXT input is
    // the caller's token for position t + 1, whatever this step predicted
    if (!BEAM1 && a.forced) tok = a.forced[static_cast<size_t>(b) * a.forced_stride + t];
    st.cur_tok[b] = tok;
    st.step[b] = t + 1;
    s_tok = tok;
    s_t = t + 1;
  }
  __syncthreads();
  // the next step's decoder input row: Embed(tok) + FixedEmbed[t+1]  (saves the embed launch of every step)
  if (a.in.y) put_input_row(a.in, b, s_tok, s_t, tid, 256);
}

int launch_argmax_step(const ArgmaxStepArgs& a, hipStream_t s) {
  const StepRetire& rt = a.rt;
  if (a.beam.f && a.forced) return mt3::fail(MT3_ERR_INVALID, "argmax_step: teacher forcing is a greedy-path feature");
  if (a.beam.f && !a.beam.len_row) return mt3::fail(MT3_ERR_INVALID, "argmax_step: the beam state needs its row-indexed lengths");
  if (a.forced && (rt.retire || rt.slot_row || rt.eos_at || rt.slot_seg || rt.max_len))
    return mt3::fail(MT3_ERR_INVALID, "argmax_step: teacher forcing keeps every row live and in place");
  if (a.ls.ss && (a.ls.n_ss <= 0 || a.ls.n_ss > 64 || a.ls.dim <= 0))
    return mt3::fail(MT3_ERR_INVALID, "argmax_step: the row scale needs 1 .. 64 partial sums");
  if (const int rc = bad_input_row(a.in, "argmax_step")) return rc;
  if (a.tm.rows && (a.forced || a.tm.stride != (a.vocab + 31) / 32))
    return mt3::fail(MT3_ERR_INVALID, "argmax_step: token masks are ceil(vocab / 32) words and not for teacher forcing");
  if (a.tp.rows && (a.forced || a.tp.stride < 1))
    return mt3::fail(MT3_ERR_INVALID, "argmax_step: prompts have a stride of at least 1 and are not for teacher forcing");
  if (a.gr.on && (a.forced || !a.st.gram || bad_token_grammar(a.gr.g, a.vocab)))
    return mt3::fail(MT3_ERR_INVALID, "argmax_step: the grammar needs the slots' states and valid ranges and is not for "
                                      "teacher forcing");
  if (a.nt.on && (!a.gr.on || !a.st.note || !a.st.nrow || !a.st.held || bad_note_grammar(a.nt.n, a.vocab) ||
                  a.st.held_words != mt3n_table_words(&a.nt.n) || std::memcmp(&a.nt.n.g, &a.gr.g, sizeof(a.gr.g)) != 0))
    return mt3::fail(MT3_ERR_INVALID, "argmax_step: the note rule needs its grammar set as the step's grammar, the slots' "
                                      "note states and a valid descriptor");
  void (*kernel)(ArgmaxStepArgs);
  if (a.nt.on) {
    kernel = a.beam.f ? argmax_step_kernel<true, true, true, true, true> : argmax_step_kernel<false, true, true, true, true>;
  } else if (a.gr.on) {
    kernel = a.beam.f ? argmax_step_kernel<true, true, true, true> : argmax_step_kernel<false, true, true, true>;
  } else if (a.tp.rows) {
    if (a.tm.rows) kernel = a.beam.f ? argmax_step_kernel<true, true, true> : argmax_step_kernel<false, true, true>;
    else kernel = a.beam.f ? argmax_step_kernel<true, false, true> : argmax_step_kernel<false, false, true>;
  } else {
    if (a.tm.rows) kernel = a.beam.f ? argmax_step_kernel<true, true, false> : argmax_step_kernel<false, true, false>;
    else kernel = a.beam.f ? argmax_step_kernel<true, false, false> : argmax_step_kernel<false, false, false>;
  }
  hipLaunchKernelGGL(kernel, dim3(a.B), dim3(256), 0, s, a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ---------------------------------------------------------------------------------------------- temperature sampling
// Order-preserving integer image of a logit: a larger float has a larger key (-0.f counts as +0.f, as cand_better's ==
// counts them).  With the id below it, (key << 11) | (2047 - id) orders the candidates of a row of <= 2048 ids exactly as
// cand_better does -- larger logit first, lower id on ties -- and no two candidates share a value.
__device__ __forceinline__ unsigned long long cand_key(float v, int i) {
  const uint32_t b = __float_as_uint(v == 0.f ? 0.f : v);
  const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (static_cast<unsigned long long>(o) << 11) | static_cast<unsigned long long>(2047 - i);
}

// One decode step of temperature sampling (SampleStepArgs; the rule: include/mt3_hip.h): argmax_step_kernel's greedy
// form -- the row in registers, the LogitScale multiply and its write-back, masks, prompts, the grammar, the EOS schedule,
// max_len, retirement, the next input row -- with the pick of a free position drawn instead of taken.  One block of 256
// per slot, eight values per thread (vocab <= 2048).
//   kept set   a THRESHOLD SEARCH, not a sort: every candidate carries an integer weight (top-k: 1; top-p: its softmax
//              mass in units of 2^-40 of the largest), and the key of the last kept candidate is the one at which the
//              weight of all candidates at or above it first reaches the target (k, or ceil(p * total)).  It is found 8 bits
//              at a time from the top of the 43-bit key: a 256-bin histogram of the weights in LDS (integer atomics: the
//              sums do not depend on the order of arrival, so the step is bitwise reproducible), a suffix scan over the
//              bins by one thread per bin, and the bin that crosses the target fixes the digit; six rounds.
//   noise      mt3s_bits / mt3s_gumbel for the kept candidates only: the draw of (seed, stream, position, id) does not
//              depend on who else is kept.
//   pick       the cand_better-best of z + g: per thread, per wave by shuffles, over the four waves by thread 0.
// Every branch on the slot's state (done, inside its prompt, at its scheduled EOS) is block-uniform.
// NOTES = true: the note rule on top of the grammar (a.nt; argmax_step_kernel's NOTES form says how); NOTES = false compiles
// from the statements the kernel had before the note rule existed.
// SEEDS = true: the Philox key of a slot is its segment's entry of sa.seed (a table indexed as sa.stream is; no row: the
// parameters' seed); SEEDS = false compiles from the statements the kernel had before the seed table existed.
template <bool NOTES, bool SEEDS>
__global__ __launch_bounds__(256) void sample_step_kernel(SampleStepArgs sa) {
  const ArgmaxStepArgs& a = sa.a;
  const SlotState& st = a.st;
  const StepRetire& rt = a.rt;
  const LogitScale& ls = a.ls;
  const int vocab = a.vocab;
  __shared__ unsigned long long s_hist[256], s_wsum[4], s_tot[4], s_target;
  __shared__ float s_v[4], s_m[4];
  __shared__ int s_i[4];
  __shared__ int s_tok, s_t, s_digit;
  __shared__ float s_rs;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (rt.retire && st.done[b]) return;
  const int out_row = rt.slot_row ? rt.slot_row[b] : b;
  float* __restrict__ row = a.logits + static_cast<size_t>(b) * vocab;
  constexpr int kPer = 8;
  // the row in registers, its mask words, the prompt token, the grammar state and the slot's counters: one batch of loads
  float xv[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = tid + u * 256;
    xv[u] = row[i < vocab ? i : vocab - 1];
  }
  const int seg = slot_segment(rt.slot_seg, b, out_row);
  const uint32_t* mrow = a.tm.rows ? seg_table_row(a.tm, seg) : nullptr;
  uint32_t mw[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int i = tid + u * 256;
    mw[u] = mrow ? mrow[(i < vocab ? i : vocab - 1) >> 5] : 0xffffffffu;
  }
  const int t = st.step[b], was_done = st.done[b];
  const int ptok = a.tp.rows ? prompt_token(a.tp, seg, t) : 0;
  const int gs = a.gr.on ? st.gram[b] : 0;
  NoteView nv{};
  if (NOTES) nv = load_note_view(st, b);
  const int eos_len = rt.eos_at ? rt.eos_at[seg] : 0x7fffffff;
  const mt3_sampling sp = *sa.params;
  const uint64_t* srow = sa.stream.rows ? seg_table_row(sa.stream, seg) : nullptr;
  const uint64_t stream = srow ? *srow : static_cast<uint64_t>(static_cast<int64_t>(sa.seg0) + seg);
  uint64_t seed = sp.seed;
  if (SEEDS) {
    const uint64_t* krow = seg_table_row(sa.seed, seg);
    if (krow) seed = *krow;
  }
  if (ls.ss) {                                           // the folded logits projection, as the greedy kernel applies it
    if (wave == 0) {
      float p = lane < ls.n_ss ? ls.ss[static_cast<size_t>(b) * ls.n_ss + lane] : 0.f;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
      if (lane == 0) s_rs = rsqrtf(p / static_cast<float>(ls.dim) + 1e-6f);
    }
    __syncthreads();
    const float rs = s_rs;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = tid + u * 256;
      xv[u] *= rs;
      if (i < vocab) row[i] = xv[u];
    }
  }
  const bool free_pick = !was_done && ptok == 0 && t + 1 < eos_len;
  int pick = 0x7fffffff;                                 // thread 0's, after the block below
  if (free_pick) {
    // the candidates: ids of the vocabulary whose logit the mask and the grammar leave above -inf
    float z[kPer];
    unsigned long long key[kPer];
    bool keep[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = tid + u * 256;
      bool c = i < vocab && mask_allows(mw[u], tid) && xv[u] > kMaskedLogit;     // (i & 31 == tid & 31)
      if (c && a.gr.on) c = mt3g_allowed(&a.gr.g, gs, i);
      if (NOTES && c) c = mt3n_allowed_extra(&a.nt.n, gs, nv.note, nv.row, i);
      keep[u] = c;
      z[u] = c ? xv[u] / sp.temperature : kMaskedLogit;
      key[u] = c ? cand_key(xv[u], i) : 0ull;
    }
    if (sp.top_k > 0 || sp.top_p > 0.f) {
      unsigned long long w[kPer];
      if (sp.top_k > 0) {
#pragma unroll
        for (int u = 0; u < kPer; ++u) w[u] = keep[u] ? 1ull : 0ull;
      } else {
        float m = kMaskedLogit;
#pragma unroll
        for (int u = 0; u < kPer; ++u) m = fmaxf(m, z[u]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) s_m[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
#pragma unroll
        for (int u = 0; u < kPer; ++u)                   // softmax mass in units of 2^-40 of the largest, truncated
          w[u] = keep[u] ? static_cast<unsigned long long>(expf(z[u] - m) * 1099511627776.0f) : 0ull;
      }
      unsigned long long tot = 0;
#pragma unroll
      for (int u = 0; u < kPer; ++u) tot += w[u];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
      if (lane == 0) s_tot[wave] = tot;
      __syncthreads();
      tot = s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
      unsigned long long target;
      if (sp.top_k > 0) {
        target = static_cast<unsigned long long>(sp.top_k);
      } else {
        target = static_cast<unsigned long long>(ceil(static_cast<double>(sp.top_p) * static_cast<double>(tot)));
        if (target < 1) target = 1;
      }
      if (target > tot) target = tot;
      unsigned long long prefix = 0;                     // the digits of the threshold key found so far
      if (tot > 0) {
        for (int shift = 40; shift >= 0; shift -= 8) {
          s_hist[tid] = 0;
          __syncthreads();
#pragma unroll
          for (int u = 0; u < kPer; ++u)
            if (w[u] && (key[u] >> (shift + 8)) == (prefix >> (shift + 8)))
              atomicAdd(&s_hist[(key[u] >> shift) & 255], w[u]);
          __syncthreads();
          // thread tid owns bin 255 - tid: the inclusive scan over threads is the weight at or above the bin
          const unsigned long long v = s_hist[255 - tid];
          unsigned long long inc = v;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long n = __shfl_up(inc, o);
            if (lane >= o) inc += n;
          }
          if (lane == 63) s_wsum[wave] = inc;
          __syncthreads();
          for (int x = 0; x < wave; ++x) inc += s_wsum[x];
          if (inc - v < target && target <= inc) {       // exactly one bin crosses the target (1 <= target <= total)
            s_digit = 255 - tid;
            s_target = target - (inc - v);
          }
          __syncthreads();
          prefix |= static_cast<unsigned long long>(s_digit) << shift;
          target = s_target;
        }
      }
#pragma unroll
      for (int u = 0; u < kPer; ++u) keep[u] = w[u] != 0 && tot > 0 && key[u] >= prefix;
    }
    // the draw: the best of z + g over the kept set
    float bv = kMaskedLogit;
    int bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      if (!keep[u]) continue;
      const int i = tid + u * 256;
      const float v = z[u] + mt3s_gumbel(mt3s_bits(seed, stream, t, i));
      if (cand_better(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (cand_better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_v[wave] = bv;
      s_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int x = 1; x < 4; ++x)
        if (cand_better(s_v[x], s_i[x], bv, bi)) {
          bv = s_v[x];
          bi = s_i[x];
        }
      pick = bi;
    }
  }
  __syncthreads();              // every thread has read the slot's counters: thread 0 may write them
  if (tid == 0) {
    int tok;
    bool finished = false;
    if (ptok != 0) {
      tok = was_done ? 0 : ptok;                         // inside the prompt: the token is given
    } else {
      // a row with no candidate at all (every logit -inf or NaN: the host checks rule it out) ends: EOS
      tok = was_done ? 0 : (t + 1 >= eos_len || pick == 0x7fffffff ? 1 : pick);
      finished = !was_done && tok == 1;
    }
    if (!was_done && rt.max_len > 0 && t + 1 >= rt.max_len) finished = true;
    if (finished) {
      st.done[b] = 1;
      atomicAdd(st.n_done, 1);
    }
    a.ids[static_cast<size_t>(out_row) * a.ids_stride + t] = tok;
    if (a.gr.on && !was_done) st.gram[b] = mt3g_advance(&a.gr.g, gs, tok);
    if (NOTES && !was_done) note_commit(a.nt.n, st, b, gs, nv, tok, nullptr, false);
    st.cur_tok[b] = tok;
    st.step[b] = t + 1;
    s_tok = tok;
    s_t = t + 1;
  }
  __syncthreads();
  if (a.in.y) put_input_row(a.in, b, s_tok, s_t, tid, 256);
}

int launch_sample_step(const SampleStepArgs& sa, hipStream_t s) {
  const ArgmaxStepArgs& a = sa.a;
  if (!sa.params) return mt3::fail(MT3_ERR_INVALID, "sample_step: the sampling parameters are missing");
  if (a.beam.f || a.forced)
    return mt3::fail(MT3_ERR_INVALID, "sample_step: sampling is a greedy-path feature (no beam-1, no teacher forcing)");
  if (a.vocab < 2 || a.vocab > MT3_SAMPLING_MAX_VOCAB)
    return mt3::fail(MT3_ERR_INVALID, "sample_step: the vocabulary must be 2 .. 2048");
  if (a.ls.ss && (a.ls.n_ss <= 0 || a.ls.n_ss > 64 || a.ls.dim <= 0))
    return mt3::fail(MT3_ERR_INVALID, "sample_step: the row scale needs 1 .. 64 partial sums");
  if (const int rc = bad_input_row(a.in, "sample_step")) return rc;
  if (a.tm.rows && a.tm.stride != (a.vocab + 31) / 32)
    return mt3::fail(MT3_ERR_INVALID, "sample_step: token masks are ceil(vocab / 32) words");
  if (a.tp.rows && a.tp.stride < 1) return mt3::fail(MT3_ERR_INVALID, "sample_step: prompts have a stride of at least 1");
  if (a.gr.on && (!a.st.gram || bad_token_grammar(a.gr.g, a.vocab)))
    return mt3::fail(MT3_ERR_INVALID, "sample_step: the grammar needs the slots' states and valid ranges");
  if (a.nt.on && (!a.gr.on || !a.st.note || !a.st.nrow || !a.st.held || bad_note_grammar(a.nt.n, a.vocab) ||
                  a.st.held_words != mt3n_table_words(&a.nt.n) || std::memcmp(&a.nt.n.g, &a.gr.g, sizeof(a.gr.g)) != 0))
    return mt3::fail(MT3_ERR_INVALID, "sample_step: the note rule needs its grammar set as the step's grammar, the slots' "
                                      "note states and a valid descriptor");
  if (sa.stream.rows && sa.stream.stride != 1)
    return mt3::fail(MT3_ERR_INVALID, "sample_step: the stream table holds one entry per row");
  if (sa.seed.rows && sa.seed.stride != 1)
    return mt3::fail(MT3_ERR_INVALID, "sample_step: the seed table holds one entry per row");
  if (sa.seed.rows) {
    if (a.nt.on) hipLaunchKernelGGL((sample_step_kernel<true, true>), dim3(a.B), dim3(256), 0, s, sa);
    else hipLaunchKernelGGL((sample_step_kernel<false, true>), dim3(a.B), dim3(256), 0, s, sa);
  } else {
    if (a.nt.on) hipLaunchKernelGGL((sample_step_kernel<true, false>), dim3(a.B), dim3(256), 0, s, sa);
    else hipLaunchKernelGGL((sample_step_kernel<false, false>), dim3(a.B), dim3(256), 0, s, sa);
  }
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ---------------------------------------------------------------------------------------------- row retirement
// Compaction of a row group's live slots (CompactArgs, kernels.h).  Three launches on the group's stream, issued at a
// poll of the early-exit loop when the live rows fit a smaller number of 32-row GEMM tiles:
//   plan    one wave: perm[i] = i-th live slot (ascending: the order of the rows never changes), perm[rows] = n_live
//   gather  block i < n_live: state of slot perm[i] -> scratch slot i
//   scatter block i: scratch slot i -> slot i, done = 0 (i < n_live);  done = 1 (i >= n_live)
// (two passes because perm[i] >= i: slot k is the source of one block and the destination of another)
__global__ __launch_bounds__(64) void compact_plan_kernel(const int* __restrict__ done, int* __restrict__ perm, int rows) {
  const int lane = threadIdx.x;
  int n = 0;
  for (int base = 0; base < rows; base += 64) {
    const int i = base + lane;
    const bool live = i < rows && done[i] == 0;
    const unsigned long long m = __ballot(live);
    if (live) perm[n + __popcll(m & ((1ull << lane) - 1ull))] = i;
    n += __popcll(m);
  }
  if (lane == 0) perm[rows] = n;
}

template <bool GATHER>
__global__ __launch_bounds__(128) void compact_move_kernel(CompactArgs c) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int n_live = c.perm[c.rows];
  if (i >= n_live) {
    if (!GATHER && tid == 0) {
      c.st.done[i] = 1;
      if (c.st.slot_seg) c.st.slot_seg[i] = -1;
    }
    return;
  }
  const size_t src = GATHER ? static_cast<size_t>(c.perm[i]) : static_cast<size_t>(i), dst = i;
  const InputRow& r = c.in;
  const int emb = r.dim, q_n = r.rp.q_n;
  const float *y = GATHER ? r.y : c.s_y, *ss = GATHER ? r.y_ss : c.s_y_ss, *q = GATHER ? r.rp.q_out : c.s_qkvf;
  float *yo = GATHER ? c.s_y : r.y, *sso = GATHER ? c.s_y_ss : r.y_ss, *qo = GATHER ? c.s_qkvf : r.rp.q_out;
  const uint2* ct = static_cast<const uint2*>(GATHER ? r.y_ct : c.s_y_ct);
  uint2* cto = static_cast<uint2*>(GATHER ? c.s_y_ct : r.y_ct);
  for (int k = tid; k < emb / 4; k += 128) {
    reinterpret_cast<float4*>(yo + dst * emb)[k] = reinterpret_cast<const float4*>(y + src * emb)[k];
    if (ct) cto[dst * (emb / 4) + k] = ct[src * (emb / 4) + k];
  }
  if (ss)
    for (int k = tid; k < emb / 16; k += 128) sso[dst * (emb / 16) + k] = ss[src * (emb / 16) + k];
  if (q)
    for (int k = tid; k < q_n / 4; k += 128)
      reinterpret_cast<float4*>(qo + dst * q_n)[k] = reinterpret_cast<const float4*>(q + src * q_n)[k];
  if (c.st.note) {
    // the note table: staged like the rows above (gather into the scratch, scatter back), so that a slot that is the source
    // of one move and the destination of another is read in full before it is written
    const uint32_t* h = (GATHER ? c.st.held : c.s_held) + src * c.st.held_words;
    uint32_t* ho = (GATHER ? c.s_held : c.st.held) + dst * c.st.held_words;
    for (int k = tid; k < c.st.held_words; k += 128) ho[k] = h[k];
  }
  if (tid == 0) {
    if (GATHER) {
      c.s_int[kCompactInts * dst + 0] = c.st.slot_row[src];
      c.s_int[kCompactInts * dst + 1] = c.st.step[src];
      c.s_int[kCompactInts * dst + 2] = c.st.cur_tok[src];
      c.s_int[kCompactInts * dst + 3] = c.beam.len ? c.beam.len[src] : 0;
      c.s_int[kCompactInts * dst + 4] = c.st.gram ? c.st.gram[src] : 0;
      if (c.st.note) {
        c.s_int[kCompactInts * dst + 5] = c.st.note[src];
        for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x)
          c.s_int[kCompactInts * dst + 6 + x] = static_cast<int>(c.st.nrow[src * MT3_NOTE_ROW_WORDS + x]);
      }
      if (c.st.slot_seg) c.s_seg[dst] = c.st.slot_seg[src];
      if (c.beam.f) {
        c.s_beam[2 * dst + 0] = c.beam.f[src];
        c.s_beam[2 * dst + 1] = c.beam.f[c.beam.rows + src];
      }
    } else {
      c.st.slot_row[dst] = c.s_int[kCompactInts * dst + 0];
      c.st.step[dst] = c.s_int[kCompactInts * dst + 1];
      c.st.cur_tok[dst] = c.s_int[kCompactInts * dst + 2];
      if (c.beam.len) c.beam.len[dst] = c.s_int[kCompactInts * dst + 3];
      if (c.st.gram) c.st.gram[dst] = c.s_int[kCompactInts * dst + 4];
      if (c.st.note) {
        c.st.note[dst] = c.s_int[kCompactInts * dst + 5];
        for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x)
          c.st.nrow[dst * MT3_NOTE_ROW_WORDS + x] = static_cast<uint32_t>(c.s_int[kCompactInts * dst + 6 + x]);
      }
      if (c.st.slot_seg) c.st.slot_seg[dst] = c.s_seg[dst];
      if (c.beam.f) {
        c.beam.f[dst] = c.s_beam[2 * dst + 0];
        c.beam.f[c.beam.rows + dst] = c.s_beam[2 * dst + 1];
      }
      c.st.done[dst] = 0;
    }
  }
}

int launch_compact(const CompactArgs& c, hipStream_t s) {
  if (!c.st.done || !c.st.slot_row || !c.st.step || !c.st.cur_tok || !c.in.y || !c.s_y || !c.s_int || !c.perm || c.rows <= 0 ||
      c.in.dim % 16 || c.in.rp.q_n % 4 || (c.in.y_ct && !c.s_y_ct) || (c.in.y_ss && !c.s_y_ss) || (c.in.rp.q_out && !c.s_qkvf) ||
      (c.beam.f && (!c.s_beam || !c.beam.len)) || (c.st.slot_seg && !c.s_seg) ||
      (c.st.note && (!c.st.nrow || !c.st.held || !c.s_held || c.st.held_words <= 0)))
    return mt3::fail(MT3_ERR_INVALID, "compact: bad arguments");
  hipLaunchKernelGGL(compact_plan_kernel, dim3(1), dim3(64), 0, s, c.st.done, c.perm, c.rows);
  hipLaunchKernelGGL(compact_move_kernel<true>, dim3(c.rows), dim3(128), 0, s, c);
  hipLaunchKernelGGL(compact_move_kernel<false>, dim3(c.rows), dim3(128), 0, s, c);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ---------------------------------------------------------------------------------------------- slot refill
// In-flight batching (RefillArgs, kernels.h).  Three launches on the group's stream at a poll of the group's loop:
//   plan   one wave: plan[i] = i-th FINISHED slot of the group (ascending), plan[rows] = how many; the group's counter of
//          finished slots drops by the number that restart
//   cross  block (i, layer x {K, V [, scales]}, part): cross-attention K/V of segment first_seg + i from the staging chunk
//          into the cache rows of slot plan[i]  (16-byte pieces, 256 lanes, a row of H*T*64 elements in `parts` pieces)
//   slot   block i: id row of slot plan[i] -> the caller's row of the segment it decoded (beam-1: the finished
//          hypothesis, as beam1_finalize_kernel would leave it); i < n_new: restart on segment first_seg + i
// (unit > 1: plan and cross copy are over ELEMENTS of `unit` slots each -- beam groups, keyed on the element's first slot)
// (StagedCross::per > 1, mt3_engine_transcribe_draws: first_seg, src_entry0 and src_batch count DRAWS, `per` of which share
// one staged entry -- restarted slot i copies entry (src_entry0 + i) / per of a chunk whose planes are src_batch / per apart)
__global__ __launch_bounds__(64) void refill_plan_kernel(const int* __restrict__ done, int* __restrict__ plan,
                                                          int* __restrict__ n_done, int rows, int n_new, int unit) {
  const int lane = threadIdx.x;
  int n = 0;
  for (int base = 0; base < rows; base += 64) {
    const int i = base + lane;
    const bool fin = i < rows && done[i * unit] != 0;
    const unsigned long long m = __ballot(fin);
    if (fin) plan[n + __popcll(m & ((1ull << lane) - 1ull))] = i;
    n += __popcll(m);
  }
  if (lane == 0) {
    plan[rows] = n;
    *n_done -= (n_new < n ? n_new : n) * unit;
  }
}

// the slots of plan entry i are plan[i] * unit + j, j < unit: every 16-byte piece is loaded once and stored to each
__global__ __launch_bounds__(256) void refill_cross_kernel(StagedCross x, const int* __restrict__ plan,
                                                            const int* __restrict__ slot_row, int rows, int n_new,
                                                            int unit, int parts) {
  const int i = blockIdx.x;
  if (i >= n_new || i >= plan[rows]) return;
  const int s0 = plan[i] * unit;
  const int l = blockIdx.y / 3, what = blockIdx.y % 3;          // 0: K rows, 1: V rows, 2: scale rows (e4m3 caches)
  const char* src;
  char* dst;
  size_t bytes;
  if (what < 2) {
    bytes = x.row_bytes;
    src = x.src[l] + (static_cast<size_t>(what) * (x.src_batch / x.per) + (x.src_entry0 + i) / x.per) * bytes;
    dst = x.dst[l] + static_cast<size_t>(what) * x.dst_batch * bytes;
  } else {
    if (!x.src_sc[l]) return;
    bytes = x.sc_bytes;
    src = x.src_sc[l] + static_cast<size_t>((x.src_entry0 + i) / x.per) * bytes;
    dst = x.dst_sc[l];
  }
  u32x4* d4[kBeamMaxK];
#pragma unroll
  for (int j = 0; j < kBeamMaxK; ++j)       // (entries past `unit` repeat the first slot's row and are never stored to)
    d4[j] = reinterpret_cast<u32x4*>(dst + static_cast<size_t>(slot_row[s0 + (j < unit ? j : 0)]) * bytes);
  const size_t n16 = bytes >> 4;                                   // rows are multiples of 16 bytes (64 elements per key)
  const u32x4* s4 = reinterpret_cast<const u32x4*>(src);
  for (size_t p = static_cast<size_t>(blockIdx.z) * 256 + threadIdx.x; p < n16; p += static_cast<size_t>(parts) * 256) {
    const u32x4 v = __builtin_nontemporal_load(s4 + p);
#pragma unroll
    for (int j = 0; j < kBeamMaxK; ++j)
      if (j < unit) d4[j][p] = v;
  }
}

__global__ __launch_bounds__(128) void refill_slot_kernel(RefillArgs a) {
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= a.plan[a.rows]) return;
  const int slot = a.plan[i];
  const int row = a.st.slot_row[slot];
  const int seg_old = a.st.slot_seg[slot];
  int* idrow = a.ids + static_cast<size_t>(row) * a.ids_stride;
  if (seg_old >= 0) {
    // the finished hypothesis of the beam-1 search: live[:n] + EOS + padding (beam1_finalize_kernel); n < 0: the live one
    const int n = a.beam.len ? a.beam.len_row[row] : -1;
    int* out = a.out_ids + static_cast<size_t>(seg_old) * a.ids_stride;
    for (int k = tid; k < a.ids_stride; k += 128) out[k] = (n >= 0 && k >= n) ? (k == n ? 1 : 0) : idrow[k];
  }
  const bool restart = i < a.n_new;
  __syncthreads();                  // every lane has read the old occupant's beam length before lane 0 resets it
  // (a thread zeroes exactly the ids it has just copied out)
  if (restart)
    for (int k = tid; k < a.ids_stride; k += 128) idrow[k] = 0;
  if (tid == 0) {
    a.st.slot_seg[slot] = restart ? a.first_seg + i : -1;
    if (restart) {
      a.st.step[slot] = 0;
      a.st.cur_tok[slot] = 0;                                       // BOS
      a.st.done[slot] = 0;
      if (a.st.gram) a.st.gram[slot] = a.gram0;
      if (a.st.note) {
        a.st.note[slot] = 0;
        for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x) a.st.nrow[static_cast<size_t>(slot) * MT3_NOTE_ROW_WORDS + x] = 0u;
      }
      if (a.beam.f) {                                            // t5x beam_search: live log-prob 0, nothing finished
        a.beam.f[slot] = 0.f;
        a.beam.f[a.beam.rows + slot] = 0.f;
        a.beam.len[slot] = -1;
        a.beam.len_row[row] = -1;
      }
    }
  }
  if (!restart) return;
  if (a.st.note)                                                  // nothing sounds at position 0
    for (int k = tid; k < a.st.held_words; k += 128) a.st.held[static_cast<size_t>(slot) * a.st.held_words + k] = 0u;
  // decoder input of position 0: Embed(BOS) + FixedEmbed[0], in the forms the step reads (embed_kernel)
  put_input_row(a.in, slot, 0, 0, tid, 128);
}

static bool bad_staged_cross(const StagedCross& x, int n_new) {   // a copy of n_new staged segments that cannot be right
  return x.n_layers <= 0 || x.n_layers > kRefillMaxLayers || x.row_bytes % 16 || x.sc_bytes % 16 || x.src_batch <= 0 ||
         x.dst_batch <= 0 || x.src_entry0 < 0 || x.src_entry0 + n_new > x.src_batch || x.per < 1 || x.src_batch % x.per;
}

// the plan (refill_plan_kernel) and the copy of the first n_new staged segments of `x` into the slots it names
static int launch_refill_plan_cross(const SlotState& st, int* plan, int rows, int n_new, int unit, const StagedCross& x,
                                    int parts, const char* who, hipStream_t s) {
  if (n_new > 0 && bad_staged_cross(x, n_new)) return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": bad staging chunk");
  hipLaunchKernelGGL(refill_plan_kernel, dim3(1), dim3(64), 0, s, st.done, plan, st.n_done, rows, n_new, unit);
  if (n_new > 0)
    hipLaunchKernelGGL(refill_cross_kernel, dim3(n_new, x.n_layers * 3, parts), dim3(256), 0, s, x, plan, st.slot_row, rows,
                       n_new, unit, parts);
  return MT3_OK;
}

int launch_refill(const RefillArgs& a, hipStream_t s) {
  const SlotState& st = a.st;
  if (!st.done || !st.slot_row || !st.slot_seg || !st.step || !st.cur_tok || !st.n_done || !a.in.y || a.in.dim % 16 || !a.ids ||
      !a.out_ids || !a.plan || a.rows <= 0 || a.n_new < 0 || a.n_new > a.rows || a.ids_stride <= 0 ||
      (a.beam.f && (!a.beam.len || !a.beam.len_row)))
    return mt3::fail(MT3_ERR_INVALID, "refill: bad arguments");
  if (const int rc = bad_input_row(a.in, "refill")) return rc;
  // a K or V row of one layer is H*T*64 elements (98 KB ... 393 KB): 8 blocks of 256 lanes per row keep >= 1000
  // workgroups in flight for a handful of segments
  if (const int rc = launch_refill_plan_cross(st, a.plan, a.rows, a.n_new, 1, a.x, 8, "refill", s)) return rc;
  hipLaunchKernelGGL(refill_slot_kernel, dim3(a.rows), dim3(128), 0, s, a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ---------------------------------------------------------------------------------------------- k-beam search
// One step of t5x beam_search with k = num_decodes (the rule: include/mt3_hip.h, mt3_engine_decode_beams).  One block of
// k waves per batch element, wave w = the live beam in slot b*k + w.
//   1. each wave holds its logits row in registers and computes log-sum-exp in EXACTLY the order of
//      argmax_step_kernel<true> (four "virtual threads" per lane stand for that kernel's 256 threads), so that k = 1
//      reproduces MT3_DECODE_BEAM1 bit for bit;
//   2. each wave takes its own top 2k by logit (lower id on ties) and scores them live + logp;
//   3. wave 0 merges the k * 2k scored candidates in LDS (higher score first; on equal scores the lower flattened index
//      beam * V + token, taken in the order of step 2 inside a beam), then lane 0 updates the live and finished sets,
//      the history, the slot -> cache-row map (a beam takes over its parent's row; the extra children of a parent take
//      the rows of parents nobody chose and are marked for beam_reorder_kernel) and the retirement;
//   4. each wave writes its slot's next input row, as the greedy / beam-1 kernel does.
// MASKED = true: the logits of the tokens the element's mask (tm) disallows are -inf in steps 1 and 2 -- 0 in the
// log-sum-exp, never among the 2k; a mask in use allows at least 2k tokens (checked on the host).
// PROMPT = true: an element at a position inside its segment's prompt (tp) takes P[t] in all k slots: the k live
// log-probs, the finished set and the slot -> row map stay as they are (no candidate, no fork: fork_src = -1, every
// beam its own parent in the history), the retirement test is skipped, and each wave writes its slot's next input row
// from P[t].  The branch is element-uniform.  live stays [0, NEG_INF, ...], so the first free step expands beam 0 only,
// as step 0 does without a prompt, and the k cache rows hold the same K/V for the prompt's positions.
// GRAMMAR = true: each beam's logits are restricted to the ids the event grammar allows in ITS slot's state (st.gram,
// requested in the batch of the logits; where the mask is applied), and new slot j gets advance(state[parent_j], tok_j):
// every wave leaves its state in LDS before the barrier the merge waits at, so all k parent states are read before lane 0
// writes any.  Inside a prompt slot j advances its own state by P[t].  As in the token kernel the flag exists on the
// <MASKED, PROMPT> form only, with empty tables where there are no masks or prompts.
// NOTES = true (on top of GRAMMAR only; gr.g == nt.n.g): each beam's logits are further restricted by the note rule in ITS
// slot's note state, and new slot j gets advance(state[parent_j], tok_j), the table of sounding notes included.  Every wave
// leaves its `note` int and row copy in LDS with the grammar state; after the merge wave j reads its parent's table into
// registers (at most 512 words: 8 per lane) -- only where parent_j != j -- and the row of a new program from the parent's
// table, the block meets at a barrier, and only then are tables, row copies and note ints written: all k parents are read
// before any slot is written.  The pitch's bit is applied on the way of the copy.
template <bool MASKED, bool PROMPT, bool GRAMMAR = false, bool NOTES = false>
__global__ __launch_bounds__(64 * kBeamMaxK) void beam_step_kernel(BeamKArgs a, LogitScale ls, TokenMask tm, TokenPrompt tp,
                                                                    TokenGrammar gr, TokenNotes nt) {
  constexpr int kPerLane = 32;                         // vocab <= 2048: lane l holds i = l + 64 * vt + 256 * u
  __shared__ float c_score[2 * kBeamMaxK * kBeamMaxK];
  __shared__ int c_tok[2 * kBeamMaxK * kBeamMaxK];
  __shared__ int s_sel[2 * kBeamMaxK];
  __shared__ int s_tok[kBeamMaxK];
  __shared__ int s_gs[kBeamMaxK];                         // GRAMMAR: the state of each beam's slot before this step
  __shared__ int s_note[kBeamMaxK], s_par[kBeamMaxK];     // NOTES: each slot's note int before the step; each new slot's parent
  __shared__ uint32_t s_nrow[kBeamMaxK][MT3_NOTE_ROW_WORDS];   // NOTES: each slot's row copy before the step
  const int k = a.k, k2 = 2 * k, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s0 = blockIdx.x * k, slot = s0 + w;
  if (a.st.done[s0]) return;                              // retired element: its state is final
  const int t = a.st.step[s0];
  const float* row = a.logits + static_cast<size_t>(slot) * a.vocab;
  float xv[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int i = lane + 64 * (j >> 3) + 256 * (j & 7);
    xv[j] = row[i < a.vocab ? i : a.vocab - 1];
  }
  // MASKED: the mask word of every logit the lane holds, requested in the same batch as the logits
  uint32_t mw[kPerLane];
  if (MASKED) {
    const uint32_t* mrow = seg_table_row(tm, slot_segment(tm.slot_seg, s0, blockIdx.x));
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int i = lane + 64 * (j >> 3) + 256 * (j & 7);
      mw[j] = mrow ? mrow[(i < a.vocab ? i : a.vocab - 1) >> 5] : 0xffffffffu;
    }
  }
  int gs = 0;
  if (GRAMMAR) {                  // this beam's packed state: one dword per wave, requested in the same batch
    gs = a.st.gram[slot];
    if (lane == 0) s_gs[w] = gs;
  }
  NoteView nv{};
  if (NOTES) {
    nv = load_note_view(a.st, slot);
    if (lane == 0) {
      s_note[w] = nv.note;
#pragma unroll
      for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x) s_nrow[w][x] = nv.row[x];
    }
  }
  if (PROMPT) {
    // the element's prompt token at its own position, requested in the same batch as the logits (0: not inside a prompt)
    const int ptok = prompt_token(tp, slot_segment(tp.slot_seg, s0, blockIdx.x), t);
    if (ptok != 0) {
      __syncthreads();             // every wave has read the element's done flag and position before thread 0 rewrites them
      if (threadIdx.x == 0) {
        // in-flight batching: an element that has run max_len steps is closed (the row ran out of positions)
        const bool closed = a.max_len > 0 && t + 1 >= a.max_len;
        for (int j = 0; j < k; ++j) {
          a.fork_src[s0 + j] = -1;
          a.hist_par[static_cast<size_t>(t) * a.hist_stride + s0 + j] = j;
          a.hist_tok[static_cast<size_t>(t) * a.hist_stride + s0 + j] = ptok;
          a.st.cur_tok[s0 + j] = ptok;
          a.st.step[s0 + j] = t + 1;
          if (GRAMMAR) a.st.gram[s0 + j] = mt3g_advance(&gr.g, s_gs[j], ptok);
          if (closed) a.st.done[s0 + j] = 1;
        }
        if (closed) atomicAdd(a.st.n_done, k);
      }
      if (NOTES && lane == 0) note_commit(nt.n, a.st, slot, gs, nv, ptok, nullptr, false);   // its own slot: nothing forks
      if (a.in.y) put_input_row(a.in, slot, ptok, t + 1, lane, 64);
      return;
    }
  }
  const float live = a.live[slot];
  if (ls.ss) {                                         // folded logits projection (LogitScale)
    float p = lane < ls.n_ss ? ls.ss[static_cast<size_t>(slot) * ls.n_ss + lane] : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
    const float rs = rsqrtf(p / static_cast<float>(ls.dim) + 1e-6f);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) xv[j] *= rs;
  }
  if (MASKED) {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
      if (!mask_allows(mw[j], lane)) xv[j] = kMaskedLogit;     // (i & 31 == lane & 31: i = lane + a multiple of 64)
  }
  if (GRAMMAR) {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
      if (!mt3g_allowed(&gr.g, gs, lane + 64 * (j >> 3) + 256 * (j & 7))) xv[j] = kMaskedLogit;
  }
  if (NOTES) {
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
      if (!mt3n_allowed_extra(&nt.n, gs, nv.note, nv.row, lane + 64 * (j >> 3) + 256 * (j & 7))) xv[j] = kMaskedLogit;
  }
  // log-sum-exp of the row, in argmax_step_kernel<true>'s order: per thread, per wave, then over the four waves
  float vmax[4], vsum[4];
#pragma unroll
  for (int vt = 0; vt < 4; ++vt) {
    float m = -3.0e38f, acc = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (lane + 64 * vt + 256 * u < a.vocab && xv[vt * 8 + u] > m) m = xv[vt * 8 + u];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (lane + 64 * vt + 256 * u < a.vocab) acc += __expf(xv[vt * 8 + u] - m);
    float wm = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o));
    acc *= __expf(m - wm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    vmax[vt] = wm;
    vsum[vt] = acc;
  }
  float bm = vmax[0];
#pragma unroll
  for (int vt = 1; vt < 4; ++vt)
    if (vmax[vt] > bm) bm = vmax[vt];
  float sum = 0.f;
#pragma unroll
  for (int vt = 0; vt < 4; ++vt) sum += vsum[vt] * __expf(vmax[vt] - bm);
  const float lse = bm + __logf(sum);
  // this beam's top 2k by logit: 2k rounds of a wave arg-max over the values not yet taken
  unsigned taken = 0u;
  for (int r = 0; r < k2; ++r) {
    float bv = -3.0e38f;
    int bi = 0x7fffffff, bj = -1;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const int i = lane + 64 * (j >> 3) + 256 * (j & 7);
      if (i < a.vocab && !((taken >> j) & 1u) && cand_better(xv[j], i, bv, bi)) {
        bv = xv[j];
        bi = i;
        bj = j;
      }
    }
    float wv = bv;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o);
      const int oi = __shfl_xor(wi, o);
      if (cand_better(ov, oi, wv, wi)) {
        wv = ov;
        wi = oi;
      }
    }
    if (bj >= 0 && bi == wi) taken |= 1u << bj;       // the lane that owns the winner
    if (lane == 0) {
      c_score[w * k2 + r] = live + (wv - lse);
      c_tok[w * k2 + r] = wi;
    }
  }
  __syncthreads();
  if (w == 0) {
    // the 2k best of the k * 2k candidates; candidate index e = beam * 2k + rank orders ties as the flattened index does
    const int n = k * k2;
    unsigned sel = 0u;
    for (int r = 0; r < k2; ++r) {
      float bv = -3.0e38f;
      int be = 0x7fffffff;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int e = lane + 64 * h;
        if (e < n && !((sel >> h) & 1u) && cand_better(c_score[e], e, bv, be)) {
          bv = c_score[e];
          be = e;
        }
      }
      float wv = bv;
      int we = be;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(wv, o);
        const int oe = __shfl_xor(we, o);
        if (cand_better(ov, oe, wv, we)) {
          wv = ov;
          we = oe;
        }
      }
      if (be == we && be != 0x7fffffff) sel |= 1u << ((we - lane) >> 6);
      if (lane == 0) s_sel[r] = we;
    }
    if (lane == 0) {
      const float bp_t = a.bp[1 + t + 1], bp_max = a.bp[0];
      // the new live beams: the k best candidates that do not end in EOS (at most k of the 2k do)
      float nl_score[kBeamMaxK];
      int nl_par[kBeamMaxK];
      float nf_score[2 * kBeamMaxK];
      int nf_par[2 * kBeamMaxK];
      int nlive = 0;
      for (int r = 0; r < k2; ++r) {
        const int e = s_sel[r], tok = c_tok[e], par = e / k2;
        const float sc = c_score[e];
        if (tok == 1) {
          nf_score[r] = sc / bp_t;
          nf_par[r] = par;
        } else {
          nf_score[r] = kBeamNegInf;
          nf_par[r] = -1;
          if (nlive < k) {
            nl_score[nlive] = sc;
            nl_par[nlive] = par;
            s_tok[nlive] = tok;
            ++nlive;
          }
        }
      }
      // finished set: the k best of [old k entries | this step's 2k], the lower index on equal scores
      float of_score[kBeamMaxK];
      int of_step[kBeamMaxK], of_beam[kBeamMaxK];
      for (int j = 0; j < k; ++j) {
        of_score[j] = a.fin_score[s0 + j];
        of_step[j] = a.fin_step[s0 + j];
        of_beam[j] = a.fin_beam[s0 + j];
      }
      unsigned used = 0u;
      float kth = kBeamNegInf;
      int kth_step = -1;
      for (int q = 0; q < k; ++q) {
        int best = -1;
        float bs = 0.f;
        for (int x = 0; x < k + k2; ++x) {
          if ((used >> x) & 1u) continue;
          const float sc = x < k ? of_score[x] : nf_score[x - k];
          if (best < 0 || sc > bs) {
            best = x;
            bs = sc;
          }
        }
        used |= 1u << best;
        const int st = best < k ? of_step[best] : (nf_par[best - k] >= 0 ? t : -1);
        const int bb = best < k ? of_beam[best] : nf_par[best - k];
        a.fin_score[s0 + q] = bs;
        a.fin_step[s0 + q] = st;
        a.fin_beam[s0 + q] = st >= 0 ? bb : -1;
        kth = bs;
        kth_step = st;
      }
      // cache rows: the first child of a parent takes the parent's row, every further child a row nobody chose
      int orow[kBeamMaxK], nchild[kBeamMaxK];
      for (int j = 0; j < k; ++j) {
        orow[j] = a.st.slot_row[s0 + j];
        nchild[j] = 0;
      }
      for (int j = 0; j < k; ++j) ++nchild[nl_par[j]];
      int free_row[kBeamMaxK], nfree = 0, forks = 0;
      for (int j = 0; j < k; ++j)
        if (nchild[j] == 0) free_row[nfree++] = orow[j];
      unsigned claimed = 0u;
      int nfree_used = 0;
      int* par_out = a.hist_par + static_cast<size_t>(t) * a.hist_stride + s0;
      int* tok_out = a.hist_tok + static_cast<size_t>(t) * a.hist_stride + s0;
      const bool retired = kth_step >= 0 && kth > nl_score[0] / bp_max;
      // in-flight batching: an element that has run max_len steps is closed as well (the row ran out of positions)
      const bool closed = retired || (a.max_len > 0 && t + 1 >= a.max_len);
      for (int j = 0; j < k; ++j) {
        const int p = nl_par[j];
        int nrow, src = -1;
        if (!((claimed >> p) & 1u)) {
          claimed |= 1u << p;
          nrow = orow[p];
        } else {
          nrow = free_row[nfree_used++];
          src = orow[p];
          ++forks;
        }
        a.st.slot_row[s0 + j] = nrow;
        a.fork_src[s0 + j] = src;
        par_out[j] = p;
        tok_out[j] = s_tok[j];
        a.live[s0 + j] = nl_score[j];
        a.st.cur_tok[s0 + j] = s_tok[j];
        a.st.step[s0 + j] = t + 1;
        if (GRAMMAR) a.st.gram[s0 + j] = mt3g_advance(&gr.g, s_gs[p], s_tok[j]);
        if (NOTES) s_par[j] = p;
        if (closed) a.st.done[s0 + j] = 1;
      }
      if (forks && !closed) atomicAdd(a.fork_count, forks);    // a closed element's forks are never copied
      if (closed) atomicAdd(a.st.n_done, k);
    }
  }
  __syncthreads();
  if (NOTES) {
    const int p = s_par[w], tok = s_tok[w], pgs = s_gs[p], HW = a.st.held_words, W = mt3n_row_words(&nt.n);
    NoteView pv;
    pv.note = s_note[p];
#pragma unroll
    for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x) pv.row[x] = s_nrow[p][x];
    int pitch = 0;
    const int eff = mt3n_pitch_effect(&nt.n, pgs, pv.note, tok, &pitch);
    const int nn = mt3n_note_advance(&nt.n, pv.note, tok);
    const bool fork = p != w;                             // wave-uniform
    const uint32_t* ptab = a.st.held + static_cast<size_t>(s0 + p) * HW;
    constexpr int kTabPerLane = MT3_NOTE_MAX_PROGRAMS * MT3_NOTE_ROW_WORDS / 64;
    uint32_t tv[kTabPerLane];
    if (fork) {
#pragma unroll
      for (int x = 0; x < kTabPerLane; ++x) tv[x] = lane + 64 * x < HW ? ptab[lane + 64 * x] : 0u;
    }
    const bool new_prog = !eff && ((nn ^ pv.note) & static_cast<int>(MT3_NOTE_PROGRAM)) != 0;
    uint32_t nr[MT3_NOTE_ROW_WORDS] = {0u, 0u, 0u, 0u};
    if (new_prog && lane == 0) {
#pragma unroll
      for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x)
        if (x < W) nr[x] = ptab[(static_cast<uint32_t>(nn) & MT3_NOTE_PROGRAM) * W + x];
    }
    __syncthreads();                 // every parent's table and row are in registers: now the slots may be written
    if (fork) {
      const int target = eff ? static_cast<int>(static_cast<uint32_t>(pv.note) & MT3_NOTE_PROGRAM) * W + (pitch >> 5) : -1;
      const uint32_t bit = 1u << (pitch & 31);
      uint32_t* dtab = a.st.held + static_cast<size_t>(slot) * HW;
#pragma unroll
      for (int x = 0; x < kTabPerLane; ++x) {
        const int idx = lane + 64 * x;
        if (idx < HW) dtab[idx] = idx != target ? tv[x] : (eff == 1 ? (tv[x] | bit) : (tv[x] & ~bit));
      }
    }
    if (lane == 0) note_commit(nt.n, a.st, slot, pgs, pv, tok, new_prog ? nr : nullptr, fork);
  }
  // the next step's input row of this wave's slot: Embed(tok) + FixedEmbed[t+1]
  if (a.in.y) put_input_row(a.in, slot, s_tok[w], t + 1, lane, 64);
}

int launch_beam_step(const BeamKArgs& a, const LogitScale& ls, const TokenMask& tm, const TokenPrompt& tp,
                     const TokenGrammar& gr, const TokenNotes& nt, hipStream_t s) {
  if (a.k < 1 || a.k > kBeamMaxK || a.elems <= 0 || a.vocab < 2 * a.k || a.vocab > 2048)
    return mt3::fail(MT3_ERR_INVALID, "beam_step: k must be 1 .. 8 and 2k <= vocab <= 2048");
  if (!a.logits || !a.live || !a.fin_score || !a.fin_step || !a.fin_beam || !a.hist_par || !a.hist_tok || !a.st.slot_row ||
      !a.fork_src || !a.fork_count || !a.st.done || !a.st.n_done || !a.st.step || !a.st.cur_tok || !a.bp)
    return mt3::fail(MT3_ERR_INVALID, "beam_step: missing state");
  if (ls.ss && (ls.n_ss <= 0 || ls.n_ss > 64 || ls.dim <= 0))
    return mt3::fail(MT3_ERR_INVALID, "beam_step: the row scale needs 1 .. 64 partial sums");
  if (a.in.y && a.in.dim % 16) return mt3::fail(MT3_ERR_INVALID, "beam_step: the next input row needs dim % 16 == 0");
  if (const int rc = bad_input_row(a.in, "beam_step")) return rc;
  if (tm.rows && tm.stride != (a.vocab + 31) / 32)
    return mt3::fail(MT3_ERR_INVALID, "beam_step: token masks are ceil(vocab / 32) words");
  if (tp.rows && tp.stride < 1) return mt3::fail(MT3_ERR_INVALID, "beam_step: prompts have a stride of at least 1");
  if (gr.on && (!a.st.gram || bad_token_grammar(gr.g, a.vocab)))
    return mt3::fail(MT3_ERR_INVALID, "beam_step: the grammar needs the slots' states and valid ranges");
  if (nt.on && (!gr.on || !a.st.note || !a.st.nrow || !a.st.held || bad_note_grammar(nt.n, a.vocab) ||
                a.st.held_words != mt3n_table_words(&nt.n) || std::memcmp(&nt.n.g, &gr.g, sizeof(gr.g)) != 0))
    return mt3::fail(MT3_ERR_INVALID, "beam_step: the note rule needs its grammar set as the step's grammar, the slots' note "
                                      "states and a valid descriptor");
  void (*kernel)(BeamKArgs, LogitScale, TokenMask, TokenPrompt, TokenGrammar, TokenNotes);
  if (nt.on) kernel = beam_step_kernel<true, true, true, true>;
  else if (gr.on) kernel = beam_step_kernel<true, true, true>;
  else if (tp.rows) kernel = tm.rows ? beam_step_kernel<true, true> : beam_step_kernel<false, true>;
  else kernel = tm.rows ? beam_step_kernel<true, false> : beam_step_kernel<false, false>;
  hipLaunchKernelGGL(kernel, dim3(a.elems), dim3(64 * a.k), 0, s, a, ls, tm, tp, gr, nt);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// block (slot, layer * H + head): a slot that did not fork this step returns at once
__global__ __launch_bounds__(256) void beam_reorder_kernel(BeamReorderArgs a) {
  const int slot = blockIdx.x, l = blockIdx.y / a.H, h = blockIdx.y % a.H;
  const int src = a.fork_src[slot];
  if (src < 0 || a.done[slot]) return;
  const int dst = a.slot_row[slot], n = a.step[slot];     // positions [0, t] = [0, step)
  const size_t pos_bytes = static_cast<size_t>(64) * a.kv_esize;
  const size_t so = (static_cast<size_t>(src) * a.H + h) * a.cap, dof = (static_cast<size_t>(dst) * a.H + h) * a.cap;
  const size_t n16 = static_cast<size_t>(n) * pos_bytes / 16;
  const uint4* ks = reinterpret_cast<const uint4*>(a.k[l] + so * pos_bytes);
  const uint4* vs = reinterpret_cast<const uint4*>(a.v[l] + so * pos_bytes);
  uint4* kd = reinterpret_cast<uint4*>(a.k[l] + dof * pos_bytes);
  uint4* vd = reinterpret_cast<uint4*>(a.v[l] + dof * pos_bytes);
  for (size_t i = threadIdx.x; i < n16; i += 256) {
    const uint4 x = ks[i], y = vs[i];
    kd[i] = x;
    vd[i] = y;
  }
  if (a.scale[l])
    for (int i = threadIdx.x; i < n; i += 256) a.scale[l][dof + i] = a.scale[l][so + i];
}

int launch_beam_reorder(const BeamReorderArgs& a, hipStream_t s) {
  if (a.n_layers <= 0 || a.n_layers > kRefillMaxLayers || a.H <= 0 || a.cap <= 0 || a.slots <= 0 ||
      (a.kv_esize != 1 && a.kv_esize != 2 && a.kv_esize != 4) || !a.fork_src || !a.slot_row || !a.step || !a.done)
    return mt3::fail(MT3_ERR_INVALID, "beam_reorder: bad arguments");
  for (int l = 0; l < a.n_layers; ++l)
    if (!a.k[l] || !a.v[l]) return mt3::fail(MT3_ERR_INVALID, "beam_reorder: missing cache");
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(a.slots, a.n_layers * a.H), dim3(256), 0, s, a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

__global__ void beam_init_kernel(float* live, float* fin_score, int* fin_step, int* fin_beam, int slots, int k) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= slots) return;
  live[i] = i % k == 0 ? 0.f : kBeamNegInf;
  fin_score[i] = kBeamNegInf;
  fin_step[i] = -1;
  fin_beam[i] = -1;
}

int launch_beam_init(float* live, float* fin_score, int* fin_step, int* fin_beam, int slots, int k, hipStream_t s) {
  if (!live || !fin_score || !fin_step || !fin_beam || slots <= 0 || k < 1 || slots % k)
    return mt3::fail(MT3_ERR_INVALID, "beam_init: bad arguments");
  hipLaunchKernelGGL(beam_init_kernel, dim3((slots + 255) / 256), dim3(256), 0, s, live, fin_score, fin_step, fin_beam,
                     slots, k);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// block (element b, output decode i): decode i of the result is state entry k - 1 - i (the state is best first, the
// result in increasing order of score).  The history is walked back from the entry's last step by one thread.
__global__ __launch_bounds__(256) void beam_finalize_kernel(BeamKArgs a, int L, int num_steps, int* ids, int* all_ids,
                                                           float* scores) {
  const int b = blockIdx.x, i = blockIdx.y, k = a.k, s0 = b * k, e = k - 1 - i;
  int* out_all = all_ids ? all_ids + (static_cast<size_t>(b) * k + i) * L : nullptr;
  int* out_best = i == k - 1 ? ids + static_cast<size_t>(b) * L : nullptr;
  for (int u = threadIdx.x; u < L; u += 256) {
    if (out_all) out_all[u] = 0;
    if (out_best) out_best[u] = 0;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const bool any_finished = a.fin_step[s0] >= 0;
  float score;
  int u, j;
  if (any_finished) {
    score = a.fin_score[s0 + e];
    u = a.fin_step[s0 + e];
    j = a.fin_beam[s0 + e];
    if (u >= 0) {
      if (out_all) out_all[u] = 1;
      if (out_best) out_best[u] = 1;
    }
    --u;                                                // u = -2 for an unfilled entry: nothing to walk
  } else {
    score = a.live[s0 + e];
    u = num_steps - 1;
    j = e;
  }
  for (; u >= 0; --u) {
    const size_t x = static_cast<size_t>(u) * a.hist_stride + s0 + j;
    const int tok = a.hist_tok[x];
    j = a.hist_par[x];
    if (out_all) out_all[u] = tok;
    if (out_best) out_best[u] = tok;
  }
  if (scores) scores[static_cast<size_t>(b) * k + i] = score;
}

int launch_beam_finalize(const BeamKArgs& a, int L, int num_steps, int* ids, int* all_ids, float* scores, hipStream_t s) {
  if (!ids || a.k < 1 || a.k > kBeamMaxK || a.elems <= 0 || L <= 0 || num_steps <= 0 || num_steps > L)
    return mt3::fail(MT3_ERR_INVALID, "beam_finalize: bad arguments");
  hipLaunchKernelGGL(beam_finalize_kernel, dim3(a.elems, a.k), dim3(256), 0, s, a, L, num_steps, ids, all_ids, scores);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ------------------------------------------------------- refill of beam elements (BeamRefillArgs, kernels.h)
// dynamic LDS: the element's history columns [n_hist][k] (token | parent << 11: vocab <= 2048, k <= 8), then the k
// decodes [k][L], both as 16-bit values
__global__ __launch_bounds__(256) void beam_refill_elem_kernel(BeamRefillArgs a) {
  extern __shared__ unsigned short s_mem[];
  const int i = blockIdx.x, tid = threadIdx.x, k = a.b.k, L = a.L;
  if (i >= a.plan[a.b.elems]) return;
  const int s0 = a.plan[i] * k;
  const int seg_old = a.b.st.slot_seg[s0];
  if (seg_old >= 0) {
    unsigned short* s_hist = s_mem;
    unsigned short* s_out = s_mem + static_cast<size_t>(a.num_steps) * k;
    const int ran = a.b.st.step[s0];
    const int n_hist = ran < a.num_steps ? ran : a.num_steps;   // steps the element ran (its history rows)
    for (int x = tid; x < n_hist * k; x += 256) {
      const int u = x / k, j = x - u * k;
      const size_t h = static_cast<size_t>(u) * a.b.hist_stride + s0 + j;
      s_hist[x] = static_cast<unsigned short>(a.b.hist_tok[h] | (a.b.hist_par[h] << 11));
    }
    for (int x = tid; x < k * L; x += 256) s_out[x] = 0;
    __syncthreads();
    float score = 0.f;
    if (tid < k) {
      // decode tid of the result = state entry k - 1 - tid (beam_finalize_kernel)
      const int e = k - 1 - tid;
      unsigned short* out = s_out + static_cast<size_t>(tid) * L;
      int u, j;
      if (a.b.fin_step[s0] >= 0) {
        score = a.b.fin_score[s0 + e];
        u = a.b.fin_step[s0 + e];
        j = a.b.fin_beam[s0 + e];
        if (u >= 0 && u < L) out[u] = 1;
        --u;                                              // u = -2 for an unfilled entry: nothing to walk
      } else {
        score = a.b.live[s0 + e];                         // nothing finished: the live beams at the last step
        u = n_hist - 1;
        j = e;
      }
      if (u >= n_hist) u = n_hist - 1;
      for (; u >= 0; --u) {
        const unsigned short hv = s_hist[u * k + j];
        out[u] = hv & 0x7ff;
        j = hv >> 11;
      }
    }
    __syncthreads();
    int* o_best = a.out_ids + static_cast<size_t>(seg_old) * L;
    int* o_all = a.out_all ? a.out_all + static_cast<size_t>(seg_old) * k * L : nullptr;
    for (int x = tid; x < k * L; x += 256) {
      const int v = s_out[x];
      if (o_all) o_all[x] = v;
      if (x >= (k - 1) * L) o_best[x - (k - 1) * L] = v;
    }
    if (tid < k && a.out_scores) a.out_scores[static_cast<size_t>(seg_old) * k + tid] = score;
  }
  const bool restart = i < a.n_new;
  __syncthreads();                  // every wave has read the old segment before threads < k write the new one
  if (tid < k) {
    const int slot = s0 + tid;
    a.b.st.slot_seg[slot] = restart ? a.first_seg + i : -1;
    if (restart) {
      a.b.live[slot] = tid == 0 ? 0.f : kBeamNegInf;
      a.b.fin_score[slot] = kBeamNegInf;
      a.b.fin_step[slot] = -1;
      a.b.fin_beam[slot] = -1;
      a.b.fork_src[slot] = -1;
      a.b.st.step[slot] = 0;
      a.b.st.cur_tok[slot] = 0;                               // BOS
      a.b.st.done[slot] = 0;
      if (a.b.st.gram) a.b.st.gram[slot] = a.gram0;
      if (a.b.st.note) {
        a.b.st.note[slot] = 0;
        for (int x = 0; x < MT3_NOTE_ROW_WORDS; ++x) a.b.st.nrow[static_cast<size_t>(slot) * MT3_NOTE_ROW_WORDS + x] = 0u;
      }
    }
  }
  if (!restart) return;
  if (a.b.st.note)                                                // nothing sounds at position 0, in any of the k slots
    for (int x = tid; x < k * a.b.st.held_words; x += 256) a.b.st.held[static_cast<size_t>(s0) * a.b.st.held_words + x] = 0u;
  // decoder input of position 0 for all k slots: Embed(BOS) + FixedEmbed[0], in the forms the step reads (embed_kernel)
  for (int j = 0; j < k; ++j) put_input_row(a.b.in, s0 + j, 0, 0, tid, 256);
}

int launch_beam_refill(const BeamRefillArgs& a, hipStream_t s) {
  const BeamKArgs& b = a.b;
  const SlotState& st = b.st;
  if (b.k < 1 || b.k > kBeamMaxK || b.elems <= 0 || b.vocab > 2048 || !b.live || !b.fin_score || !b.fin_step || !b.fin_beam ||
      !b.hist_par || !b.hist_tok || !st.slot_row || !b.fork_src || !st.done || !st.n_done || !st.step || !st.cur_tok ||
      !st.slot_seg || !b.in.y || b.in.dim % 16 || !a.plan || !a.out_ids || a.L <= 0 || a.num_steps <= 0 || a.num_steps > a.L ||
      a.n_new < 0 || a.n_new > b.elems)
    return mt3::fail(MT3_ERR_INVALID, "beam_refill: bad arguments");
  if (const int rc = bad_input_row(b.in, "beam_refill")) return rc;
  const size_t lds = (static_cast<size_t>(a.num_steps) + a.L) * b.k * sizeof(unsigned short);
  if (lds > 65536) return mt3::fail(MT3_ERR_INVALID, "beam_refill: history and decodes of an element exceed 64 KB of LDS");
  // parts: twice the greedy refill's, a block stores every piece it loads k times
  if (const int rc = launch_refill_plan_cross(st, a.plan, b.elems, a.n_new, b.k, a.x, 16, "beam_refill", s)) return rc;
  hipLaunchKernelGGL(beam_refill_elem_kernel, dim3(b.elems), dim3(256), lds, s, a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

__global__ void beam_stream_init_kernel(int* done, int* slot_seg, int* fork_src, int* slot_row, int* n_done, int slots,
                                        int groups, GroupSlots gs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < groups) n_done[i] = gs.n[i];
  if (i >= slots) return;
  done[i] = 1;
  slot_seg[i] = -1;
  fork_src[i] = -1;
  slot_row[i] = i;
}

int launch_beam_stream_init(int* done, int* slot_seg, int* fork_src, int* slot_row, int* n_done, int slots, int groups,
                            const GroupSlots& group_slots, hipStream_t s) {
  if (!done || !slot_seg || !fork_src || !slot_row || !n_done || slots <= 0 || groups < 1 || groups > 4)
    return mt3::fail(MT3_ERR_INVALID, "beam_stream_init: bad arguments");
  hipLaunchKernelGGL(beam_stream_init_kernel, dim3((slots + 255) / 256), dim3(256), 0, s, done, slot_seg, fork_src,
                     slot_row, n_done, slots, groups, group_slots);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

__global__ void iota_kernel(int* dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = i;
}
int launch_iota(int* dst, int n, hipStream_t s) {
  hipLaunchKernelGGL(iota_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, n);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// one float into device memory from a kernel ARGUMENT (no host buffer has to outlive the call)
__global__ void set_float_kernel(float* dst, float v) { *dst = v; }
int launch_set_float(float* dst, float v, hipStream_t s) {
  hipLaunchKernelGGL(set_float_kernel, dim3(1), dim3(1), 0, s, dst, v);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// end of a beam-1 decode: rows with a finished hypothesis return live[:len] + EOS (+ pad), the others
// keep their live sequence (t5x beam_search: "if no finished sequence, return the live one")
__global__ __launch_bounds__(256) void beam1_finalize_kernel(int* __restrict__ ids, int L,
                                                              const int* __restrict__ beam_len) {
  const int b = blockIdx.x, n = beam_len[b];
  if (n < 0) return;
  int* row = ids + static_cast<size_t>(b) * L;
  for (int i = n + threadIdx.x; i < L; i += 256) row[i] = i == n ? 1 : 0;
}

int launch_beam1_finalize(int* ids, int L, const int* beam_len, int B, hipStream_t s) {
  hipLaunchKernelGGL(beam1_finalize_kernel, dim3(B), dim3(256), 0, s, ids, L, beam_len);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

__global__ __launch_bounds__(256) void ids_to_tokens_kernel(const int* __restrict__ ids, int L, int num_regular,
                                                             int* __restrict__ out) {
  __shared__ int s_first[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* row = ids + static_cast<size_t>(b) * L;
  int first = L;                                      // index of the first EOS (id == 1)
  for (int i = tid; i < L; i += 256)
    if (row[i] == 1) {
      first = i;
      break;                                          // ascending i per thread
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
  if (lane == 0) s_first[wave] = first;
  __syncthreads();
  first = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
  for (int i = tid; i < L; i += 256) {
    const int id = row[i];
    int t;
    if (i >= first) t = -1;                           // DECODED_EOS_ID from the first EOS onward
    else if (id >= 3 && id < 3 + num_regular) t = id - 3;
    else t = -2;                                      // DECODED_INVALID_ID
    out[static_cast<size_t>(b) * L + i] = t;
  }
}

int launch_ids_to_tokens(const int* ids, int B, int L, int num_regular, int* out, hipStream_t s) {
  if (!ids || !out || B <= 0 || L <= 0) return mt3::fail(MT3_ERR_INVALID, "ids_to_tokens: bad arguments");
  hipLaunchKernelGGL(ids_to_tokens_kernel, dim3(B), dim3(256), 0, s, ids, L, num_regular, out);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

}  // namespace mt3k

extern "C" int mt3_op_residual_split(int32_t dtype, const float* d_x, void* d_x_ct, float* d_x_ss, int32_t rows,
                                     int32_t dim, void* stream) {
  if (dtype != MT3_BF16) return mt3::fail(MT3_ERR_INVALID, "residual_split: the split stream is a bf16-path format");
  return mt3k::launch_residual_split(d_x, d_x_ct, d_x_ss, rows, dim, static_cast<hipStream_t>(stream));
}

// include/mt3_hip.h: the kernel alone (the engine launches it once per encode, for encoder_norm)
extern "C" int mt3_op_rmsnorm(int32_t dtype, const float* d_x, const float* d_scale, void* d_out_ct, float* d_out_f32,
                              int32_t rows, int32_t dim, void* stream) {
  if (dtype != MT3_BF16 && dtype != MT3_F32) return mt3::fail(MT3_ERR_INVALID, "mt3_op_rmsnorm: dtype is MT3_BF16 or MT3_F32");
  if (dim <= 0) return mt3::fail(MT3_ERR_INVALID, "mt3_op_rmsnorm: dim < 4");
  return mt3::fail_as("mt3_op_rmsnorm", mt3k::launch_rmsnorm(dtype, d_x, d_scale, d_out_ct, d_out_f32, rows, dim,
                                                             static_cast<hipStream_t>(stream)));
}

extern "C" int mt3_ids_to_tokens(const int32_t* d_ids, int32_t batch, int32_t length, int32_t num_regular,
                                 int32_t* d_tokens, void* stream) {
  return mt3k::launch_ids_to_tokens(d_ids, batch, length, num_regular, d_tokens, static_cast<hipStream_t>(stream));
}

// ------------------------------------------------------------------ scripted drivers of the token-rule kernels
// mt3_op_beam_search_scripted / mt3_op_token_steps_scripted / mt3_op_beam_reorder (mt3_hip.h): the launchers above on
// logits the caller wrote, with state these calls own.  Test drivers: synchronous, one allocation for the whole state.
namespace {

#define MT3_OP_TRY(expr)            \
  do {                              \
    const int _rc = (expr);         \
    if (_rc != MT3_OK) return _rc;  \
  } while (0)

// one zero-filled (or `fill`-filled) device allocation carved into 256-byte aligned pieces; freed when the call returns
struct Scratch {
  char* base = nullptr;
  size_t size = 0, used = 0;
  ~Scratch() {
    if (base) (void)hipFree(base);
  }
  static size_t piece(size_t bytes) { return (bytes + 255) / 256 * 256; }
  int alloc(size_t bytes, hipStream_t s, int fill = 0) {
    MT3_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&base), bytes));
    size = bytes;
    MT3_HIP_CHECK(hipMemsetAsync(base, fill, bytes, s));
    return MT3_OK;
  }
  template <typename T>
  T* take(size_t n) {
    T* p = reinterpret_cast<T*>(base + used);
    used += piece(n * sizeof(T));
    return p;
  }
};

// the brevity-penalty table of a search over `num_steps` positions, as the engine uploads and bounds it
int upload_brevity(float* d_bp, int num_steps, hipStream_t s) {
  const std::vector<float> bp = mt3k::brevity_table(num_steps);
  MT3_HIP_CHECK(hipMemcpyAsync(d_bp, bp.data(), bp.size() * 4, hipMemcpyHostToDevice, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));                    // `bp` leaves scope
  return mt3k::launch_set_float(d_bp, mt3k::brevity_penalty(num_steps + 1), s);
}

bool bad_scale(const float* d_ss, int n_ss, int dim) { return d_ss && (n_ss < 1 || n_ss > 64 || dim <= 0); }

// the per-row index of a driver's table, d_index [n], read back into *h and checked on the host before a kernel indexes
// with it: every entry in [-1, bound), or the failure `bad`
int driver_index(const std::string& who, const int32_t* d_index, int n, int bound, const char* bad, std::vector<int32_t>* h) {
  h->resize(static_cast<size_t>(n));
  MT3_HIP_CHECK(hipMemcpy(h->data(), d_index, h->size() * 4, hipMemcpyDeviceToHost));
  for (int32_t v : *h)
    if (v < -1 || v >= bound) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  return MT3_OK;
}

// the masks of a masked driver, read back and checked on the host before a kernel indexes with them: every mask valid
// (bad_token_mask) with at least `need` allowed tokens, every entry of d_row_mask [n] in [-1, n_masks)
int driver_masks(const std::string& who, const uint32_t* d_masks, int n_masks, const int32_t* d_row_mask, int n, int vocab,
                 int need, mt3k::TokenMask* tm) {
  if (!d_masks || n_masks < 1 || n_masks > 4096) return mt3::fail(MT3_ERR_INVALID, who + ": 1 .. 4096 masks");
  const int words = (vocab + 31) / 32;
  std::vector<uint32_t> h(static_cast<size_t>(n_masks) * words);
  MT3_HIP_CHECK(hipMemcpy(h.data(), d_masks, h.size() * 4, hipMemcpyDeviceToHost));
  for (int m = 0; m < n_masks; ++m) {
    int allowed = 0;
    if (const char* bad = mt3k::bad_token_mask(h.data() + static_cast<size_t>(m) * words, vocab, &allowed))
      return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
    if (allowed < need) return mt3::fail(MT3_ERR_INVALID, who + ": a mask allows fewer than 2 * k tokens");
  }
  std::vector<int32_t> r;
  if (d_row_mask) MT3_OP_TRY(driver_index(who, d_row_mask, n, n_masks, "mask index outside [-1, n_masks)", &r));
  *tm = mt3k::TokenMask{d_masks, d_row_mask, nullptr, words};
  return MT3_OK;
}

// the prompts of a prompted driver, read back and checked on the host before a kernel indexes with them: every entry of
// d_row_prompt [n] at least -1 (the prompts it names are rows 0 .. its largest entry; nullptr: prompt 0 for every row),
// every prompt valid (bad_prompt)
int driver_prompts(const std::string& who, const int32_t* d_prompts, int stride, const int32_t* d_row_prompt, int n,
                   int vocab, mt3k::TokenPrompt* tp) {
  if (stride < 1 || stride > 4096) return mt3::fail(MT3_ERR_INVALID, who + ": the prompt stride must be 1 .. 4096");
  int n_prompts = 1;
  if (d_row_prompt) {
    std::vector<int32_t> r;
    MT3_OP_TRY(driver_index(who, d_row_prompt, n, 4096, "prompt index outside [-1, 4096)", &r));
    n_prompts = 0;
    for (int32_t v : r) n_prompts = std::max(n_prompts, v + 1);
  }
  std::vector<int32_t> h(static_cast<size_t>(n_prompts) * stride);
  if (!h.empty()) MT3_HIP_CHECK(hipMemcpy(h.data(), d_prompts, h.size() * 4, hipMemcpyDeviceToHost));
  for (int p = 0; p < n_prompts; ++p) {
    int len = 0;
    if (const char* bad = mt3k::bad_prompt(h.data() + static_cast<size_t>(p) * stride, stride, vocab, &len))
      return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  }
  *tp = mt3k::TokenPrompt{d_prompts, d_row_prompt, nullptr, stride};
  return MT3_OK;
}

// the grammar of a grammar driver, checked on the host as mt3_engine_set_token_grammar and the decode calls check it: a
// valid descriptor, and under every mask (d_masks == nullptr: none) at least `need` ids in the two bounding states
int driver_grammar(const std::string& who, const mt3_token_grammar* h_grammar, const uint32_t* d_masks, int n_masks,
                   int vocab, int need, mt3k::TokenGrammar* gr) {
  if (const char* bad = mt3k::bad_token_grammar(*h_grammar, vocab)) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  const int words = (vocab + 31) / 32;
  std::vector<uint32_t> h(d_masks ? static_cast<size_t>(n_masks) * words : 0);
  if (!h.empty()) MT3_HIP_CHECK(hipMemcpy(h.data(), d_masks, h.size() * 4, hipMemcpyDeviceToHost));
  for (int m = 0; m < (d_masks ? n_masks : 1); ++m) {
    int in_tie = 0, after = 0;
    mt3k::grammar_room(*h_grammar, d_masks ? h.data() + static_cast<size_t>(m) * words : nullptr, vocab, &in_tie, &after);
    if ((h_grammar->with_ties && in_tie < need) || after < need)
      return mt3::fail(MT3_ERR_INVALID, who + ": the grammar (with a mask) leaves fewer than 2 * k ids in a state");
  }
  gr->g = *h_grammar;
  gr->on = 1;
  return MT3_OK;
}

// the note rule of a notes driver: the descriptor checked as mt3_engine_set_note_grammar checks it, the room it leaves under
// every mask (with driver_grammar's own check of n.g), and the slots' note states in device memory of their own, all zero:
// program 0, velocity non-zero, nothing held
int driver_notes(const std::string& who, const mt3_note_grammar* h_notes, const uint32_t* d_masks, int n_masks, int vocab,
                 int need, size_t slots, hipStream_t s, Scratch* mem, mt3k::TokenNotes* nt, mt3k::SlotState* st) {
  if (const char* bad = mt3k::bad_note_grammar(*h_notes, vocab)) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  const int words = (vocab + 31) / 32;
  std::vector<uint32_t> h(d_masks ? static_cast<size_t>(n_masks) * words : 0);
  if (!h.empty()) MT3_HIP_CHECK(hipMemcpy(h.data(), d_masks, h.size() * 4, hipMemcpyDeviceToHost));
  for (int m = 0; m < (d_masks ? n_masks : 1); ++m)
    if (mt3k::note_room_after(*h_notes, d_masks ? h.data() + static_cast<size_t>(m) * words : nullptr, vocab) < need)
      return mt3::fail(MT3_ERR_INVALID, who + ": the note rule (with a mask) leaves fewer than 2 * k ids after a note-off "
                                              "marker with nothing held");
  const size_t hw = static_cast<size_t>(mt3n_table_words(h_notes));
  MT3_OP_TRY(mem->alloc(Scratch::piece(slots * 4) + Scratch::piece(slots * MT3_NOTE_ROW_WORDS * 4) +
                            Scratch::piece(slots * hw * 4),
                        s));
  st->note = mem->take<int>(slots);
  st->nrow = mem->take<uint32_t>(slots * MT3_NOTE_ROW_WORDS);
  st->held = mem->take<uint32_t>(slots * hw);
  st->held_words = static_cast<int>(hw);
  nt->n = *h_notes;
  nt->on = 1;
  return MT3_OK;
}
// the slots' note states after a step, into the caller's host arrays (either may be nullptr)
int driver_notes_out(const mt3k::SlotState& st, size_t slots, int t, int32_t* h_note, uint32_t* h_held, hipStream_t s) {
  const size_t hw = static_cast<size_t>(st.held_words);
  if (h_note) MT3_HIP_CHECK(hipMemcpyAsync(h_note + static_cast<size_t>(t) * slots, st.note, slots * 4, hipMemcpyDeviceToHost, s));
  if (h_held)
    MT3_HIP_CHECK(hipMemcpyAsync(h_held + static_cast<size_t>(t) * slots * hw, st.held, slots * hw * 4, hipMemcpyDeviceToHost, s));
  return MT3_OK;
}

}  // namespace

// shared body of mt3_op_beam_search_scripted (masked == false), mt3_op_beam_search_masked, mt3_op_beam_search_prompted and
// mt3_op_beam_search_grammar
static int beam_search_driver(const std::string& who, bool masked, const float* d_logits, const float* d_ss, int32_t n_ss,
                              int32_t dim, int32_t elems, int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len,
                              const float* d_table, const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids,
                              float* d_scores, float* d_y_next, int32_t* h_trace, float* h_live, int32_t* h_forks,
                              int32_t* h_steps_run, void* stream, const uint32_t* d_masks, int32_t n_masks,
                              const int32_t* d_row_mask, const int32_t* d_prompts = nullptr, int32_t stride = 0,
                              const int32_t* d_row_prompt = nullptr, const mt3_token_grammar* h_grammar = nullptr,
                              int32_t* h_state = nullptr, const mt3_note_grammar* h_notes = nullptr,
                              int32_t* h_note = nullptr, uint32_t* h_held = nullptr) {
  if (h_notes) h_grammar = &h_notes->g;             // the note rule's grammar is the grammar
  if (!d_logits || !d_ids || !d_all_ids || !d_scores || !h_trace || !h_live || !h_forks || !h_steps_run)
    return mt3::fail(MT3_ERR_INVALID, who + ": null argument");
  if (k < 1 || k > mt3k::kBeamMaxK || vocab < 2 * k || vocab > 2048)
    return mt3::fail(MT3_ERR_INVALID, who + ": k must be 1 .. 8 and 2k <= vocab <= 2048");
  if (elems <= 0 || elems > 4096 || num_steps <= 0 || num_steps > 4096 || max_len < 0 || bad_scale(d_ss, n_ss, dim))
    return mt3::fail(MT3_ERR_INVALID, who + ": elems / num_steps / max_len / row scale out of range");
  if ((d_table != nullptr) != (d_pos != nullptr) || (d_table != nullptr) != (d_y_next != nullptr) ||
      (d_table && (dim_e <= 0 || dim_e % 16)))
    return mt3::fail(MT3_ERR_INVALID, who + ": the tables and the next-row output come together, dim_e % 16 == 0");
  if (h_grammar)                                  // the descriptor itself: before anything is read back from the device
    if (const char* bad = mt3k::bad_token_grammar(*h_grammar, vocab)) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  if (h_notes)
    if (const char* bad = mt3k::bad_note_grammar(*h_notes, vocab)) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  mt3k::TokenMask tm{};
  if (masked) MT3_OP_TRY(driver_masks(who, d_masks, n_masks, d_row_mask, elems, vocab, 2 * k, &tm));
  mt3k::TokenPrompt tp{};
  if (d_prompts) MT3_OP_TRY(driver_prompts(who, d_prompts, stride, d_row_prompt, elems, vocab, &tp));
  mt3k::TokenGrammar gr{};
  if (h_grammar) MT3_OP_TRY(driver_grammar(who, h_grammar, masked ? d_masks : nullptr, n_masks, vocab, 2 * k, &gr));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int slots = elems * k;
  const size_t n = static_cast<size_t>(slots), hist = static_cast<size_t>(num_steps) * n;
  Scratch m;
  MT3_OP_TRY(m.alloc(10 * Scratch::piece(n * 4) + 2 * Scratch::piece(hist * 4) + 2 * Scratch::piece(4) +
                         Scratch::piece((static_cast<size_t>(num_steps) + 3) * 4),
                     s));
  mt3k::BeamKArgs b{};
  b.vocab = vocab;
  b.k = k;
  b.elems = elems;
  b.live = m.take<float>(n);
  b.fin_score = m.take<float>(n);
  b.fin_step = m.take<int>(n);
  b.fin_beam = m.take<int>(n);
  b.hist_par = m.take<int>(hist);
  b.hist_tok = m.take<int>(hist);
  b.hist_stride = slots;
  b.st.slot_row = m.take<int>(n);
  b.fork_src = m.take<int>(n);
  b.st.done = m.take<int>(n);
  b.st.step = m.take<int>(n);
  b.st.cur_tok = m.take<int>(n);
  if (gr.on) b.st.gram = m.take<int>(n);
  b.fork_count = m.take<int>(1);
  b.st.n_done = m.take<int>(1);
  float* d_bp = m.take<float>(static_cast<size_t>(num_steps) + 3);
  b.bp = d_bp;
  b.in.table = d_table;
  b.in.pos = d_pos;
  b.in.max_pos = num_steps + 1;
  b.in.y = d_y_next;
  b.in.dim = dim_e;
  b.max_len = max_len;
  Scratch nm;
  mt3k::TokenNotes nt{};
  if (h_notes) MT3_OP_TRY(driver_notes(who, h_notes, masked ? d_masks : nullptr, n_masks, vocab, 2 * k, n, s, &nm, &nt, &b.st));
  MT3_HIP_CHECK(hipMemsetAsync(b.fork_src, 0xFF, n * 4, s));               // -1: no fork pending
  if (gr.on) MT3_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b.st.gram), mt3g_initial(&gr.g), n, s));
  MT3_OP_TRY(mt3k::launch_iota(b.st.slot_row, slots, s));
  MT3_OP_TRY(mt3k::launch_beam_init(b.live, b.fin_score, b.fin_step, b.fin_beam, slots, k, s));
  MT3_OP_TRY(upload_brevity(d_bp, num_steps, s));
  int ran = 0;
  for (int t = 0; t < num_steps; ++t) {
    b.logits = const_cast<float*>(d_logits) + static_cast<size_t>(t) * n * vocab;
    const mt3k::LogitScale ls{d_ss ? d_ss + static_cast<size_t>(t) * n * n_ss : nullptr, n_ss, dim};
    MT3_OP_TRY(mt3k::launch_beam_step(b, ls, tm, tp, gr, nt, s));
    if (nt.on) MT3_OP_TRY(driver_notes_out(b.st, n, t, h_note, h_held, s));
    if (gr.on && h_state)
      MT3_HIP_CHECK(hipMemcpyAsync(h_state + static_cast<size_t>(t) * n, b.st.gram, n * 4, hipMemcpyDeviceToHost, s));
    int32_t* tr = h_trace + static_cast<size_t>(t) * 4 * n;
    MT3_HIP_CHECK(hipMemcpyAsync(tr, b.st.slot_row, n * 4, hipMemcpyDeviceToHost, s));
    MT3_HIP_CHECK(hipMemcpyAsync(tr + n, b.fork_src, n * 4, hipMemcpyDeviceToHost, s));
    MT3_HIP_CHECK(hipMemcpyAsync(tr + 2 * n, b.st.done, n * 4, hipMemcpyDeviceToHost, s));
    MT3_HIP_CHECK(hipMemcpyAsync(tr + 3 * n, b.st.cur_tok, n * 4, hipMemcpyDeviceToHost, s));
    MT3_HIP_CHECK(hipMemcpyAsync(h_live + static_cast<size_t>(t) * n, b.live, n * 4, hipMemcpyDeviceToHost, s));
    MT3_HIP_CHECK(hipStreamSynchronize(s));
    ran = t + 1;
    bool all_done = true;
    for (size_t i = 0; i < n; ++i) all_done = all_done && tr[2 * n + i] != 0;
    if (all_done) break;                                   // every element retired or closed: the search is over
  }
  // an element that max_len closed has max_len steps of history: that is where its live beams are walked back from
  const int walk = max_len > 0 && max_len < num_steps ? max_len : num_steps;
  MT3_OP_TRY(mt3k::launch_beam_finalize(b, num_steps, walk, d_ids, d_all_ids, d_scores, s));
  MT3_HIP_CHECK(hipMemcpyAsync(h_forks, b.fork_count, 4, hipMemcpyDeviceToHost, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));
  *h_steps_run = ran;
  return MT3_OK;
}

extern "C" int mt3_op_beam_search_scripted(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim,
                                           int32_t elems, int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len,
                                           const float* d_table, const float* d_pos, int32_t dim_e, int32_t* d_ids,
                                           int32_t* d_all_ids, float* d_scores, float* d_y_next, int32_t* h_trace,
                                           float* h_live, int32_t* h_forks, int32_t* h_steps_run, void* stream) {
  return beam_search_driver("mt3_op_beam_search_scripted", false, d_logits, d_ss, n_ss, dim, elems, k, vocab, num_steps,
                            max_len, d_table, d_pos, dim_e, d_ids, d_all_ids, d_scores, d_y_next, h_trace, h_live, h_forks,
                            h_steps_run, stream, nullptr, 0, nullptr);
}

extern "C" int mt3_op_beam_search_masked(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t elems,
                                         int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len, const float* d_table,
                                         const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids,
                                         float* d_scores, float* d_y_next, int32_t* h_trace, float* h_live,
                                         int32_t* h_forks, int32_t* h_steps_run, void* stream, const uint32_t* d_masks,
                                         int32_t n_masks, const int32_t* d_row_mask) {
  return beam_search_driver("mt3_op_beam_search_masked", true, d_logits, d_ss, n_ss, dim, elems, k, vocab, num_steps,
                            max_len, d_table, d_pos, dim_e, d_ids, d_all_ids, d_scores, d_y_next, h_trace, h_live, h_forks,
                            h_steps_run, stream, d_masks, n_masks, d_row_mask);
}

extern "C" int mt3_op_beam_search_prompted(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim,
                                           int32_t elems, int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len,
                                           const float* d_table, const float* d_pos, int32_t dim_e, int32_t* d_ids,
                                           int32_t* d_all_ids, float* d_scores, float* d_y_next, int32_t* h_trace,
                                           float* h_live, int32_t* h_forks, int32_t* h_steps_run, void* stream,
                                           const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                                           const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt) {
  return beam_search_driver("mt3_op_beam_search_prompted", d_masks != nullptr, d_logits, d_ss, n_ss, dim, elems, k, vocab,
                            num_steps, max_len, d_table, d_pos, dim_e, d_ids, d_all_ids, d_scores, d_y_next, h_trace, h_live,
                            h_forks, h_steps_run, stream, d_masks, n_masks, d_row_mask, d_prompts, stride, d_row_prompt);
}

// shared body of mt3_op_token_steps_scripted (masked == false), mt3_op_token_steps_masked, mt3_op_token_steps_prompted,
// mt3_op_token_steps_grammar and mt3_op_token_steps_sampled (h_sampling == nullptr: every statement the others run, no other)
static int token_steps_driver(const std::string& who, bool masked, float* d_logits, const float* d_ss, int32_t n_ss,
                              int32_t dim, int32_t rows, int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len,
                              int32_t* d_ids, int32_t* h_done, void* stream, const uint32_t* d_masks, int32_t n_masks,
                              const int32_t* d_row_mask, const int32_t* d_prompts = nullptr, int32_t stride = 0,
                              const int32_t* d_row_prompt = nullptr, const mt3_token_grammar* h_grammar = nullptr,
                              int32_t* h_state = nullptr, const mt3_sampling* h_sampling = nullptr,
                              const uint64_t* h_row_stream = nullptr, const mt3_note_grammar* h_notes = nullptr,
                              int32_t* h_note = nullptr, uint32_t* h_held = nullptr,
                              const uint64_t* h_row_seed = nullptr) {
  if (h_notes) h_grammar = &h_notes->g;             // the note rule's grammar is the grammar
  if (!d_logits || !d_ids || !h_done) return mt3::fail(MT3_ERR_INVALID, who + ": null argument");
  if ((mode != 0 && mode != 1) || rows <= 0 || rows > 4096 || vocab < 2 || num_steps <= 0 || num_steps > 4096 ||
      max_len < 0 || bad_scale(d_ss, n_ss, dim))
    return mt3::fail(MT3_ERR_INVALID, who + ": mode is 0 (greedy) or 1 (beam-1); rows, vocab >= 2, num_steps, max_len or "
                                            "the row scale out of range");
  if (h_grammar)                                  // the descriptor itself: before anything is read back from the device
    if (const char* bad = mt3k::bad_token_grammar(*h_grammar, vocab)) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  if (h_notes)
    if (const char* bad = mt3k::bad_note_grammar(*h_notes, vocab)) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
  if (h_sampling) {                               // as mt3_engine_set_sampling and mt3_engine_decode check it
    if (const char* bad = mt3s_bad_params(h_sampling)) return mt3::fail(MT3_ERR_INVALID, who + ": " + bad);
    if (vocab > MT3_SAMPLING_MAX_VOCAB) return mt3::fail(MT3_ERR_INVALID, who + ": sampling needs a vocabulary of at most 2048");
    if (mode != 0) return mt3::fail(MT3_ERR_INVALID, who + ": beam-1 (mode 1) does not sample");
  }
  mt3k::TokenMask tm{};
  if (masked) MT3_OP_TRY(driver_masks(who, d_masks, n_masks, d_row_mask, rows, vocab, 2, &tm));
  mt3k::TokenPrompt tp{};
  if (d_prompts) MT3_OP_TRY(driver_prompts(who, d_prompts, stride, d_row_prompt, rows, vocab, &tp));
  mt3k::TokenGrammar gr{};
  if (h_grammar) MT3_OP_TRY(driver_grammar(who, h_grammar, masked ? d_masks : nullptr, n_masks, vocab, 2, &gr));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(rows);
  Scratch m;
  MT3_OP_TRY(m.alloc(6 * Scratch::piece(n * 4) + Scratch::piece(2 * n * 4) + Scratch::piece(4) +
                         Scratch::piece((static_cast<size_t>(num_steps) + 3) * 4),
                     s));
  mt3k::ArgmaxStepArgs a{};
  a.vocab = vocab;
  a.ids = d_ids;
  a.ids_stride = num_steps;
  a.st.cur_tok = m.take<int>(n);
  a.st.done = m.take<int>(n);
  a.st.step = m.take<int>(n);
  int* len = m.take<int>(n);
  int* len_row = m.take<int>(n);
  float* f = m.take<float>(2 * n);
  a.st.n_done = m.take<int>(1);
  if (gr.on) a.st.gram = m.take<int>(n);
  a.gr = gr;
  float* d_bp = m.take<float>(static_cast<size_t>(num_steps) + 3);
  a.in.max_pos = num_steps + 1;
  if (mode == 1) a.beam = mt3k::BeamState{f, len, d_bp, rows, len_row};
  // a row that max_len closes is retired, as it is in the engine's streaming jobs (the only ones that set max_len)
  a.rt = mt3k::StepRetire{max_len > 0 ? 1 : 0, nullptr, nullptr, nullptr, max_len};
  a.B = rows;
  a.tm = tm;
  a.tp = tp;
  MT3_HIP_CHECK(hipMemsetAsync(d_ids, 0, n * num_steps * 4, s));
  MT3_HIP_CHECK(hipMemsetAsync(len, 0xFF, n * 4, s));                       // -1: nothing finished
  MT3_HIP_CHECK(hipMemsetAsync(len_row, 0xFF, n * 4, s));
  if (gr.on) MT3_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.st.gram), mt3g_initial(&gr.g), n, s));
  MT3_OP_TRY(upload_brevity(d_bp, num_steps, s));
  Scratch nm;
  if (h_notes) MT3_OP_TRY(driver_notes(who, h_notes, masked ? d_masks : nullptr, n_masks, vocab, 2, n, s, &nm, &a.nt, &a.st));
  // sampling: the parameters and the rows' streams in device memory of their own (freed with `sm`)
  Scratch sm;
  mt3k::SampleStepArgs sa{};
  if (h_sampling) {
    MT3_OP_TRY(sm.alloc(Scratch::piece(sizeof(mt3_sampling)) + 2 * Scratch::piece(n * 8) + Scratch::piece(n * 4), s));
    mt3_sampling* d_sp = sm.take<mt3_sampling>(1);
    uint64_t* d_stream = sm.take<uint64_t>(n);
    uint64_t* d_seed = sm.take<uint64_t>(n);
    int* d_row = sm.take<int>(n);                              // row i's stream (and seed) is entry i of its table
    MT3_HIP_CHECK(hipMemcpyAsync(d_sp, h_sampling, sizeof(mt3_sampling), hipMemcpyHostToDevice, s));
    if (h_row_stream) MT3_HIP_CHECK(hipMemcpyAsync(d_stream, h_row_stream, n * 8, hipMemcpyHostToDevice, s));
    if (h_row_seed) MT3_HIP_CHECK(hipMemcpyAsync(d_seed, h_row_seed, n * 8, hipMemcpyHostToDevice, s));
    MT3_OP_TRY(mt3k::launch_iota(d_row, rows, s));
    MT3_HIP_CHECK(hipStreamSynchronize(s));                    // the host arrays are the caller's
    sa.params = d_sp;
    if (h_row_stream) sa.stream = mt3k::SampleStream{d_stream, d_row, nullptr, 1};
    if (h_row_seed) sa.seed = mt3k::SampleStream{d_seed, d_row, nullptr, 1};
  }
  for (int t = 0; t < num_steps; ++t) {
    a.logits = d_logits + static_cast<size_t>(t) * n * vocab;
    a.ls = mt3k::LogitScale{d_ss ? d_ss + static_cast<size_t>(t) * n * n_ss : nullptr, n_ss, dim};
    if (h_sampling) {
      sa.a = a;
      MT3_OP_TRY(mt3k::launch_sample_step(sa, s));
    } else {
      MT3_OP_TRY(mt3k::launch_argmax_step(a, s));
    }
    MT3_HIP_CHECK(hipMemcpyAsync(h_done + static_cast<size_t>(t) * n, a.st.done, n * 4, hipMemcpyDeviceToHost, s));
    if (gr.on && h_state)
      MT3_HIP_CHECK(hipMemcpyAsync(h_state + static_cast<size_t>(t) * n, a.st.gram, n * 4, hipMemcpyDeviceToHost, s));
    if (a.nt.on) MT3_OP_TRY(driver_notes_out(a.st, n, t, h_note, h_held, s));
  }
  if (mode == 1) MT3_OP_TRY(mt3k::launch_beam1_finalize(d_ids, num_steps, len_row, rows, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));
  return MT3_OK;
}

extern "C" int mt3_op_token_steps_scripted(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                           int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len,
                                           int32_t* d_ids, int32_t* h_done, void* stream) {
  return token_steps_driver("mt3_op_token_steps_scripted", false, d_logits, d_ss, n_ss, dim, rows, vocab, num_steps, mode,
                            max_len, d_ids, h_done, stream, nullptr, 0, nullptr);
}

extern "C" int mt3_op_token_steps_masked(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                         int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids,
                                         int32_t* h_done, void* stream, const uint32_t* d_masks, int32_t n_masks,
                                         const int32_t* d_row_mask) {
  return token_steps_driver("mt3_op_token_steps_masked", true, d_logits, d_ss, n_ss, dim, rows, vocab, num_steps, mode,
                            max_len, d_ids, h_done, stream, d_masks, n_masks, d_row_mask);
}

extern "C" int mt3_op_token_steps_prompted(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                           int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids,
                                           int32_t* h_done, void* stream, const uint32_t* d_masks, int32_t n_masks,
                                           const int32_t* d_row_mask, const int32_t* d_prompts, int32_t stride,
                                           const int32_t* d_row_prompt) {
  return token_steps_driver("mt3_op_token_steps_prompted", d_masks != nullptr, d_logits, d_ss, n_ss, dim, rows, vocab,
                            num_steps, mode, max_len, d_ids, h_done, stream, d_masks, n_masks, d_row_mask, d_prompts, stride,
                            d_row_prompt);
}

extern "C" int mt3_op_beam_search_grammar(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim,
                                          int32_t elems, int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len,
                                          const float* d_table, const float* d_pos, int32_t dim_e, int32_t* d_ids,
                                          int32_t* d_all_ids, float* d_scores, float* d_y_next, int32_t* h_trace,
                                          float* h_live, int32_t* h_forks, int32_t* h_steps_run, void* stream,
                                          const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                                          const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt,
                                          const mt3_token_grammar* h_grammar, int32_t* h_state) {
  return beam_search_driver("mt3_op_beam_search_grammar", d_masks != nullptr, d_logits, d_ss, n_ss, dim, elems, k, vocab,
                            num_steps, max_len, d_table, d_pos, dim_e, d_ids, d_all_ids, d_scores, d_y_next, h_trace, h_live,
                            h_forks, h_steps_run, stream, d_masks, n_masks, d_row_mask, d_prompts, stride, d_row_prompt,
                            h_grammar, h_state);
}

extern "C" int mt3_op_token_steps_grammar(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                          int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids,
                                          int32_t* h_done, void* stream, const uint32_t* d_masks, int32_t n_masks,
                                          const int32_t* d_row_mask, const int32_t* d_prompts, int32_t stride,
                                          const int32_t* d_row_prompt, const mt3_token_grammar* h_grammar,
                                          int32_t* h_state) {
  return token_steps_driver("mt3_op_token_steps_grammar", d_masks != nullptr, d_logits, d_ss, n_ss, dim, rows, vocab,
                            num_steps, mode, max_len, d_ids, h_done, stream, d_masks, n_masks, d_row_mask, d_prompts, stride,
                            d_row_prompt, h_grammar, h_state);
}

extern "C" int mt3_op_token_steps_sampled(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                          int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids,
                                          int32_t* h_done, void* stream, const uint32_t* d_masks, int32_t n_masks,
                                          const int32_t* d_row_mask, const int32_t* d_prompts, int32_t stride,
                                          const int32_t* d_row_prompt, const mt3_token_grammar* h_grammar,
                                          int32_t* h_state, const mt3_sampling* h_sampling, const uint64_t* h_row_stream) {
  return token_steps_driver("mt3_op_token_steps_sampled", d_masks != nullptr, d_logits, d_ss, n_ss, dim, rows, vocab,
                            num_steps, mode, max_len, d_ids, h_done, stream, d_masks, n_masks, d_row_mask, d_prompts, stride,
                            d_row_prompt, h_grammar, h_state, h_sampling, h_row_stream);
}

extern "C" int mt3_op_token_steps_notes(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                        int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids,
                                        int32_t* h_done, void* stream, const uint32_t* d_masks, int32_t n_masks,
                                        const int32_t* d_row_mask, const int32_t* d_prompts, int32_t stride,
                                        const int32_t* d_row_prompt, const mt3_note_grammar* h_notes, int32_t* h_state,
                                        const mt3_sampling* h_sampling, const uint64_t* h_row_stream, int32_t* h_note,
                                        uint32_t* h_held) {
  return token_steps_driver("mt3_op_token_steps_notes", d_masks != nullptr, d_logits, d_ss, n_ss, dim, rows, vocab,
                            num_steps, mode, max_len, d_ids, h_done, stream, d_masks, n_masks, d_row_mask, d_prompts, stride,
                            d_row_prompt, nullptr, h_state, h_sampling, h_row_stream, h_notes, h_note, h_held);
}

extern "C" int mt3_op_token_steps_seeded(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                         int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids,
                                         int32_t* h_done, void* stream, const uint32_t* d_masks, int32_t n_masks,
                                         const int32_t* d_row_mask, const int32_t* d_prompts, int32_t stride,
                                         const int32_t* d_row_prompt, const mt3_note_grammar* h_notes, int32_t* h_state,
                                         const mt3_sampling* h_sampling, const uint64_t* h_row_stream, int32_t* h_note,
                                         uint32_t* h_held, const uint64_t* h_row_seed) {
  return token_steps_driver("mt3_op_token_steps_seeded", d_masks != nullptr, d_logits, d_ss, n_ss, dim, rows, vocab,
                            num_steps, mode, max_len, d_ids, h_done, stream, d_masks, n_masks, d_row_mask, d_prompts, stride,
                            d_row_prompt, nullptr, h_state, h_sampling, h_row_stream, h_notes, h_note, h_held, h_row_seed);
}

extern "C" int mt3_op_beam_search_notes(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t elems,
                                        int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len, const float* d_table,
                                        const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids,
                                        float* d_scores, float* d_y_next, int32_t* h_trace, float* h_live,
                                        int32_t* h_forks, int32_t* h_steps_run, void* stream, const uint32_t* d_masks,
                                        int32_t n_masks, const int32_t* d_row_mask, const int32_t* d_prompts,
                                        int32_t stride, const int32_t* d_row_prompt, const mt3_note_grammar* h_notes,
                                        int32_t* h_state, int32_t* h_note, uint32_t* h_held) {
  return beam_search_driver("mt3_op_beam_search_notes", d_masks != nullptr, d_logits, d_ss, n_ss, dim, elems, k, vocab,
                            num_steps, max_len, d_table, d_pos, dim_e, d_ids, d_all_ids, d_scores, d_y_next, h_trace, h_live,
                            h_forks, h_steps_run, stream, d_masks, n_masks, d_row_mask, d_prompts, stride, d_row_prompt,
                            nullptr, h_state, h_notes, h_note, h_held);
}

extern "C" int mt3_note_grammar_check(const mt3_note_grammar* n, int32_t vocab) {
  if (!n) return mt3::fail(MT3_ERR_INVALID, "mt3_note_grammar_check: null descriptor");
  if (const char* bad = mt3k::bad_note_grammar(*n, vocab))
    return mt3::fail(MT3_ERR_INVALID, std::string("mt3_note_grammar_check: ") + bad);
  return MT3_OK;
}

extern "C" int mt3_op_beam_reorder(int32_t n_layers, int32_t H, int32_t cap, int32_t kv_esize, int32_t slots,
                                   void* const* h_k, void* const* h_v, void* const* h_scale, const int32_t* d_fork_src,
                                   const int32_t* d_slot_row, const int32_t* d_step, const int32_t* d_done,
                                   void* stream) {
  if (!h_k || !h_v || !d_fork_src || !d_slot_row || !d_step || !d_done)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_reorder: null argument");
  if (n_layers <= 0 || n_layers > mt3k::kRefillMaxLayers)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_reorder: 1 .. 16 layers");
  mt3k::BeamReorderArgs r{};
  r.n_layers = n_layers;
  r.H = H;
  r.cap = cap;
  r.kv_esize = kv_esize;
  r.slots = slots;
  for (int l = 0; l < n_layers; ++l) {
    r.k[l] = static_cast<char*>(h_k[l]);
    r.v[l] = static_cast<char*>(h_v[l]);
    r.scale[l] = h_scale ? static_cast<float2*>(h_scale[l]) : nullptr;
  }
  r.fork_src = d_fork_src;
  r.slot_row = d_slot_row;
  r.step = d_step;
  r.done = d_done;
  MT3_OP_TRY(mt3k::launch_beam_reorder(r, static_cast<hipStream_t>(stream)));
  MT3_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return MT3_OK;
}

// ------------------------------------------------------------------ drivers of the slot-moving launches
// mt3_op_embed_rows / mt3_op_slot_compact / mt3_op_slot_refill / mt3_op_beam_refill / mt3_op_beam_stream_init
// (mt3_hip.h): the launchers above, unchanged, on slot state the caller owns.  Everything a launcher refuses is refused
// here first, before the driver's own scratch is allocated.
namespace {

mt3k::InputRow input_row_of(const mt3_input_row_view& v) {
  mt3k::InputRow r{};
  r.table = v.table;
  r.pos = v.pos;
  r.max_pos = v.max_pos;
  r.y = v.y;
  r.y_ct = v.y_ct;
  r.y_ss = v.y_ss;
  r.dim = v.dim;
  r.rp = mt3k::RowProj{v.ew, v.pw, v.q_out, v.q_n};
  return r;
}

mt3k::SlotState slot_state_of(const mt3_slot_state_view& v) {
  return mt3k::SlotState{v.done, v.slot_row, v.slot_seg, v.step, v.cur_tok, v.n_done};
}

// a written input row in the split-capable layout the slot movers take: the row, its tables, dim % 16 == 0
bool bad_written_row(const mt3k::InputRow& r) {
  return !r.y || !r.table || !r.pos || r.max_pos < 1 || r.dim <= 0 || r.dim % 16 || (r.y_ct && !r.y_ss) ||
         (r.rp.q_out && (!r.rp.ew || !r.rp.pw || r.rp.q_n <= 0 || r.rp.q_n % 4));
}

// MT3_OK and `out` filled, or what is wrong with a staged-cross view of n_new segments (unused when n_new == 0)
// (per > 1, mt3_op_slot_refill_draws: the view's src_batch counts staged ENTRIES, its src_entry0 draws)
int staged_cross_of(const mt3_staged_cross_view* v, int n_new, const char* who, mt3k::StagedCross* out, int per = 1) {
  *out = mt3k::StagedCross{};
  out->per = per;
  if (n_new <= 0) return MT3_OK;
  const std::string w(who);
  if (!v || !v->src || !v->dst) return mt3::fail(MT3_ERR_INVALID, w + ": segments to hand out need a staging chunk");
  if (v->n_layers <= 0 || v->n_layers > mt3k::kRefillMaxLayers || v->row_bytes == 0 || v->row_bytes % 16 ||
      v->sc_bytes % 16 || v->src_batch <= 0 || v->dst_batch <= 0 || v->src_entry0 < 0 ||
      static_cast<long long>(v->src_entry0) + n_new > static_cast<long long>(v->src_batch) * per ||
      static_cast<long long>(v->src_batch) * per > 0x7fffffffLL)
    return mt3::fail(MT3_ERR_INVALID, w + ": bad staging chunk");
  out->n_layers = v->n_layers;
  out->src_batch = v->src_batch * per;
  out->src_entry0 = v->src_entry0;
  out->dst_batch = v->dst_batch;
  out->row_bytes = v->row_bytes;
  out->sc_bytes = v->sc_bytes;
  for (int l = 0; l < v->n_layers; ++l) {
    out->src[l] = static_cast<const char*>(v->src[l]);
    out->dst[l] = static_cast<char*>(v->dst[l]);
    out->src_sc[l] = v->src_sc ? static_cast<const char*>(v->src_sc[l]) : nullptr;
    out->dst_sc[l] = v->dst_sc ? static_cast<char*>(v->dst_sc[l]) : nullptr;
    if (!out->src[l] || !out->dst[l]) return mt3::fail(MT3_ERR_INVALID, w + ": missing staging chunk or cache of a layer");
    if (out->src_sc[l] && (!out->dst_sc[l] || v->sc_bytes == 0))
      return mt3::fail(MT3_ERR_INVALID, w + ": staged scale rows need their cache rows and sc_bytes");
  }
  return MT3_OK;
}

constexpr int kOpMaxSlots = 1 << 16;

}  // namespace

extern "C" int mt3_op_embed_rows(const mt3_input_row_view* in, const int32_t* d_tok, const int32_t* d_t, int32_t rows,
                                 void* stream) {
  if (!in || !in->y || !d_tok || !d_t) return mt3::fail(MT3_ERR_INVALID, "mt3_op_embed_rows: null argument");
  if (rows <= 0 || rows > kOpMaxSlots) return mt3::fail(MT3_ERR_INVALID, "mt3_op_embed_rows: 1 .. 65536 rows");
  if (in->q_out && in->q_n <= 0) return mt3::fail(MT3_ERR_INVALID, "mt3_op_embed_rows: the row projection needs q_n > 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  MT3_OP_TRY(mt3k::launch_embed(input_row_of(*in), d_tok, d_t, rows, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));
  return MT3_OK;
}

extern "C" int mt3_op_slot_compact(const mt3_slot_state_view* st, const mt3_input_row_view* in, float* d_beam_f,
                                   int32_t beam_rows, int32_t* d_beam_len, int32_t rows, int32_t* h_perm, void* stream) {
  if (!st || !in || !st->done || !st->slot_row || !st->step || !st->cur_tok || !in->y)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_slot_compact: null argument");
  if (rows <= 0 || rows > kOpMaxSlots || in->dim <= 0 || in->dim % 16 || (in->q_out && (in->q_n <= 0 || in->q_n % 4)) ||
      (in->y_ct && !in->y_ss))
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_slot_compact: 1 .. 65536 rows, dim % 16 == 0, q_n % 4 == 0, y_ss with y_ct");
  if (d_beam_f ? (!d_beam_len || beam_rows < rows) : d_beam_len != nullptr)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_slot_compact: the beam state is f (two arrays beam_rows >= rows apart) "
                                      "and len, together");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(rows), dim = static_cast<size_t>(in->dim);
  const size_t q_n = in->q_out ? static_cast<size_t>(in->q_n) : 0;
  Scratch m;
  MT3_OP_TRY(m.alloc(Scratch::piece(n * dim * 4) + Scratch::piece(n * dim * 2) + Scratch::piece(n * dim / 16 * 4) +
                         Scratch::piece(n * q_n * 4) + Scratch::piece(n * mt3k::kCompactInts * 4) + Scratch::piece(n * 8) +
                         Scratch::piece(n * 4) + Scratch::piece((n + 1) * 4),
                     s, 0xFF));
  mt3k::CompactArgs c{};
  c.st = slot_state_of(*st);
  c.in = input_row_of(*in);
  if (!in->q_out) c.in.rp = mt3k::RowProj{};
  c.beam = mt3k::BeamState{d_beam_f, d_beam_len, nullptr, beam_rows, nullptr};
  // the scatter pass reads a form back from its scratch wherever that scratch exists: a form that is not in use has none
  c.s_y = m.take<float>(n * dim);
  unsigned short* s_y_ct = m.take<unsigned short>(n * dim);
  float* s_y_ss = m.take<float>(n * dim / 16);
  float* s_qkvf = m.take<float>(n * q_n);
  c.s_y_ct = in->y_ct ? s_y_ct : nullptr;
  c.s_y_ss = in->y_ss ? s_y_ss : nullptr;
  c.s_qkvf = in->q_out ? s_qkvf : nullptr;
  c.s_int = m.take<int>(n * mt3k::kCompactInts);
  c.s_beam = m.take<float>(n * 2);
  c.s_seg = m.take<int>(n);
  c.perm = m.take<int>(n + 1);
  c.rows = rows;
  MT3_OP_TRY(mt3k::launch_compact(c, s));
  if (h_perm) MT3_HIP_CHECK(hipMemcpyAsync(h_perm, c.perm, (n + 1) * 4, hipMemcpyDeviceToHost, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));
  return MT3_OK;
}

// shared body of mt3_op_slot_refill (per = 1) and mt3_op_slot_refill_draws
static int slot_refill_driver(const std::string& who, const mt3_slot_state_view* st, const mt3_input_row_view* in,
                              float* d_beam_f, int32_t beam_rows, int32_t* d_beam_len, int32_t* d_beam_len_row,
                              int32_t* d_ids, int32_t ids_stride, int32_t* d_out_ids, int32_t rows, int32_t n_new,
                              int32_t first_seg, const mt3_staged_cross_view* x, int32_t per, int32_t* h_plan,
                              void* stream) {
  if (!st || !in || !st->done || !st->slot_row || !st->slot_seg || !st->step || !st->cur_tok || !st->n_done || !d_ids ||
      !d_out_ids)
    return mt3::fail(MT3_ERR_INVALID, who + ": null argument");
  if (per < 1) return mt3::fail(MT3_ERR_INVALID, who + ": per must be at least 1");
  if (rows <= 0 || rows > kOpMaxSlots || n_new < 0 || n_new > rows || ids_stride <= 0 || first_seg < 0)
    return mt3::fail(MT3_ERR_INVALID, who + ": 1 .. 65536 rows, 0 <= n_new <= rows, ids_stride > 0, "
                                      "first_seg >= 0");
  if (d_beam_f ? (!d_beam_len || !d_beam_len_row || beam_rows < rows) : (d_beam_len || d_beam_len_row))
    return mt3::fail(MT3_ERR_INVALID, who + ": the beam state is f (two arrays beam_rows >= rows apart), "
                                      "len and len_row, together");
  mt3k::RefillArgs a{};
  a.in = input_row_of(*in);
  if (bad_written_row(a.in))
    return mt3::fail(MT3_ERR_INVALID, who + ": the input row needs y, its tables, dim % 16 == 0, y_ss with "
                                      "y_ct, and ew / pw / q_n % 4 == 0 with q_out");
  MT3_OP_TRY(staged_cross_of(x, n_new, who.c_str(), &a.x, per));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(rows);
  Scratch m;
  MT3_OP_TRY(m.alloc(Scratch::piece((n + 1) * 4), s, 0xFF));
  a.st = slot_state_of(*st);
  a.beam = mt3k::BeamState{d_beam_f, d_beam_len, nullptr, beam_rows, d_beam_len_row};
  a.ids = d_ids;
  a.ids_stride = ids_stride;
  a.out_ids = d_out_ids;
  a.plan = m.take<int>(n + 1);
  a.rows = rows;
  a.n_new = n_new;
  a.first_seg = first_seg;
  MT3_OP_TRY(mt3k::launch_refill(a, s));
  if (h_plan) MT3_HIP_CHECK(hipMemcpyAsync(h_plan, a.plan, (n + 1) * 4, hipMemcpyDeviceToHost, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));
  return MT3_OK;
}

extern "C" int mt3_op_slot_refill(const mt3_slot_state_view* st, const mt3_input_row_view* in, float* d_beam_f,
                                  int32_t beam_rows, int32_t* d_beam_len, int32_t* d_beam_len_row, int32_t* d_ids,
                                  int32_t ids_stride, int32_t* d_out_ids, int32_t rows, int32_t n_new, int32_t first_seg,
                                  const mt3_staged_cross_view* x, int32_t* h_plan, void* stream) {
  return slot_refill_driver("mt3_op_slot_refill", st, in, d_beam_f, beam_rows, d_beam_len, d_beam_len_row, d_ids, ids_stride,
                            d_out_ids, rows, n_new, first_seg, x, 1, h_plan, stream);
}

extern "C" int mt3_op_slot_refill_draws(const mt3_slot_state_view* st, const mt3_input_row_view* in, float* d_beam_f,
                                        int32_t beam_rows, int32_t* d_beam_len, int32_t* d_beam_len_row, int32_t* d_ids,
                                        int32_t ids_stride, int32_t* d_out_ids, int32_t rows, int32_t n_new,
                                        int32_t first_seg, const mt3_staged_cross_view* x, int32_t per, int32_t* h_plan,
                                        void* stream) {
  return slot_refill_driver("mt3_op_slot_refill_draws", st, in, d_beam_f, beam_rows, d_beam_len, d_beam_len_row, d_ids,
                            ids_stride, d_out_ids, rows, n_new, first_seg, x, per, h_plan, stream);
}

extern "C" int mt3_op_beam_refill(const mt3_beam_k_view* b, const mt3_slot_state_view* st, const mt3_input_row_view* in,
                                  int32_t L, int32_t num_steps, int32_t* d_out_ids, int32_t* d_out_all,
                                  float* d_out_scores, int32_t n_new, int32_t first_seg, const mt3_staged_cross_view* x,
                                  int32_t* h_plan, void* stream) {
  if (!b || !st || !in || !b->live || !b->fin_score || !b->fin_step || !b->fin_beam || !b->hist_par || !b->hist_tok ||
      !b->fork_src || !st->done || !st->slot_row || !st->slot_seg || !st->step || !st->cur_tok || !st->n_done || !d_out_ids)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_refill: null argument");
  if (b->k < 1 || b->k > mt3k::kBeamMaxK || b->vocab < 1 || b->vocab > 2048)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_refill: k must be 1 .. 8 and vocab <= 2048");
  if (b->elems <= 0 || b->elems > kOpMaxSlots / mt3k::kBeamMaxK || b->hist_stride < b->elems * b->k || n_new < 0 ||
      n_new > b->elems || first_seg < 0)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_refill: 1 .. 8192 elems, hist_stride >= elems * k, 0 <= n_new <= "
                                      "elems, first_seg >= 0");
  if (L <= 0 || num_steps <= 0 || num_steps > L)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_refill: 1 <= num_steps <= L");
  if ((static_cast<size_t>(num_steps) + L) * b->k * sizeof(unsigned short) > 65536)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_refill: history and decodes of an element exceed 64 KB of LDS");
  mt3k::BeamRefillArgs a{};
  a.b.in = input_row_of(*in);
  if (bad_written_row(a.b.in))
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_refill: the input row needs y, its tables, dim % 16 == 0, y_ss with "
                                      "y_ct, and ew / pw / q_n % 4 == 0 with q_out");
  MT3_OP_TRY(staged_cross_of(x, n_new, "mt3_op_beam_refill", &a.x));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(b->elems);
  Scratch m;
  MT3_OP_TRY(m.alloc(Scratch::piece((n + 1) * 4), s, 0xFF));
  a.b.vocab = b->vocab;
  a.b.k = b->k;
  a.b.elems = b->elems;
  a.b.st = slot_state_of(*st);
  a.b.live = b->live;
  a.b.fin_score = b->fin_score;
  a.b.fin_step = b->fin_step;
  a.b.fin_beam = b->fin_beam;
  a.b.hist_par = b->hist_par;
  a.b.hist_tok = b->hist_tok;
  a.b.hist_stride = b->hist_stride;
  a.b.fork_src = b->fork_src;
  a.plan = m.take<int>(n + 1);
  a.L = L;
  a.num_steps = num_steps;
  a.out_ids = d_out_ids;
  a.out_all = d_out_all;
  a.out_scores = d_out_scores;
  a.n_new = n_new;
  a.first_seg = first_seg;
  MT3_OP_TRY(mt3k::launch_beam_refill(a, s));
  if (h_plan) MT3_HIP_CHECK(hipMemcpyAsync(h_plan, a.plan, (n + 1) * 4, hipMemcpyDeviceToHost, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));
  return MT3_OK;
}

extern "C" int mt3_op_beam_stream_init(int32_t* d_done, int32_t* d_slot_seg, int32_t* d_fork_src, int32_t* d_slot_row,
                                       int32_t* d_n_done, int32_t slots, int32_t groups, const int32_t* h_group_slots,
                                       void* stream) {
  if (!d_done || !d_slot_seg || !d_fork_src || !d_slot_row || !d_n_done || !h_group_slots)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_stream_init: null argument");
  if (slots <= 0 || slots > kOpMaxSlots || groups < 1 || groups > 4)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_beam_stream_init: 1 .. 65536 slots in 1 .. 4 groups");
  mt3k::GroupSlots gs{};
  for (int g = 0; g < groups; ++g) gs.n[g] = h_group_slots[g];
  hipStream_t s = static_cast<hipStream_t>(stream);
  MT3_OP_TRY(mt3k::launch_beam_stream_init(d_done, d_slot_seg, d_fork_src, d_slot_row, d_n_done, slots, groups, gs, s));
  MT3_HIP_CHECK(hipStreamSynchronize(s));
  return MT3_OK;
}
