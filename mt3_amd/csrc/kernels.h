// Internal launcher interface between the engine (engine.hip) and the kernel files.
#ifndef MT3_KERNELS_H_
#define MT3_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "mt3_hip.h"

namespace mt3k {

struct GemmArgs {
  const void* A;      // [M, lda]  f32 or compute type
  const void* Wt;     // [N, K]    compute type
  void* out;          // see epilogue
  const float* aux;   // EPI_POS: positional table [seq_len, N]
  int M, N, K;
  int lda, ldo;
  int seq_len;        // EPI_POS / EPI_HEADS: rows per batch item
  // bf16 decode path: the residual stream travels as f32 rows PLUS a compute-type copy and, per row, the sums of
  // squares of every 16-column group (exact f32), so that the RMSNorm-fused GEMMs read half the A bytes and need
  // no statistics pass of their own
  const float* a_ss;  // norm == 2: [M][K/16] partial sums of squares of the rows whose compute-type copy is A
  void* out_ct;       // EPI_RESID: also write the updated rows in the compute type here [M][ldo] (nullptr: no)
  float* out_ss;      // EPI_RESID with out_ct: [M][N/16] partial sums of squares of the updated rows
  // kEpiStoreQ / kEpiResidQ / kEpiGegluP: output columns [n_split, N) are a SECOND product riding in the same launch --
  // they go to out2 (f32, unscaled, no activation; ResidQ accumulates into it), columns [0, n_split) take the STORE /
  // RESID / GEGLU path.  kEpiGegluP: Wt's N rows are padded to whole 64-column tiles, out2 rows are ld2 columns wide
  // and only those are written
  float* out2;
  int n_split;
  int ld2;            // row stride of out2 in floats (0: N - n_split)
  // tile -> XCD dealing: 0 = an XCD owns a run of row blocks (all weight columns pass through its L2), 1 = an XCD
  // owns a run of weight-column tiles for ALL row blocks (its L2 sees 1/8 of the weights; set by launch_gemm)
  int n_major;
  // decode-sized f32 launches: this launch is one of several row groups running side by side (set by the engine), so
  // a row block of >= 256 rows takes the 64 x 32 tiles (gemm.hip: launch_tile); alone on the chip the 32-row tiles win
  int concurrent;
};
// internal epilogues (not part of the C ABI): STORE / RESID / GEGLU with a second f32 output region, see GemmArgs::out2
// (8 was the two-source fold launch of rounds 3-6)
constexpr int kEpiStoreQ = 6, kEpiResidQ = 7, kEpiGegluP = 9;

// norm: 0 none, 1 fused RMSNorm with statistics from the f32 A stream, 2 fused RMSNorm from g.a_ss (A = compute type)
int launch_gemm(int dtype, const GemmArgs& g, bool a_f32, int norm, int epi, bool small, hipStream_t s);

// f32 operands as three bf16 planes (gemm_x6_kernel, the f32 engine's encoder): A f32 [M][lda]; g.Wt / Wm / Wl = the hi /
// mid / lo bf16 planes [N][K] of the weight; outputs f32.  (norm, epi): (true, STORE | GEGLU), (false, RESID | POS | HEADS)
int launch_gemm_x6(const GemmArgs& g, const void* Wm, const void* Wl, bool norm, int epi, hipStream_t s);

// encoder self-attention, qkv [B, T, 3, H, 64] -> out [B, T, H*64]
int launch_encoder_attention(int dtype, const void* qkv, void* out, int B, int T, int H, hipStream_t s);
// the f32 engine's encoder attention with Q, K, V and P as three bf16 planes each (enc_attention_x6.hip): f32 qkv
// [B * T][3 * H * 64] -> f32 out [B * T][H * 64]; T = 256 or 512
int launch_encoder_attention_x6(const void* qkv, void* out, int B, int T, int H, hipStream_t s);

struct DecAttnArgs {
  const void* q;        // [B, q_stride] compute type; head h at +h*64
  int q_stride;
  void* kcache;         // [B, H, cap, 64]
  void* vcache;
  int cap;
  const void* new_k;    // [B, kv_stride] rows; head h at +h*64 (NULL: no append)
  const void* new_v;
  int kv_stride;
  const int* step;      // device, per row: n_keys = step[b] + 1 (NULL: use n_keys)
  int n_keys;
  void* out;            // [B, H*64] compute type
  int B, H;
  // non-null: the cache holds OCP e4m3 bytes [B, H, cap, 64] and this is its side array [B, H, cap] of
  // {k_scale, v_scale} (power-of-two row scales); q / new rows / out are bf16
  float2* kv_scale;
  // bf16 path, no append: the query arrives as UNNORMALISED f32 rows q_f32 [B][q_stride] plus the partial sums of
  // squares q_ss [B][q_ss_n] of the residual row it was projected from (emb = 16 * q_ss_n); the kernel applies
  // rsqrt(mean + 1e-6) itself (the cross-attention q-projection folded into the neighbouring GEMM launches)
  const float* q_f32;
  const float* q_ss;
  int q_ss_n;
  // Row retirement (mt3_engine_decode with MT3_DECODE_EARLY_EXIT): `done` [B] per SLOT -- a workgroup whose slot has
  // finished (EOS emitted / beam search closed) returns before it requests a single cache byte; `cache_row` [B] maps a
  // slot to the row of kcache / vcache / kv_scale it owns (the live slots are compacted to the front of the batch while
  // the caches stay where they are).  Both nullptr: slot b = row b, every row is attended (the canonical schedule).
  const int* done;
  const int* cache_row;
};
// bf16 K rows then V rows ([2][rows][64]) -> e4m3 [2][rows][64] + float2 scales [rows]
int launch_kv_quantize_fp8(const void* src_bf16, void* dst_fp8, void* scales, int rows, hipStream_t s);
int launch_decode_attention(int dtype, const DecAttnArgs& a, hipStream_t s);

// out_ct[row] = x[row] * rsqrt(mean(x^2)+eps) * scale ; optional f32 copy
int launch_rmsnorm(int dtype, const float* x, const float* scale, void* out_ct, float* out_f32, int rows, int dim,
                   hipStream_t s);
// x f32 [rows][dim] -> bf16 copy + per-16-column sums of squares (the split residual form, see GemmArgs)
int launch_residual_split(const float* x, void* x_ct, float* x_ss, int rows, int dim, hipStream_t s);
// first-layer projections by table lookup (the decoder's first QKV launch folded away): when q_out != nullptr the
// kernels that produce a decoder input row Embed(tok) + FixedEmbed[t] also write its UNNORMALISED projection
// q_out[b][0 .. q_n) = ew[tok] + pw[t]  (ew = embedding . W, pw = position table . W, both f32 [rows][q_n])
struct RowProj {
  const float* ew;
  const float* pw;
  float* q_out;
  int q_n;
};
// A decoder input row Embed(tok) + FixedEmbed[min(t, max_pos - 1)] and the forms it is written in (put_input_row,
// decode_ops.hip; checked by one validator there).  The slot-indexed pointers are those of the step's or group's first slot.
struct InputRow {
  const float* table;   // token embedding [vocab][dim] (row 0 = BOS)
  const float* pos;     // position table [max_pos][dim]
  int max_pos;
  float* y;             // [slots][dim] f32 rows (nullptr: the kernel writes no input row)
  void* y_ct;           // bf16 copy (nullptr: f32 engine, or no split form)
  float* y_ss;          // [slots][dim / 16] sums of squares of every 16-column group (nullptr: single residual stream)
  int dim;
  RowProj rp;           // q_out = the slots' layer-0 rows (nullptr: no qkv-fold)
};
// The per-slot state that lives from one step to the next.  Pointers of the step's or group's first slot (n_done: the
// row group's counter of finished slots); a kernel reads the ones it needs.
struct SlotState {
  int* done;            // [slots] set once the slot has finished (EOS / search closed / out of positions)
  int* slot_row;        // [slots] slot -> row of the caches and of `ids`
  int* slot_seg;        // [slots] in-flight batching: the segment the slot decodes (-1: none)
  int* step;            // [slots] position counter
  int* cur_tok;         // [slots] input token of the next step
  int* n_done;
  int* gram;            // [slots] packed state of the event grammar (TokenGrammar; nullptr: not kept -- it then neither
                        // travels with the slot nor is reset)
  // note-consistent decoding (TokenNotes; the state: include/mt3_hip.h, mt3n_*).  note == nullptr: not kept
  int* note;            // [slots] current program value | MT3_NOTE_VELOCITY_ZERO
  uint32_t* nrow;       // [slots][MT3_NOTE_ROW_WORDS] a copy of held[slot][current program]: what the pick reads, at an
                        // address that needs nothing but the slot index
  uint32_t* held;       // [slots][held_words] the sounding (program, pitch) pairs
  int held_words;       // mt3n_table_words of the descriptor in use
};
// logits that arrive UNNORMALISED (the logits projection folded into the last layer's MLP out-projection launch): the
// kernel that picks the token applies the decoder_norm row scale rsqrt(sum(ss[b][0 .. n_ss)) / dim + 1e-6) itself and
// writes the scaled logits back (ss == nullptr: the logits are final)
struct LogitScale {
  const float* ss;
  int n_ss;
  int dim;
};
// A per-segment table: fixed-stride rows in device memory and an optional index from segment to row.  The one indexing
// contract (seg_table_row, decode_ops.hip): the row of segment `seg` is rows + seg_row[seg] * stride; a null seg_row means
// row 0 for every segment; a negative seg or a negative index means no row.  rows == nullptr: no table -- the launchers
// then run the instantiations whose statements do not mention it.  `seg` is the segment index the EOS schedule uses
// (token kernel: rt.slot_seg[b] in in-flight jobs, else the row the slot decodes; its slot_seg here is unused) / the
// element's segment (beam kernel: slot_seg[first slot], else the block).  Its two uses:
//   TokenMask   constrained decoding (mt3_engine_set_token_masks; the rule: include/mt3_hip.h): bit sets over the
//               vocabulary, stride = ceil(vocab / 32) uint32 each, bit i % 32 of word i / 32 set = token i allowed.  The
//               kernel that picks the token treats the logit of a disallowed token as -inf (after the LogitScale multiply
//               and its write-back: the logits in memory stay the model's own).  No row: unconstrained.
//   TokenPrompt prompted decoding (mt3_engine_set_prompts; the rule: include/mt3_hip.h): forced token prefixes, `stride`
//               ids each, padded with 0.  A slot at position t < stride whose row holds P[t] != 0 is INSIDE its prompt: the
//               kernel that picks the token emits P[t], writes the next input row from it and leaves the search state alone
//               (no score, no EOS candidate, no stop test, no fork).  No row: no prompt.
template <typename T>
struct SegTable {
  const T* rows;          // [n_rows][stride]
  const int* seg_row;     // [segments] row index per segment, -1 = none (nullptr: row 0 for every segment); offset like
                          // StepRetire::eos_at / by the step's first element
  const int* slot_seg;    // beam kernel only: [slots] the segment of an element's first slot (nullptr: element = block)
  int stride;             // elements of T per row
};
using TokenMask = SegTable<uint32_t>;
using TokenPrompt = SegTable<int>;
// the one host-side check of a mask of ceil(vocab / 32) words: nullptr and *allowed = its number of allowed tokens, or
// what is wrong with it (EOS, id 1, must stay reachable; a pick needs two candidates; no bits past the vocabulary)
inline const char* bad_token_mask(const uint32_t* h_mask, int vocab, int* allowed) {
  const int words = (vocab + 31) / 32;
  int n = 0;
  for (int w = 0; w < words; ++w) n += __builtin_popcount(h_mask[w]);
  *allowed = n;
  if (vocab % 32 && (h_mask[words - 1] >> (vocab % 32))) return "bits at or past vocab are set in the last word";
  if (!(h_mask[0] & 2u)) return "a mask must allow EOS (id 1)";
  if (n < 2) return "a mask must allow at least 2 tokens";
  return nullptr;
}
// the one host-side check of a prompt row of `stride` ids: nullptr and *len = its length (the index of the first 0, or
// stride), or what is wrong with it (EOS, id 1, cannot be forced; 0 is padding and ends the prompt)
inline const char* bad_prompt(const int* h_prompt, int stride, int vocab, int* len) {
  int n = 0;
  while (n < stride && h_prompt[n] != 0) ++n;
  *len = n;
  for (int i = 0; i < stride; ++i) {
    if (h_prompt[i] != 0 && (h_prompt[i] < 2 || h_prompt[i] >= vocab)) return "a prompt id outside {0} and [2, vocab)";
    if (i > n && h_prompt[i] != 0) return "a non-zero prompt id after a 0";
  }
  if (n == 0) return "an empty prompt (its first id is 0)";
  return nullptr;
}
// Well-formed decoding (mt3_engine_set_token_grammar; the rule and the packed per-slot state: include/mt3_hip.h, mt3g_*).
// The descriptor travels by value in the kernel arguments; `on` selects the GRAMMAR instantiations of the token kernels,
// which read the slot's state from SlotState::gram in the batch of the logits, count a disallowed id as -inf where the
// mask does, and write advance(state, emitted token) back.  on == 0: the launchers run the instantiations whose
// statements do not mention it.
struct TokenGrammar {
  mt3_token_grammar g;
  int on;
};
// Note-consistent decoding (mt3_engine_set_note_grammar; the rule: include/mt3_hip.h, mt3n_*).  on selects the NOTES
// instantiations of the token kernels, which exist on top of the GRAMMAR ones only: the step's TokenGrammar then holds n.g.
// They read the slot's `note` int and its copy of the current program's row (SlotState::note / nrow) in the batch of the
// logits, count what the rule disallows as -inf where the grammar does, and the thread that owns the slot's bookkeeping
// writes the advanced state back: plain read-modify-writes of the row copy and the table, one owner per slot.
struct TokenNotes {
  mt3_note_grammar n;
  int on;
};
// the one host-side check of a grammar descriptor against a vocabulary: nullptr, or what is wrong with it
inline const char* bad_token_grammar(const mt3_token_grammar& g, int vocab) {
  const long long lo[4] = {g.shift_first, g.program_first, g.pitch_first, g.tie_id};
  const long long n[4] = {g.shift_count, g.program_count, g.pitch_count, 1};
  for (int i = 0; i < 4; ++i)
    if (n[i] < 1 || lo[i] < 3 || lo[i] + n[i] > vocab) return "a grammar range is empty or outside [3, vocab)";
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (lo[i] < lo[j] + n[j] && lo[j] < lo[i] + n[i]) return "grammar ranges overlap";
  if (g.max_steps < 1 || g.max_steps > g.shift_count - 1) return "max_steps must be in [1, shift_count - 1]";
  return nullptr;
}
// the one host-side check of a note grammar descriptor against a vocabulary: nullptr, or what is wrong with it
inline const char* bad_note_grammar(const mt3_note_grammar& n, int vocab) {
  if (const char* bad = bad_token_grammar(n.g, vocab)) return bad;
  if (!n.g.with_ties) return "the note rule needs a tie section (with_ties == 1)";
  if (n.g.program_count > MT3_NOTE_MAX_PROGRAMS || n.g.pitch_count > MT3_NOTE_MAX_PITCHES)
    return "the note rule keeps at most 128 programs and 128 pitches";
  const long long lo[6] = {n.velocity_first, n.drum_first, n.g.shift_first, n.g.program_first, n.g.pitch_first, n.g.tie_id};
  const long long c[6] = {n.velocity_count, n.drum_count, n.g.shift_count, n.g.program_count, n.g.pitch_count, 1};
  for (int i = 0; i < 2; ++i)
    if (c[i] < 1 || lo[i] < 3 || lo[i] + c[i] > vocab) return "a velocity or drum range is empty or outside [3, vocab)";
  for (int i = 0; i < 2; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (lo[i] < lo[j] + c[j] && lo[j] < lo[i] + c[i]) return "a velocity or drum range overlaps another range";
  return nullptr;
}
// grammar_room's count for the note rule: the ids of the worst state after the tie section, which now has no pitch and no
// drum id either (velocity zero, nothing held); the tie-section state loses nothing (nothing declared yet)
inline int note_room_after(const mt3_note_grammar& n, const uint32_t* h_mask, int vocab) {
  const int32_t s_after = static_cast<int32_t>(MT3_GRAMMAR_PREV_SHIFT), note = static_cast<int32_t>(MT3_NOTE_VELOCITY_ZERO);
  const uint32_t row[MT3_NOTE_ROW_WORDS] = {0, 0, 0, 0};
  int b = 0;
  for (int i = 0; i < vocab; ++i) {
    if (h_mask && !((h_mask[i >> 5] >> (i & 31)) & 1u)) continue;
    b += mt3g_allowed(&n.g, s_after, i) && mt3n_allowed_extra(&n, s_after, note, row, i);
  }
  return b;
}
// the ids a free pick may take under grammar `g` and mask `h_mask` (nullptr: none) in the two states that bound every
// other: *in_tie = the tie-section state, *after = the worst state after it (no shift, no tie)
inline void grammar_room(const mt3_token_grammar& g, const uint32_t* h_mask, int vocab, int* in_tie, int* after) {
  const int32_t s_tie = static_cast<int32_t>(MT3_GRAMMAR_TIE_SECTION), s_after = static_cast<int32_t>(MT3_GRAMMAR_PREV_SHIFT);
  int a = 0, b = 0;
  for (int i = 0; i < vocab; ++i) {
    if (h_mask && !((h_mask[i >> 5] >> (i & 31)) & 1u)) continue;
    a += mt3g_allowed(&g, s_tie, i);
    b += mt3g_allowed(&g, s_after, i);
  }
  *in_tie = a;
  *after = b;
}
// in.y[b] = table[tok[b]] + pos[step[b]] for b < B, in every form `in` holds
int launch_embed(const InputRow& in, const int* tok, const int* step, int B, hipStream_t s);
// per-row state of the beam-1 search (t5x beam_search, num_decodes = 1): f = [live_logp | best finished
// score], the second array `rows` floats after the first; len = prefix length of the best finished
// hypothesis or -1; cfg[0] = brevity_penalty(max_len + 1), cfg[1 + n] = brevity_penalty(n) (device memory)
// t5x decoding.brevity_penalty(alpha = 0.6, length): ((5 + length) / 6) ^ alpha
inline float brevity_penalty(int length) { return static_cast<float>(std::pow((5.0 + length) / 6.0, 0.6)); }
// host image of BeamState::cfg / BeamKArgs::bp for id rows of L positions: [0] = 0, the bound of a call (set per call to
// brevity_penalty(num_steps + 1)), [1 + n] = brevity_penalty(n), n = 0 .. L + 1
inline std::vector<float> brevity_table(int L) {
  std::vector<float> bp(static_cast<size_t>(L) + 3, 0.f);
  for (int n = 0; n <= L + 1; ++n) bp[1 + n] = brevity_penalty(n);
  return bp;
}
struct BeamState {
  float* f;
  int* len;
  const float* cfg;
  int rows;
  // a copy of `len` indexed by the ROW a slot decodes (what the finalisation reads once the loop is over: under row
  // retirement the slot-indexed state of a finished row is gone by then); the base of the step's rows, or -- with a
  // slot map -- of the whole batch
  int* len_row;
};
// Row retirement and the synthetic EOS schedule of one step (all nullptr / 0: the canonical schedule).
//   retire  : a block whose slot is already done returns at once (its ids stay 0, its position counter stops)
//   slot_row: [B] slot -> row of `ids` / `eos_at` (nullptr: identity); with it `ids` is the UN-offset base of the batch
//   eos_at  : [rows] bench / test hook (mt3_debug_engine_set_eos_schedule): row r's distribution at step eos_at[r] - 1
//             is replaced by a point mass on EOS -- greedy emits EOS there, the beam-1 search finishes prefix + EOS with
//             log-prob 0 and closes (its live hypothesis drops to -inf)
//   slot_seg: [B] in-flight batching (mt3_engine_transcribe): the SEGMENT a slot is decoding -- `eos_at` is then indexed by
//             segment, not by row (a cache row serves many segments in turn)
//   max_len : > 0: a slot whose position counter reaches max_len is finished whether or not it emitted EOS (a refilled slot
//             starts at position 0 at an arbitrary step of its group's loop, so the loop bound cannot do it)
struct StepRetire {
  int retire;
  const int* slot_row;
  const int* eos_at;
  const int* slot_seg;
  int max_len;
};
// token pick + bookkeeping for one decode step (see decode_ops.hip): slot b < B picks from logits[b], writes
// ids[row * ids_stride + t] and the next step's input row
struct ArgmaxStepArgs {
  float* logits;        // [B][vocab]
  int vocab;
  int* ids;
  int ids_stride;
  SlotState st;         // (slot_row / slot_seg are read through `rt`, which says whether they are in use)
  InputRow in;
  BeamState beam;       // f == nullptr: greedy
  const int* forced;    // greedy only: teacher forcing, the next input token is forced[b * forced_stride + t]
  int forced_stride;
  LogitScale ls;
  StepRetire rt;
  int B;
  TokenMask tm;         // rows == nullptr: unconstrained
  TokenPrompt tp;       // rows == nullptr: none
  TokenGrammar gr;      // on == 0: none; else st.gram holds the slots' states
  TokenNotes nt;        // on == 0: none; else gr.g == nt.n.g and st.note / nrow / held hold the slots' note states
};
int launch_argmax_step(const ArgmaxStepArgs& a, hipStream_t s);
// Temperature sampling (mt3_engine_set_sampling; the rule and the noise: include/mt3_hip.h, mt3s_*): the greedy step `a`
// (no beam state, no teacher forcing) with the pick of a free position drawn by sample_step_kernel, which takes
// argmax_step_kernel's place in the step.  The parameters are read from DEVICE memory, so that a captured step serves
// every seed.  The noise stream of a slot is that of its segment: the entry of `stream`, a per-segment table of one
// uint64 per row indexed as the masks are, or -- no table -- seg0 + the segment index the masks would be indexed by.
// vocab <= MT3_SAMPLING_MAX_VOCAB: the row lives in registers, eight values per thread.  The Philox key of a slot is the
// parameters' seed, or -- `seed`, a second table of one uint64 per row indexed exactly as `stream` is
// (mt3_engine_set_sampling_seeds) -- its segment's entry: several draws of one segment can then sit in one job.
using SampleStream = SegTable<uint64_t>;
struct SampleStepArgs {
  ArgmaxStepArgs a;
  const mt3_sampling* params;   // device
  SampleStream stream;          // rows == nullptr: stream = seg0 + segment
  int seg0;
  SampleStream seed;            // rows == nullptr: the key is params->seed (the instantiations that do not mention it run)
};
int launch_sample_step(const SampleStepArgs& a, hipStream_t s);
// Compaction of the live slots of one row group to the front of the group (row retirement): the per-slot state that
// lives from one step to the next -- the next step's input row in its three forms, layer 0's projected row, position
// counter, current token, beam-search state, the slot -> row map -- moves from slot perm[i] to slot i (i < n_live) by
// way of a scratch copy; slots [n_live, rows) are marked done.  All pointers are those of the group's first slot.
constexpr int kCompactInts = 6 + MT3_NOTE_ROW_WORDS;
struct CompactArgs {
  SlotState st;         // slot_seg == nullptr: no in-flight batching (a dropped slot decodes nothing: -1)
  InputRow in;          // y / y_ct / y_ss / rp.q_out (each nullptr: not in use), dim, rp.q_n
  BeamState beam;       // f == nullptr: greedy (f and len travel with the slot)
  // scratch of the same shapes (slot-indexed from the group's first slot as well)
  float* s_y;
  void* s_y_ct;
  float* s_y_ss;
  float* s_qkvf;
  int* s_int;           // [rows][kCompactInts]: slot_row, step, cur_tok, beam_len, grammar state, note, the row copy
  uint32_t* s_held;     // [rows][st.held_words]: the staged copy of the note tables (st.note != nullptr)
  float* s_beam;        // [rows][2]
  int* s_seg;           // [rows]
  int* perm;            // [rows + 1]: perm[i] = source slot of new slot i; perm[rows] = n_live
  int rows;             // slots of the group in use before the compaction
};
int launch_compact(const CompactArgs& c, hipStream_t s);
// Refill of finished slots (in-flight batching, mt3_engine_transcribe): at a poll of a row group's loop every FINISHED
// slot of the group hands its id row to the caller's output (row = the segment it decoded; the beam-1 finalisation of
// that row applied on the way) and the first `n_new` of them, in ascending slot order, restart at position 0 on segments
// first_seg, first_seg + 1, ...: BOS input row in its three forms, layer 0's projected row, counters, beam state, a
// zeroed id row, and the segment's cross-attention K/V copied from the staging chunk an encoder pass left them in into
// the cache rows the slot owns (the self-attention cache needs nothing: what lies past a row's position is discarded by
// position).  The others decode nothing from then on (slot_seg = -1) until a later refill.  All slot-indexed pointers are
// those of the group's first slot; ids / beam_len_row / the caches are batch bases (reached through slot_row).
constexpr int kRefillMaxLayers = 16;
// The staged cross-attention K/V of a run of segments and the caches they are copied into: per decoder layer, staging
// chunk [2][src_batch][row_bytes] (the run starts at entry src_entry0) -> cache [2][dst_batch][row_bytes]; with e4m3
// caches also the scale rows [src_batch][sc_bytes] -> [dst_batch][sc_bytes] (src_sc[l] == nullptr: none).
// per > 1 (mt3_engine_transcribe_draws): `per` consecutive restarted slots share one staged entry -- src_batch and
// src_entry0 count DRAWS, the i-th restarted slot copies entry (src_entry0 + i) / per and the chunk's planes are
// src_batch / per entries apart (src_batch % per == 0; the run may start in the middle of an entry's draws).  per = 1:
// one entry per slot, the copy it always was.
struct StagedCross {
  int n_layers;
  const char* src[kRefillMaxLayers];
  char* dst[kRefillMaxLayers];
  const char* src_sc[kRefillMaxLayers];
  char* dst_sc[kRefillMaxLayers];
  int src_batch, src_entry0, dst_batch;
  size_t row_bytes, sc_bytes;
  int per;
};
struct RefillArgs {
  SlotState st;         // n_done is decremented by the number of slots refilled
  InputRow in;          // the BOS row is in.table[0] + in.pos[0]
  BeamState beam;       // f == nullptr: greedy; len_row is the batch base
  int* ids;             // engine id rows [max_batch][ids_stride] (batch base)
  int ids_stride;
  int* out_ids;         // caller's [n_segments][ids_stride]
  int* plan;            // [rows + 1] scratch: plan[i] = i-th finished slot (ascending), plan[rows] = how many
  int rows;             // slots of the group in use
  int n_new;            // segments handed out by this call (<= finished slots)
  int first_seg;
  StagedCross x;        // where their cross-attention K/V come from and go to (read when n_new > 0)
  int gram0;            // the grammar state a restarted slot begins in (st.gram != nullptr)
};
int launch_refill(const RefillArgs& a, hipStream_t s);
// ---- k-beam search (mt3_engine_decode_beams; the rule is stated in include/mt3_hip.h)
// Slots b*k .. b*k + k - 1 hold the k live beams of batch element b.  All slot-indexed pointers are those of the step's
// first slot; `hist_*` are [L][hist_stride] with the step's first slot as column 0.
constexpr int kBeamMaxK = 8;
constexpr float kBeamNegInf = -1.0e7f;       // t5x decoding.NEG_INF
struct BeamKArgs {
  float* logits;
  int vocab, k, elems;
  SlotState st;         // slot_row is rewritten (a beam takes over its parent's row); done is set for all k slots once the
                        // element is retired, n_done then grows by k
  InputRow in;          // the next step's input rows
  float* live;          // [slots] running log-prob of each live beam, best first within an element
  float* fin_score;     // [slots] the element's k finished entries, best first (kBeamNegInf: unfilled)
  int* fin_step;        // [slots] step of the entry's EOS (-1: unfilled)
  int* fin_beam;        // [slots] beam (0 .. k-1) whose prefix the EOS ends
  int* hist_par;        // [L][hist_stride] parent beam of the new beam in each slot
  int* hist_tok;        // [L][hist_stride] its token
  int hist_stride;
  int* fork_src;        // [slots] row to copy positions [0, t] from into the slot's new row (-1: no copy)
  int* fork_count;      // running count of forks (copies)
  const float* bp;      // BeamState::cfg
  // > 0 (mt3_engine_transcribe_beams): an element whose position counter reaches max_len is closed whether or not its
  // search has -- its k slots are marked done and counted, its live and finished sets stay as the step left them (in
  // mt3_engine_decode_beams the host loop's bound does that: it passes 0)
  int max_len;
};
int launch_beam_step(const BeamKArgs& a, const LogitScale& ls, const TokenMask& tm, const TokenPrompt& tp,
                     const TokenGrammar& gr, const TokenNotes& nt, hipStream_t s);
// copies positions [0, step[slot]) of row fork_src[slot] into row slot_row[slot] of every layer's self-attention K/V
// (and e4m3 scale rows), for every slot that forked this step; the grid covers every slot x layer x head
struct BeamReorderArgs {
  int n_layers, H, cap, kv_esize, slots;
  char* k[kRefillMaxLayers];
  char* v[kRefillMaxLayers];
  float2* scale[kRefillMaxLayers];   // nullptr: no e4m3 side array
  const int* fork_src;
  const int* slot_row;
  const int* step;
  const int* done;
};
int launch_beam_reorder(const BeamReorderArgs& a, hipStream_t s);
// state of a new search: live = [0, NEG_INF, ...] per element, nothing finished
int launch_beam_init(float* live, float* fin_score, int* fin_step, int* fin_beam, int slots, int k, hipStream_t s);
// backtracks the result of every element: ids [elems][L] (the best decode), all_ids [elems][k][L] and scores
// [elems][k] in increasing order of score (either may be nullptr)
int launch_beam_finalize(const BeamKArgs& a, int L, int num_steps, int* ids, int* all_ids, float* scores, hipStream_t s);
// Refill of finished beam ELEMENTS (in-flight batching of the k-beam search, mt3_engine_transcribe_beams): the beam
// counterpart of launch_refill, three launches on the group's stream at a poll of the group's loop.
//   plan   refill_plan_kernel over elements (an element is finished when its first slot is done): plan[i] = i-th finished
//          element, plan[elems] = how many; the group's counter of finished slots drops by k per restarted element
//   cross  refill_cross_kernel with unit = k: the cross-attention K/V (and e4m3 scale rows) of segment first_seg + i from
//          the staging chunk into EACH of the k cache rows slot_row[s0 .. s0 + k) of element plan[i]
//   elem   block i: the k decodes of element plan[i] are walked back from the history (beam_finalize_kernel's walk, on a
//          copy of the element's history columns in LDS) straight into the caller's rows of the segment it held; then,
//          i < n_new: the element restarts on segment first_seg + i (live = [0, NEG_INF, ...], nothing finished, position 0,
//          BOS input rows in their three forms and layer 0's projected rows for all k slots); the others keep done = 1 and
//          get slot_seg = -1 -- they decode nothing until a later refill.
// b: the group's beam state (pointers of the group's first slot, b.elems = elements of the group); the self-attention
// caches need nothing: an element's slot_row entries stay a permutation of its own k rows.
struct BeamRefillArgs {
  BeamKArgs b;          // b.st.slot_seg: the segment an element is decoding, in all k of its slots (-1: none)
  int* plan;            // [elems + 1] scratch
  int L, num_steps;     // id row length; steps per segment of the job
  int* out_ids;         // caller's [n_segments][L]
  int* out_all;         // caller's [n_segments][k][L] or nullptr
  float* out_scores;    // caller's [n_segments][k] or nullptr
  int n_new, first_seg;
  StagedCross x;        // as RefillArgs::x
  int gram0;            // as RefillArgs::gram0 (b.st.gram != nullptr)
};
int launch_beam_refill(const BeamRefillArgs& a, hipStream_t s);
// start of an mt3_engine_transcribe_beams job: every slot finished and without a segment (the first refill starts the
// elements), slot i on cache row i, no fork pending; n_done[g] = group_slots[g] for the `groups` row groups
struct GroupSlots {
  int n[4];
};
int launch_beam_stream_init(int* done, int* slot_seg, int* fork_src, int* slot_row, int* n_done, int slots, int groups,
                            const GroupSlots& group_slots, hipStream_t s);
int launch_iota(int* dst, int n, hipStream_t s);
int launch_set_float(float* dst, float v, hipStream_t s);
int launch_beam1_finalize(int* ids, int L, const int* beam_len, int B, hipStream_t s);
int launch_ids_to_tokens(const int* ids, int B, int L, int num_regular, int* out, hipStream_t s);

// ---- teacher-forced scoring (mt3_engine_score, score.hip).  A chunk holds `rows` = segments * Lp rows, row = seg * Lp + t;
// caller arrays are [batch][length], the chunk's first segment is seg0
struct ScoreEmbedArgs {
  const float* table;     // token embedding [vocab][dim]
  const float* pos;       // position table
  const int* targets;     // caller [batch][length]
  const int* dec_in;      // caller [batch][length] or nullptr: shift_right(targets), BOS = 0
  int* tgt_pad;           // [rows] targets, 0 past `length`
  float* y;               // [rows][dim] f32 decoder input rows
  int rows, Lp, length, seg0, dim, vocab;
};
int launch_score_embed(const ScoreEmbedArgs& a, hipStream_t s);
struct ScoreAttnArgs {
  const void* q;          // [B][Lq] query rows, row stride q_stride elements; head h at +h*64
  int q_stride;
  const void* k;          // key j of (batch b, head h) at k + b*kv_bstride + h*kv_hstride + j*kv_stride
  const void* v;
  int kv_stride;
  long long kv_bstride, kv_hstride;
  const int* key_tgt;     // [B][Lq] (causal only): key j is visible iff key_tgt[b][j] != 0 (nullptr: every key)
  void* out;              // [B][Lq] rows of out_stride elements; head h at +h*64
  int out_stride;
  int B, H, Lq, n_keys;   // Lq % 64 == 0; causal: n_keys = Lq; cross: n_keys = T (a multiple of 64)
  int causal;
  // rows that share one K / V row (mt3_engine_score_candidates): batch b reads K / V batch (b + kv_b0) / kv_share
  int kv_share = 1, kv_b0 = 0;
};
int launch_score_attention(int dtype, const ScoreAttnArgs& a, hipStream_t s);
struct ScoreReduceArgs {
  const float* logits;    // [rows][vocab]
  const int* tgt_pad;     // [rows]
  const float* weights;   // caller [batch][length] or nullptr (1)
  float* tok_pad;         // [rows] token scores of the chunk
  float* token_scores;    // caller [batch][length] or nullptr
  float* seq_scores;      // caller [batch]
  int rows, Lp, length, seg0, vocab;
};
int launch_score_reduce(const ScoreReduceArgs& a, hipStream_t s);
// launch_score_reduce with the arg-max of every row next to its token score (score_token_stats_kernel, then the same
// score_sum_kernel): token scores with launch_score_reduce's bits
struct ScoreStatsArgs {
  ScoreReduceArgs r;
  int* top1_ids;          // caller [batch][length] or nullptr: arg-max of the row (lowest id on ties), 0 where target == 0
  float* top1_scores;     // caller [batch][length] or nullptr: log_softmax(logits)[top1], 0 where target == 0
};
int launch_score_stats(const ScoreStatsArgs& a, hipStream_t s);
// f32 [n] -> three bf16 planes (gemm_x6_kernel's weight operand)
int launch_planes(const float* w, void* hi, void* mid, void* lo, size_t n, hipStream_t s);

}  // namespace mt3k
#endif  // MT3_KERNELS_H_
