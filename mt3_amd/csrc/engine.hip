// The MT3 encoder-decoder engine behind mt3_engine_* (include/mt3_hip.h).
//
// Replaces network.Transformer (mt3/network.py:265-409) as t5x's predict_batch_with_aux drives it
// (mt3/models.py:121-152): `encode` once, then a cached single-token `decode` per step.
//
// MI355X design notes
//   * weights live on the device in the layouts the kernels want, built once at finalize():
//       - every DenseGeneral kernel [in,out] (layers.py:373-418) is stored output-major Wt[out][in];
//       - Q|K|V (layers.py:238-240) are fused into one [3*H*64][emb] matrix, wi_0|wi_1
//         (layers.py:460-468) are interleaved in 16-row groups for the GEGLU epilogue;
//       - every pre-norm scale (network.py:54-56,71,104-106,126-128,142,244) is folded into the
//         rows of the matrix that consumes the normalised activations (the rsqrt part is computed
//         inside that GEMM), so the only standalone norm left is `encoder_norm`.
//   * cross-attention K/V (layers.py:239-240 via network.py:129-135) are computed ONCE per encode
//     for all decoder layers, head-major for the streaming decode kernel; the reference recomputes
//     them inside every decode step unless XLA hoists them.
//   * the self-attention cache is [B][H][L][64] written in place at position t (the reference
//     rewrites the whole [B,H,64,L] cache per step: layers.py:272-292).
//   * one decode step = 8 x 8 + 2 kernels with per-row position counters in DEVICE memory (the argmax
//     kernel also writes the next step's embedding row), captured once per
//     batch size into a hipGraph and replayed L times.  The batch can be dealt to `decode_chains`
//     independent row groups, one graph BRANCH each (fork/join capture over several streams), so that one
//     chain's latency-bound GEMMs run beside another chain's HBM-bound K/V streaming; it paid +6 % with the
//     first kernels and nothing with the current ones, so the default is one chain.
//   * host side, every decoding entry point is the same three pieces: a start on the caller's stream (reset_slots,
//     embed_bos, reset_beam1_state), one GroupJob dealt to the row groups' worker threads (post_groups / run_one_group
//     around run_group, or around run_group_stream for the in-flight batched jobs, which run_stream_job drives), and
//     a join (decode_finish, or run_stream_job's own).
//   * sized for 288 GB HBM: all workspaces for max_batch are allocated up front
//     (B=256: ~3.3 GB KV cache + ~0.9 GB cross K/V + ~0.5 GB activations in bf16).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "feed.h"
#include "kernels.h"
#include "mx8.h"
#include "mt3_hip.h"
#include "mt3_hip_debug.h"

namespace {

constexpr int kMaxPos = 2048;   // FixedEmbed.max_length, layers.py:565
constexpr int kMaxChains = 8;
constexpr int kForksPinned = 15;  // h_pinned[15]: fork count of the last beam decode (h_pinned[0 .. kMaxGroups): polls)

uint16_t f32_to_bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40);   // NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                                       // RNE
  return static_cast<uint16_t>(u >> 16);
}

struct HostWeight {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

// One weight matrix on the device: output-major [N][K] in the compute type, and the other forms of the same numbers
// that some launches read instead (made by upload_dense and ensure_score_planes)
struct Dense {
  void* w = nullptr;         // [N][K] compute type (a qkv-fold layer's `wi` goes on past row N, see LayerDev)
  int N = 0, K = 0;
  // f32 engine, encoder-sized launches (gemm_x6_kernel): three bf16 planes (hi / mid / lo) [N][K].  Encoder matrices and
  // wkv_x get them at finalize, the decoder's other matrices with the first mt3_engine_score call (the decode step never
  // reads them)
  void* p[3] = {};
  // MXFP8 dense path (dense_dtype MT3_FP8_E4M3; encoder matrices and wkv_x): e4m3 bytes [N][K] + E8M0 block scales [N][K / 32]
  uint8_t *q = nullptr, *sc = nullptr;
};
constexpr int kFormPlanes = 1, kFormMx8 = 2;     // upload_dense: the forms a matrix gets beside the compute type

struct LayerDev {
  Dense wqkv;                // [3HD][emb]
  Dense wo;                  // [emb][HD]
  Dense wq_x;                // decoder cross query [HD][emb]
  Dense wkv_x;               // decoder cross key|value [2HD][emb]
  Dense wo_x;                // decoder cross out [emb][HD]
  // q-fold (bf16 decode): the cross-attention q-projection rides in the two neighbouring launches
  Dense wqkv_ext;            // decoder [3HD + HD][emb]: wqkv rows, then the cross query rows (pre_cross norm scale folded)
  Dense wo_ext;              // decoder [emb + HD][HD]: self out-projection rows, then (Wo . (s2 * Wq_x))^T
  // qkv-fold (round 3): the NEXT layer's q | k | v | cross-q projections ride in this layer's GEGLU and MLP
  // out-projection launches.  Wext = the next layer's scaled [q | k | v | cross-q] (last layer: the scaled logits matrix)
  Dense w_fold;              // decoder [emb + nx][mlp]: rows < emb = Wo_mlp^T; rows >= emb = (Wo_mlp . Wext)^T
  Dense wi;                  // [2*mlp][emb] interleaved gate/linear.  qkv-fold decoder layers: the buffer goes on with
                             // Wext^T [nx][emb] and zero rows up to a multiple of 64, which only the decode step's
                             // GEGLU launch reads (it states its own N)
  Dense wo_mlp;              // [emb][mlp]
  void* self_k = nullptr;    // decoder [Bm][H][L][64]
  void* self_v = nullptr;
  void* cross_kv = nullptr;  // decoder [2][B][H][T][64]
  // fp8 (e4m3) K/V caches only: {k_scale, v_scale} per cached row
  float2* self_scale = nullptr;    // [Bm][H][L]
  float2* cross_scale = nullptr;   // [B][H][T]
};

// Variant bits of one decode step (part of the key of its captured graph, GroupGraph): 1 / 2 = mt3_debug_engine_decode's
// skipped kernels (no self-attention / no cross-attention: differential profiling only),
// 4 = beam-1 token selection, 8 = teacher forcing, 16 = row retirement (finished slots cost nothing, the slot map is
// in use), 32 = the synthetic EOS schedule (mt3_debug_engine_set_eos_schedule)
// 64 = in-flight batching (mt3_engine_transcribe: finished slots restart on new segments, the slot -> segment map is in use)
// 128 = token masks (mt3_engine_set_token_masks): the step ends with the MASKED token / beam kernel, so masked and unmasked
// steps never share a captured graph
// 256 = prompts (mt3_engine_set_prompts): the step ends with the PROMPT token / beam kernel, so prompted and unprompted steps
// never share a captured graph
// 512 = the event grammar (mt3_engine_set_token_grammar): the step ends with the GRAMMAR token / beam kernel, so steps with
// a grammar never share a captured graph with steps without one
// 1024 = temperature sampling (mt3_engine_set_sampling): the step ends with sample_step_kernel in the token kernel's place,
// so sampled and unsampled steps never share a captured graph
// 2048 = the note rule (mt3_engine_set_note_grammar; always with 512): the step ends with the NOTES token / sample / beam
// kernel, so steps with the note rule never share a captured graph with other steps
constexpr int kVarBeam = 4, kVarForced = 8, kVarRetire = 16, kVarEos = 32, kVarStream = 64, kVarMask = 128,
              kVarPrompt = 256, kVarGrammar = 512, kVarSample = 1024, kVarNotes = 2048;
// not a rule of the step itself: set in GroupRun::variant when the decode runs as SEVERAL row groups, so that a step
// knows it runs beside other groups' launches (GemmArgs::concurrent) and the step-graph cache keeps such steps apart
// from a lone stream's steps of the same shape
constexpr int kVarBeside = 4096;
// a step of mt3_engine_decode_beams (always with kVarRetire's slot -> row map); the number of beams rides in bits
// kVarBeamsShift .. +3 so that the step-graph cache keeps different k apart
constexpr int kVarBeams = 8192, kVarBeamsShift = 14;
constexpr int kMaxGroups = 4;
// staging ring of mt3_engine_transcribe: cross-attention K/V of segments that wait for a slot, kStageChunks chunks of up
// to kStageChunkCap segments each (one encoder pass per chunk)
constexpr int kStageChunks = mt3feed::kStageChunks, kStageChunkCap = 64, kStageMinBatch = 8;
constexpr int kStreamPollSteps = 4;     // steps between two refill polls of a row group.  Drained polls, f32, 10,000 ragged segments:
                                        // 32 / 16 / 8 steps -> 2395 / 2417 / 2423 audio-s/s at 1250 slots, 1861 / 1889 / 1905 at 256
                                        // (a finished slot idles half an interval on average, a drained poll costs a bubble of
                                        // ~50 us, more when the host sleeps); the pipelined poll has no bubble and reacts one
                                        // interval later: a slot idles 1.5 intervals on average
constexpr int kThrottleWindow = 16;     // steps per window of the sleeping enqueue throttle (mt3_engine::wait_ev)

// One persistent host thread per row group (created with the first decode that needs it, joined at destroy): a
// decode call hands each group's loop to one of them instead of spawning threads per call, and with
// MT3_DECODE_ASYNC the caller gets its own thread back while they run.
struct Worker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, quit = false;
};

// a captured decode step of rows [row0, row0 + rows) of a `batch`-row decode, dealt to `chains` parallel branches
struct GroupGraph {
  int variant, batch, row0, rows, slot, max_len, chains;
  hipGraph_t graph;
  hipGraphExec_t exec;
};

// The job in flight: what every group of it leaves behind (run_one_group), and what mt3_engine_decode left for
// mt3_engine_decode_wait (decode_finish)
struct PendingDecode {
  bool active = false;
  int posted = 0;               // workers that hold a job of this decode
  int groups = 1;
  int rcs[kMaxGroups] = {};
  int ran[kMaxGroups] = {};
  bool used_graph[kMaxGroups] = {};
  std::string errs[kMaxGroups];
  // decode_finish: where the ids go
  bool beam1 = false;
  int batch = 0;
  int32_t* d_ids = nullptr;
  hipStream_t s = nullptr;
  // ... and what only the k-beam finalisation reads (mt3_engine_decode_beams)
  int beams = 0;                // k (0: mt3_engine_decode)
  int num_steps = 0;
  int32_t* d_all_ids = nullptr;
  float* d_scores = nullptr;
};

// A per-segment table as the engine owns it (set_seg_table; the kernels' view of it: seg_view / mt3k::SegTable).  The
// step graphs of its kVar* bit hold the addresses of both arrays, the stride and whether the index is in use.
template <typename T>
struct SegTableHost {
  T* rows = nullptr;             // [rows_cap] elements: n rows of `stride`
  int* seg = nullptr;            // [seg_cap] row index per row / element / segment of a job
  size_t rows_cap = 0, seg_cap = 0;
  int n = 0;                     // rows set (0: the table is not in use)
  int stride = 0;                // elements of T per row
  bool seg_on = false;           // a per-segment index is set (false: row 0 for every segment)
  std::vector<int> seg_host;     // host copy of the per-segment index
  std::vector<int> stat;         // host, per row: what the job checks read (fits)
  std::vector<T> rows_host;      // host copy of the rows (the grammar's check of its intersection with the masks)
};

}  // namespace

struct mt3_engine {
  mt3_engine_config cfg{};
  std::map<std::string, HostWeight> raw;
  std::vector<void*> allocs;
  int64_t device_bytes = 0;
  bool finalized = false;
  int esize = 2;
  int kv_esize = 2;              // bytes per cached K/V element: esize, or 1 with the fp8 (e4m3) caches
  bool kv_fp8 = false;
  void* cross_stage = nullptr;   // fp8 caches: bf16 [2][Bm][H][T][64] landing buffer of the cross-K/V GEMM (one layer)
  // MXFP8 encoder (gemm_mx8.hip): every GEMM operand of the encoder as e4m3 + E8M0 block scales
  bool dense_fp8 = false;
  uint8_t *x_q = nullptr, *x_sc = nullptr;         // residual rows [M][emb], written by the RESID epilogues
  uint8_t *attn_q = nullptr, *attn_sc = nullptr;   // attention output [M][HD]
  uint8_t *h_q = nullptr, *h_sc = nullptr;         // GEGLU output [M][mlp], written by the GEGLU epilogue
  uint8_t *enc_q = nullptr, *enc_sc = nullptr;     // normed encoder output [M][emb] (A of the cross-K/V projections)

  Dense enc_in;                  // [emb][input_depth]
  bool x6 = false;               // f32 engine: the encoder's dense layers multiply on the bf16 pipes (three planes per operand)
  float* enc_norm = nullptr;     // [emb] f32
  float* embedding = nullptr;    // [V][emb] f32
  Dense logits_w;                // [V][emb] (decoder_norm folded)
  float* pos_table = nullptr;    // [kMaxPos][emb] f32
  std::vector<LayerDev> enc, dec;

  // encoder workspaces
  float* x = nullptr;
  // bf16 path: the encoder's residual rows also travel split (bf16 copy + partial sums of squares), so that every
  // encoder GEMM reads bf16 operands through the LDS-DMA staged tile
  void* x_ct = nullptr;          // [max_batch * T][emb] bf16
  float* x_ss = nullptr;         // [max_batch * T][emb / 16]
  bool x_split = false;
  void* qkv = nullptr;
  void* attn = nullptr;
  void* hbuf = nullptr;
  void* enc_out = nullptr;
  // decode workspaces
  float* y = nullptr;
  // bf16 decode path: compute-type copy of the residual rows + their per-16-column sums of squares, kept up to
  // date by every producer of `y` (embed / argmax / the RESID GEMMs), read by the RMSNorm-fused GEMMs
  void* y_ct = nullptr;          // [max_batch][emb] bf16
  float* y_ss = nullptr;         // [max_batch][emb/16]
  bool y_split = false;
  // q-fold: y_new . Wq' = y_old . Wq' + attn . (Wo . Wq') by linearity, so the first term is 384 extra output columns
  // of the QKV launch (same A operand), the second 384 extra columns of the self out-projection launch (same A
  // operand), and the row's 1/rms is applied by the cross-attention kernel from the partial sums the out-projection's
  // RESID epilogue leaves anyway: 8 launches per step fewer
  float* qf = nullptr;           // [max_batch][HD] f32, unnormalised cross-attention query
  bool q_fold = false;
  // qkv-fold: y_in(l+1) . W = y2(l) . W + h(l) . (Wo_mlp . W) by the same linearity, W = the next layer's
  // [q | k | v | cross-q].  The first term needs only the row the GEGLU launch reads anyway: it is that launch's side
  // product (4HD extra output columns, kEpiGegluP, stored to qkvf); the second rides as 4HD extra output columns in
  // layer l's MLP out-projection launch and is added to it (kEpiResidQ).  Layer 0's row comes from two table rows
  // (embedding . W, position table . W) written by the kernel that creates the decoder input row.  The self-attention
  // kernel applies 1/rms and rounds q / k / v itself.  8 more launches per step gone.
  bool qkv_fold = false;
  float* qkvf = nullptr;         // [max_batch][4HD] f32 unnormalised q | k | v | cross-q of the current layer's input row
  float* ew0 = nullptr;          // [vocab][4HD] f32: embedding . Wext(layer 0)
  float* pw0 = nullptr;          // [kMaxPos][4HD] f32: position table . Wext(layer 0)
  void* qkv_d = nullptr;
  void* attn_d = nullptr;
  void* q_d = nullptr;
  void* h_d = nullptr;
  float* logits = nullptr;
  int* ids = nullptr;
  int* cur_tok = nullptr;
  int* done = nullptr;
  int* step = nullptr;
  int* n_done = nullptr;
  int* h_pinned = nullptr;
  int* forced = nullptr;         // [max_batch][L] teacher-forcing tokens of the current mt3_engine_decode_forced call
  std::atomic<int> graph_fallbacks{0};   // decode loops whose step graph could not be captured (ran as direct launches)
  int last_used_graph = 0;
  // Row retirement (MT3_DECODE_EARLY_EXIT): per-row-of-the-batch state lives in SLOTS; slot_row maps a slot to the row
  // whose caches / ids it works on.  Live slots are compacted to the front of their row group at the early-exit poll
  // (launch_compact), so attention grids and the GEMMs' M shrink with the live set while the caches stay in place.
  int* slot_row = nullptr;       // [max_batch]
  int* eos_at = nullptr;         // [eos_cap] synthetic EOS schedule (mt3_debug_engine_set_eos_schedule): per row, or -- in
                                 // mt3_engine_transcribe -- per segment
  int eos_cap = 0;
  bool eos_on = false;
  SegTableHost<uint32_t> tm;     // constrained decoding (mt3_engine_set_token_masks, kVarMask): masks of ceil(vocab / 32)
                                 // words; stat = the allowed tokens of each
  SegTableHost<int> tp;          // prompted decoding (mt3_engine_set_prompts, kVarPrompt): 0-padded id rows; stat = the
                                 // length of each
  mt3k::TokenGrammar gr{};       // well-formed decoding (mt3_engine_set_token_grammar, kVarGrammar): the descriptor travels by
                                 // value in the step's kernel arguments (a graph that captured another one is dropped)
  bool gr_seen = false;          // a descriptor has been set before (step graphs may hold it)
  mt3k::TokenNotes nt{};         // note-consistent decoding (mt3_engine_set_note_grammar, kVarNotes).  While on, gr holds nt.n.g
                                 // and is on as well: the note rule's grammar is the engine's grammar
  int* note = nullptr;           // [max_batch] SlotState::note; allocated with the first note grammar, like the three below
  uint32_t* nrow = nullptr;      // [max_batch][MT3_NOTE_ROW_WORDS] SlotState::nrow
  uint32_t* held = nullptr;      // [max_batch][held_words] SlotState::held, held_words = mt3n_table_words(&nt.n)
  uint32_t* cs_held = nullptr;   // [max_batch][held_words] compaction scratch of the tables
  SegTableHost<uint64_t> sstream;  // temperature sampling (mt3_engine_set_sampling, kVarSample): the noise stream of every
                                 // segment, one row of one entry each behind an identity index (not set: the stream of
                                 // segment i is i)
  mt3_sampling* samp = nullptr;  // device copy of the parameters, allocated by the first set: the sampled step graphs hold
                                 // its address, so another seed or temperature needs no new graph
  bool samp_on = false;
  bool samp_seen = false, samp_table = false;   // sampling has been set before, and then with a stream table: the sampled
                                 // step graphs hold whether there is one
  SegTableHost<uint64_t> sseed;  // per-segment Philox keys (mt3_engine_set_sampling_seeds): a table like sstream, indexed as it
                                 // is (not set: every segment's key is the parameters' seed)
  bool seed_table = false;       // the form the sampled step graphs hold (there may be some as soon as sampling has been set,
                                 // captured without a seed table: false is the true state of a new engine)
  int* gram = nullptr;           // [max_batch] per slot: the packed grammar state (SlotState::gram); with a grammar set it
                                 // travels with the slot and is reset with it, without one no launch is handed it
  // In-flight batching (mt3_engine_transcribe): slot_seg maps a slot to the SEGMENT it is decoding (-1: none); a
  // finished slot hands its id row to the caller's output and restarts on the next encoded segment (launch_refill)
  int* slot_seg = nullptr;       // [max_batch]
  int* cs_seg = nullptr;         // compaction scratch
  int* refill_plan = nullptr;    // [max_batch + kMaxChains]: rows + 1 entries per group
  int stream_max_len = 0;        // steps per segment of the transcribe call in flight (a kernel argument of its step graphs)
  int stage_cap = 0;             // segments per staging chunk (0: staging not allocated yet)
  std::vector<void*> stage_kv;       // per decoder layer: [kStageChunks][2][stage_cap][H][T][64] cache elements
  std::vector<float2*> stage_scale;  // e4m3 caches: [kStageChunks][stage_cap][H][T]
  float* cs_y = nullptr;         // compaction scratch: same shapes as y / y_ct / y_ss / qkvf, 4 ints + 2 floats per slot
  void* cs_y_ct = nullptr;
  float* cs_y_ss = nullptr;
  float* cs_qkvf = nullptr;
  int* cs_int = nullptr;
  float* cs_beam = nullptr;
  int* cs_perm = nullptr;        // [max_batch + kMaxChains]: rows + 1 entries per group
  int compactions = 0;           // compactions of the most recent decode (all groups; written at the end of the decode)
  std::atomic<int> compactions_now{0};
  // every captured step graph: one per row group and shape (the single-stream schedule is the group [0, batch))
  std::vector<GroupGraph> group_graphs;
  std::mutex graph_mu;
  Worker* workers[kMaxGroups] = {};
  int device = 0;
  PendingDecode pending;
  float* beam_f = nullptr;       // [2][max_batch]: live log-prob | best finished score (MT3_DECODE_BEAM1)
  int* beam_len = nullptr;       // [max_batch] per slot
  int* beam_len_row = nullptr;   // [max_batch] per row (read by the finalisation)
  float* beam_cfg = nullptr;     // [0] brevity penalty of the loop bound, [1 + n] brevity_penalty(n)
  // k-beam search (mt3_engine_decode_beams; allocated by its first call): slot-indexed state and the per-step history
  float* bk_live = nullptr;      // [max_batch]
  float* bk_fin_score = nullptr; // [max_batch]: k entries per element
  int* bk_fin_step = nullptr;
  int* bk_fin_beam = nullptr;
  int* bk_fork_src = nullptr;    // [max_batch]
  int* bk_forks = nullptr;       // [1] forks of the decode in flight
  int* bk_par = nullptr;         // [L][max_batch]
  int* bk_tok = nullptr;         // [L][max_batch]

  // Row-group decode schedule (round 3): the batch as 2 or 4 row groups (row_groups_for), each on an engine-owned stream
  // with a hardware queue of its own, each driven by its own host thread with direct launches -- one group's HBM-bound
  // attention kernels run beside the other groups' latency-bound GEMMs.  The streams are created with
  // hipExtStreamCreateWithCUMask and a mask of ALL compute units: measured at B = 256 (bf16), two PLAIN streams take
  // 818 ms per 1024-step decode (HIP multiplexes them onto its queue pool and the groups serialise), two masked ones
  // 588 ms whether the masks are disjoint halves, overlap, or cover every CU (one graph-replayed chain: 626 ms).
  hipStream_t part_stream[kMaxGroups] = {};
  hipEvent_t part_begin = nullptr;
  // Sleeping waits (round 5): a group's worker keeps at most two windows of kThrottleWindow steps enqueued ahead of the
  // device and waits for the older one on a BLOCKING-SYNC event -- the thread sleeps until the interrupt instead of
  // spinning in the runtime's queue back-pressure / hipStreamSynchronize (round 4: five cores busy for the length of a
  // decode).  Index kMaxGroups = the caller's stream (single-stream schedule, the encoder passes of transcribe).
  // events the workers NAP-POLL (sleep_until: hipEventQuery between 20..200 us naps; not blocking-sync waits):
  hipEvent_t wait_ev[kMaxGroups + 1][4] = {};     // [0] waits, [1] throttle, [2], [3] the two poll snapshots of transcribe
  bool spin_waits = false;       // MT3_OPT_SPIN_WAITS: round 4's behaviour
  int part_failed = 0;           // partitioned decodes that fell back to the single-stream schedule (stream creation failed)
  int last_groups = 1;           // row groups of the most recent decode

  int cur_batch = 0;             // batch of the last encode
  // step graphs are captured on engine-owned streams (the caller's may be the legacy default stream, which cannot be
  // captured), under graph_mu: a row group's on cap_stream[its slot], a step of several chains on one stream per chain,
  // forked from and joined to cap_stream[0] through cap_event (group_graph)
  hipStream_t cap_stream[8] = {};     // kMaxChains
  hipEvent_t cap_event[8] = {};

  // Teacher-forced scoring (mt3_engine_score): a workspace of score_cap segments x score_Lp rows, allocated by the first
  // call (and grown by mt3_debug_engine_set_score_chunk); an engine that never scores keeps its device bytes
  int score_cap = 0;             // segments the workspace holds (0: not allocated)
  int score_Lp = 0;              // rows per segment: max_decode_len rounded up to 64
  int score_chunk_req = 0;       // mt3_debug_engine_set_score_chunk (0: the workspace default)
  int score_chunks = 0;          // chunks of the most recent score call
  int score_passes = 0;          // encoder passes of the most recent mt3_engine_score_segments / _score_candidates
  bool score_planes = false;     // f32 engine (x6): the plane copies of the decoder's matrices and of logits_w exist
  float* sc_y = nullptr;         // [rows][emb] f32 residual rows
  void* sc_y_ct = nullptr;       // bf16: compute-type copy [rows][emb] ...
  float* sc_y_ss = nullptr;      // ... and per-16-column sums of squares [rows][emb / 16]
  void* sc_qkv = nullptr;        // [rows][3HD]
  void* sc_attn = nullptr;       // [rows][HD]
  void* sc_q = nullptr;          // [rows][HD] cross-attention queries
  void* sc_h = nullptr;          // [rows][mlp]
  float* sc_logits = nullptr;    // [rows][vocab]
  int* sc_tgt = nullptr;         // [rows] padded targets
  float* sc_tok = nullptr;       // [rows] token scores

  int HD() const { return cfg.num_heads * cfg.head_dim; }
};

namespace {

using mt3k::brevity_penalty;     // t5x decoding.brevity_penalty(alpha = 0.6, length), kernels.h

#define MT3_TRY(expr)           \
  do {                          \
    int _rc = (expr);           \
    if (_rc != MT3_OK) return _rc; \
  } while (0)

// the kernels' view of a table for one step: the index starts at the step's first row / element `seg0` (0 with `slot_seg`,
// the in-flight map of the step's first slot, which then names the segment)
template <typename T>
mt3k::SegTable<T> seg_view(const SegTableHost<T>& tb, size_t seg0, const int* slot_seg) {
  return mt3k::SegTable<T>{tb.rows, tb.seg_on ? tb.seg + seg0 : nullptr, slot_seg, tb.stride};
}

// MT3_OK, or why a job of `n` rows / elements / segments cannot run under table `tb` (`whose`): the per-row statistic of
// every row in use must lie in [lo, hi], else `why`
template <typename T>
int fits(const SegTableHost<T>& tb, const char* who, int n, int lo, int hi, const char* whose, const char* why) {
  if (!tb.n) return MT3_OK;
  if (tb.seg_on && n > static_cast<int>(tb.seg_host.size()))
    return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": more rows or segments than " + whose + " n_segments");
  for (int i = 0; i < (tb.seg_on ? n : 1); ++i) {
    const int r = tb.seg_on ? tb.seg_host[i] : 0;
    if (r >= 0 && (tb.stat[r] < lo || tb.stat[r] > hi)) return mt3::fail(MT3_ERR_INVALID, std::string(who) + why);
  }
  return MT3_OK;
}

int dmalloc(mt3_engine* e, void** p, size_t bytes) {
  MT3_HIP_CHECK(hipMalloc(p, bytes));
  e->allocs.push_back(*p);
  e->device_bytes += static_cast<int64_t>(bytes);
  return MT3_OK;
}

// Upload a host f32 matrix [N][K] as the compute type and, of `forms` (kFormPlanes | kFormMx8), as those the engine
// multiplies with: three bf16 planes on the f32 engine's three-plane tile (mt3_engine::x6), MXFP8 on the MXFP8 dense path.
// `h` may go on past row N: all of it is uploaded in the compute type, the other forms cover [N][K]
int upload_dense(mt3_engine* e, const std::vector<float>& h, int N, int K, int forms, Dense* D) {
  const size_t n = static_cast<size_t>(N) * K;
  if (h.size() < n) return mt3::fail(MT3_ERR_INVALID, "upload_dense: the host matrix is smaller than [N][K]");
  D->N = N;
  D->K = K;
  MT3_TRY(dmalloc(e, &D->w, h.size() * e->esize));
  if (e->cfg.compute_dtype == MT3_BF16) {
    std::vector<uint16_t> t(h.size());
    for (size_t i = 0; i < h.size(); ++i) t[i] = f32_to_bf16_bits(h[i]);
    MT3_HIP_CHECK(hipMemcpy(D->w, t.data(), t.size() * 2, hipMemcpyHostToDevice));
  } else {
    MT3_HIP_CHECK(hipMemcpy(D->w, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  }
  if ((forms & kFormPlanes) && e->x6) {
    // hi = rne(w), mid = rne(w - hi), lo = rne(w - hi - mid) (both differences exact)
    std::vector<uint16_t> pl[3];
    for (auto& v : pl) v.resize(n);
    for (size_t i = 0; i < n; ++i) {
      auto val = [](uint16_t b) {
        const uint32_t u = static_cast<uint32_t>(b) << 16;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
      };
      const uint16_t hi = f32_to_bf16_bits(h[i]);
      const float r1 = h[i] - val(hi);
      const uint16_t mi = f32_to_bf16_bits(r1);
      const float r2 = r1 - val(mi);
      pl[0][i] = hi;
      pl[1][i] = mi;
      pl[2][i] = f32_to_bf16_bits(r2);
    }
    for (int k = 0; k < 3; ++k) {
      MT3_TRY(dmalloc(e, &D->p[k], n * 2));
      MT3_HIP_CHECK(hipMemcpy(D->p[k], pl[k].data(), n * 2, hipMemcpyHostToDevice));
    }
  }
  if ((forms & kFormMx8) && e->dense_fp8) {
    std::vector<uint8_t> hq(n), hs(static_cast<size_t>(N) * (K / 32));
    MT3_TRY(mt3_host_mx8_quantize(h.data(), N, K, hq.data(), hs.data()));
    MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&D->q), hq.size()));
    MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&D->sc), hs.size()));
    MT3_HIP_CHECK(hipMemcpy(D->q, hq.data(), hq.size(), hipMemcpyHostToDevice));
    MT3_HIP_CHECK(hipMemcpy(D->sc, hs.data(), hs.size(), hipMemcpyHostToDevice));
  }
  return MT3_OK;
}

int upload_f32(mt3_engine* e, const std::vector<float>& h, float** d) {
  int rc = dmalloc(e, reinterpret_cast<void**>(d), h.size() * 4);
  if (rc) return rc;
  MT3_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  return MT3_OK;
}

const HostWeight* find(mt3_engine* e, const std::string& name, int64_t d0, int64_t d1) {
  auto it = e->raw.find(name);
  if (it == e->raw.end()) {
    mt3::fail(MT3_ERR_MISSING, "weight not loaded: " + name);
    return nullptr;
  }
  const HostWeight& w = it->second;
  const bool ok = (d1 < 0) ? (w.shape.size() == 1 && w.shape[0] == d0)
                           : (w.shape.size() == 2 && w.shape[0] == d0 && w.shape[1] == d1);
  if (!ok) {
    mt3::fail(MT3_ERR_INVALID, "weight has the wrong shape: " + name);
    return nullptr;
  }
  return &w;
}

// dst rows [row0, row0+out) of an output-major matrix with `in` columns  <-  W[in][out] (* scale[in])
void put_transposed(std::vector<float>& dst, int in, int row0, const HostWeight& w, const float* scale) {
  const int out = static_cast<int>(w.shape[1]);
  for (int k = 0; k < in; ++k) {
    const float s = scale ? scale[k] : 1.f;
    const float* src = w.data.data() + static_cast<size_t>(k) * out;
    for (int n = 0; n < out; ++n) dst[static_cast<size_t>(row0 + n) * in + k] = src[n] * s;
  }
}

int build_attention(mt3_engine* e, const std::string& prefix, const float* scale, bool cross, LayerDev* L,
                    bool encoder = false) {
  const int emb = e->cfg.emb_dim, hd = e->HD();
  const HostWeight *q = find(e, prefix + "/query/kernel", emb, hd), *k = find(e, prefix + "/key/kernel", emb, hd),
                   *v = find(e, prefix + "/value/kernel", emb, hd), *o = find(e, prefix + "/out/kernel", hd, emb);
  if (!q || !k || !v || !o) return MT3_ERR_MISSING;
  const int all = kFormPlanes | kFormMx8;
  std::vector<float> ot(static_cast<size_t>(emb) * hd);
  put_transposed(ot, hd, 0, *o, nullptr);
  if (!cross) {
    std::vector<float> t(static_cast<size_t>(3) * hd * emb);
    put_transposed(t, emb, 0, *q, scale);
    put_transposed(t, emb, hd, *k, scale);
    put_transposed(t, emb, 2 * hd, *v, scale);
    MT3_TRY(upload_dense(e, t, 3 * hd, emb, encoder ? all : 0, &L->wqkv));
    MT3_TRY(upload_dense(e, ot, emb, hd, encoder ? all : 0, &L->wo));
  } else {
    std::vector<float> tq(static_cast<size_t>(hd) * emb), tkv(static_cast<size_t>(2) * hd * emb);
    put_transposed(tq, emb, 0, *q, scale);         // query side sees the pre_cross_attention norm
    put_transposed(tkv, emb, 0, *k, nullptr);      // key/value side sees `encoded` (already normed)
    put_transposed(tkv, emb, hd, *v, nullptr);
    MT3_TRY(upload_dense(e, tq, hd, emb, 0, &L->wq_x));
    MT3_TRY(upload_dense(e, tkv, 2 * hd, emb, all, &L->wkv_x));     // the encoder pass multiplies with it
    MT3_TRY(upload_dense(e, ot, emb, hd, 0, &L->wo_x));
  }
  return MT3_OK;
}

const float* scale_of(mt3_engine* e, const std::string& name) {
  const HostWeight* w = find(e, name, e->cfg.emb_dim, -1);
  return w ? w->data.data() : nullptr;
}

// Wext^T of decoder layer l: output-major [4HD][emb] = scaled q | k | v of the self-attention, scaled cross-attention
// query (what the q-fold's QKV launch multiplies with, and what the qkv-fold folds into the previous layer's launches)
int wext_t(mt3_engine* e, int l, std::vector<float>* t) {
  const int emb = e->cfg.emb_dim, hd = e->HD();
  const std::string P = "decoder/layers_" + std::to_string(l);
  const float* s1 = scale_of(e, P + "/pre_self_attention_layer_norm/scale");
  const float* s2 = scale_of(e, P + "/pre_cross_attention_layer_norm/scale");
  const HostWeight *q = find(e, P + "/self_attention/query/kernel", emb, hd),
                   *k = find(e, P + "/self_attention/key/kernel", emb, hd),
                   *v = find(e, P + "/self_attention/value/kernel", emb, hd),
                   *qx = find(e, P + "/encoder_decoder_attention/query/kernel", emb, hd);
  if (!s1 || !s2 || !q || !k || !v || !qx) return MT3_ERR_MISSING;
  t->assign(static_cast<size_t>(4) * hd * emb, 0.f);
  put_transposed(*t, emb, 0, *q, s1);
  put_transposed(*t, emb, hd, *k, s1);
  put_transposed(*t, emb, 2 * hd, *v, s1);
  put_transposed(*t, emb, 3 * hd, *qx, s2);
  return MT3_OK;
}

// q-fold matrices of one decoder layer (see mt3_engine::qf)
int build_q_fold(mt3_engine* e, int l, const float* s2, LayerDev* L) {
  const int emb = e->cfg.emb_dim, hd = e->HD();
  const std::string P = "decoder/layers_" + std::to_string(l);
  const HostWeight *o = find(e, P + "/self_attention/out/kernel", hd, emb),
                   *qx = find(e, P + "/encoder_decoder_attention/query/kernel", emb, hd);
  if (!o || !qx) return MT3_ERR_MISSING;
  std::vector<float> t;
  MT3_TRY(wext_t(e, l, &t));
  MT3_TRY(upload_dense(e, t, 4 * hd, emb, 0, &L->wqkv_ext));
  // rows [0, emb): Wo^T;  rows [emb, emb + hd): P^T with P[k][n] = sum_e Wo[k][e] * s2[e] * Wq_x[e][n]  (double)
  std::vector<float> u(static_cast<size_t>(emb + hd) * hd);
  put_transposed(u, hd, 0, *o, nullptr);
  std::vector<double> acc(hd);
  for (int kk = 0; kk < hd; ++kk) {
    std::fill(acc.begin(), acc.end(), 0.0);
    const float* orow = o->data.data() + static_cast<size_t>(kk) * emb;
    for (int ee = 0; ee < emb; ++ee) {
      const double w = static_cast<double>(orow[ee]) * s2[ee];
      const float* qrow = qx->data.data() + static_cast<size_t>(ee) * hd;
      for (int n = 0; n < hd; ++n) acc[n] += w * qrow[n];
    }
    for (int n = 0; n < hd; ++n) u[static_cast<size_t>(emb + n) * hd + kk] = static_cast<float>(acc[n]);
  }
  return upload_dense(e, u, emb + hd, hd, 0, &L->wo_ext);
}

mt3k::GemmArgs gemm_args(const void* A, const void* Wt, void* out, int M, int N, int K, int ldo);

// qkv-fold matrices and tables (see mt3_engine::qkv_fold); wi_host[l] = layer l's GEGLU matrix as build_mlp laid it
// out, which leaves here with the layer's Wext^T rows appended.  The matrix products (Wo_mlp . Wext per layer: 0.8 GFLOP;
// embedding / position table . Wext of layer 0) run on the device with the engine's own f32 GEMM (exact f32 products,
// f32 accumulation: ~1e-6 of an entry, far below what the operand formats keep) instead of seconds of host loops.
int build_qkv_fold(mt3_engine* e, const std::vector<std::vector<float>>& wi_host) {
  const mt3_engine_config& c = e->cfg;
  const int emb = c.emb_dim, hd = e->HD(), mlp = c.mlp_dim, n4 = 4 * hd, nl = c.num_decoder_layers;
  float *d_wext = nullptr, *d_wo = nullptr, *d_prod = nullptr;
  auto cleanup = [&]() {
    if (d_wext) (void)hipFree(d_wext);
    if (d_wo) (void)hipFree(d_wo);
    if (d_prod) (void)hipFree(d_prod);
  };
  int rc = MT3_OK;
  const int n_max = n4 > c.vocab_size ? n4 : c.vocab_size;
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&d_wext), static_cast<size_t>(n_max) * emb * 4);
  if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&d_wo), static_cast<size_t>(mlp) * emb * 4);
  if (he == hipSuccess) he = hipMalloc(reinterpret_cast<void**>(&d_prod), static_cast<size_t>(n_max) * mlp * 4);
  std::vector<float> wt, prod, w;
  // layer l's MLP out-projection launch carries the NEXT consumer of its output row: layer l + 1's q | k | v | cross-q
  // (4HD columns), or -- last layer -- the logits projection (vocab columns, decoder_norm scale folded)
  for (int l = 0; l < nl && he == hipSuccess && rc == MT3_OK; ++l) {
    const bool last = l + 1 == nl;
    const int nx = last ? c.vocab_size : n4;
    const HostWeight* wo = find(e, "decoder/layers_" + std::to_string(l) + "/mlp/wo/kernel", mlp, emb);
    if (!wo) rc = MT3_ERR_MISSING;
    if (rc == MT3_OK && !last) rc = wext_t(e, l + 1, &wt);
    if (rc == MT3_OK && last) {
      const float* sn = scale_of(e, "decoder/decoder_norm/scale");
      const HostWeight* wl = find(e, "decoder/logits_dense/kernel", emb, c.vocab_size);
      if (!sn || !wl) rc = MT3_ERR_MISSING;
      else {
        wt.assign(static_cast<size_t>(nx) * emb, 0.f);
        put_transposed(wt, emb, 0, *wl, sn);
      }
    }
    if (rc != MT3_OK) break;
    he = hipMemcpy(d_wext, wt.data(), wt.size() * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_wo, wo->data.data(), wo->data.size() * 4, hipMemcpyHostToDevice);
    if (he != hipSuccess) break;
    // prod[n][k] = sum_e Wext^T[n][e] * Wo_mlp[k][e]: "A" = Wext^T rows, "Wt" = Wo_mlp rows (K = emb for both)
    mt3k::GemmArgs g = gemm_args(d_wext, d_wo, d_prod, nx, mlp, emb, mlp);
    rc = mt3k::launch_gemm(MT3_F32, g, false, 0, MT3_EPI_F32, false, nullptr);
    if (rc != MT3_OK) break;
    prod.resize(static_cast<size_t>(nx) * mlp);
    he = hipMemcpy(prod.data(), d_prod, prod.size() * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) break;
    // MLP out-projection launch: [Wo_mlp^T ; (Wo_mlp . Wext)^T], K = mlp
    w.assign((static_cast<size_t>(emb) + nx) * mlp, 0.f);
    for (int k = 0; k < mlp; ++k)
      for (int n = 0; n < emb; ++n) w[static_cast<size_t>(n) * mlp + k] = wo->data[static_cast<size_t>(k) * emb + n];
    std::memcpy(w.data() + static_cast<size_t>(emb) * mlp, prod.data(), static_cast<size_t>(nx) * mlp * 4);
    rc = upload_dense(e, w, emb + nx, mlp, 0, &e->dec[l].w_fold);
    if (rc != MT3_OK) break;
    // GEGLU launch: [wi_0 | wi_1 interleaved ; Wext^T ; zero rows up to whole 64-column tiles], K = emb
    const size_t n_wi = static_cast<size_t>(2) * mlp * emb, nx64 = (static_cast<size_t>(nx) + 63) / 64 * 64;
    if (wi_host[l].size() != n_wi) {
      rc = mt3::fail(MT3_ERR_INVALID, "qkv-fold: GEGLU matrix of the layer missing");
      break;
    }
    w.assign(n_wi + nx64 * emb, 0.f);
    std::memcpy(w.data(), wi_host[l].data(), n_wi * 4);
    std::memcpy(w.data() + n_wi, wt.data(), static_cast<size_t>(nx) * emb * 4);
    rc = upload_dense(e, w, 2 * mlp, emb, 0, &e->dec[l].wi);     // (N: the GEGLU rows, see LayerDev::wi)
  }
  // layer 0: its input row is Embed(tok) + FixedEmbed[t], so its projection is the sum of two table rows
  if (he == hipSuccess && rc == MT3_OK) rc = wext_t(e, 0, &wt);
  if (he == hipSuccess && rc == MT3_OK) {
    he = hipMemcpy(d_wext, wt.data(), wt.size() * 4, hipMemcpyHostToDevice);
    if (he == hipSuccess) rc = dmalloc(e, reinterpret_cast<void**>(&e->ew0), static_cast<size_t>(c.vocab_size) * n4 * 4);
    if (he == hipSuccess && rc == MT3_OK)
      rc = dmalloc(e, reinterpret_cast<void**>(&e->pw0), static_cast<size_t>(kMaxPos) * n4 * 4);
    if (he == hipSuccess && rc == MT3_OK)
      rc = mt3k::launch_gemm(MT3_F32, gemm_args(e->embedding, d_wext, e->ew0, c.vocab_size, n4, emb, n4), false, 0,
                             MT3_EPI_F32, false, nullptr);
    if (he == hipSuccess && rc == MT3_OK)
      rc = mt3k::launch_gemm(MT3_F32, gemm_args(e->pos_table, d_wext, e->pw0, kMaxPos, n4, emb, n4), false, 0,
                             MT3_EPI_F32, false, nullptr);
    if (he == hipSuccess && rc == MT3_OK) he = hipDeviceSynchronize();
  }
  cleanup();
  if (rc != MT3_OK) return rc;
  if (he != hipSuccess) return mt3::fail(MT3_ERR_HIP, std::string("qkv-fold tables: ") + hipGetErrorString(he));
  return MT3_OK;
}

// keep_wi != nullptr: the GEGLU matrix is not uploaded but handed back (build_qkv_fold uploads it with more rows)
int build_mlp(mt3_engine* e, const std::string& prefix, const float* scale, LayerDev* L, bool encoder = false,
              std::vector<float>* keep_wi = nullptr) {
  const int emb = e->cfg.emb_dim, mlp = e->cfg.mlp_dim;
  const HostWeight *w0 = find(e, prefix + "/wi_0/kernel", emb, mlp), *w1 = find(e, prefix + "/wi_1/kernel", emb, mlp),
                   *wo = find(e, prefix + "/wo/kernel", mlp, emb);
  if (!w0 || !w1 || !wo) return MT3_ERR_MISSING;
  // rows [32q, 32q+16) = gate columns 16q.., rows [32q+16, 32q+32) = linear columns 16q..
  std::vector<float> t(static_cast<size_t>(2) * mlp * emb);
  for (int k = 0; k < emb; ++k) {
    const float s = scale[k];
    for (int n = 0; n < mlp; ++n) {
      const int q = n >> 4, r = n & 15;
      t[static_cast<size_t>(32 * q + r) * emb + k] = w0->data[static_cast<size_t>(k) * mlp + n] * s;
      t[static_cast<size_t>(32 * q + 16 + r) * emb + k] = w1->data[static_cast<size_t>(k) * mlp + n] * s;
    }
  }
  std::vector<float> ot(static_cast<size_t>(emb) * mlp);
  put_transposed(ot, mlp, 0, *wo, nullptr);
  const int forms = encoder ? kFormPlanes | kFormMx8 : 0;
  MT3_TRY(upload_dense(e, ot, emb, mlp, forms, &L->wo_mlp));
  if (keep_wi) keep_wi->swap(t);
  else MT3_TRY(upload_dense(e, t, 2 * mlp, emb, forms, &L->wi));
  return MT3_OK;
}

mt3k::GemmArgs gemm_args(const void* A, const void* Wt, void* out, int M, int N, int K, int ldo) {
  mt3k::GemmArgs g{};
  g.A = A;
  g.Wt = Wt;
  g.out = out;
  g.M = M;
  g.N = N;
  g.K = K;
  g.lda = K;
  g.ldo = ldo;
  return g;
}

// One decode step of rows [row0, row0 + rows) -- a "chain".  The batch of a decode call is split into
// `e->chains` such chains; they are data-independent (a segment never looks at another segment), so
// the step graph has one branch per chain and the GPU overlaps one chain's latency-bound GEMMs with
// another chain's HBM-bound attention streams.  Every row-indexed workspace is simply offset.
// Op `op` of the decode step of rows [row0, row0 + rows): per decoder layer 8 ops
//   0 QKV GEMM (fused RMSNorm)   1 self-attention (+cache append)   2 out-proj + residual
//   3 q-proj (fused RMSNorm)     4 cross-attention                  5 out-proj + residual
//   6 GEGLU GEMM (fused RMSNorm) 7 wo + residual
// then  8*L: logits GEMM (fused decoder_norm),  8*L + 1: argmax / EOS / position += 1 / next input row.
// Ops 1 and 4 are the HBM-streaming ("heavy") ones; everything else is latency-bound.
inline int chain_num_ops(const mt3_engine* e) { return 8 * e->cfg.num_decoder_layers + 2; }
inline bool chain_op_is_heavy(const mt3_engine* e, int op) {
  return op < 8 * e->cfg.num_decoder_layers && ((op & 7) == 1 || (op & 7) == 4);
}

// the per-slot state of slots [row0, ...) of the row group that counts its finished slots in n_done[done_slot]
mt3k::SlotState slot_state(mt3_engine* e, int row0, int done_slot) {
  // (the grammar state only with a grammar set: without one nothing moves, resets or reads it)
  mt3k::SlotState st{e->done + row0, e->slot_row + row0, e->slot_seg + row0, e->step + row0,
                     e->cur_tok + row0,  e->n_done + done_slot, e->gr.on ? e->gram + row0 : nullptr};
  if (e->nt.on) {                // (the note state only while the note rule is set, as the grammar state)
    st.held_words = mt3n_table_words(&e->nt.n);
    st.note = e->note + row0;
    st.nrow = e->nrow + static_cast<size_t>(row0) * MT3_NOTE_ROW_WORDS;
    st.held = e->held + static_cast<size_t>(row0) * st.held_words;
  }
  return st;
}

// the decoder input rows of slots [row0, ...) and what they are written from.  The one place that knows which forms the
// engine keeps: the bf16 copy with the split form of the bf16 path (f32: the compute-type rows ARE the f32 rows), the
// sums of squares with the split form, layer 0's projected rows with the qkv-fold
mt3k::InputRow input_row(mt3_engine* e, int row0) {
  const mt3_engine_config& c = e->cfg;
  const size_t r0 = static_cast<size_t>(row0);
  const int emb = c.emb_dim, n4 = 4 * e->HD();
  mt3k::InputRow in{};
  in.table = e->embedding;
  in.pos = e->pos_table;
  in.max_pos = kMaxPos;
  in.y = e->y + r0 * emb;                        // the token-pick kernels leave the next input row in buffer 0
  if (e->y_split && c.compute_dtype == MT3_BF16) in.y_ct = static_cast<char*>(e->y_ct) + r0 * emb * 2;
  if (e->y_split) in.y_ss = e->y_ss + r0 * (emb / 16);
  in.dim = emb;
  in.rp = mt3k::RowProj{e->ew0, e->pw0, e->qkv_fold ? e->qkvf + r0 * n4 : nullptr, n4};
  return in;
}

// the beam-1 state of slots [row0, ...); its row-indexed lengths start at row crow0 (row0, or 0 under a slot map)
mt3k::BeamState beam1_state(mt3_engine* e, int row0, size_t crow0) {
  return mt3k::BeamState{e->beam_f + row0, e->beam_len + row0, e->beam_cfg, e->cfg.max_batch, e->beam_len_row + crow0};
}

// the k-beam state of slots [row0, row0 + rows) (the kernel-side pointers are those of the first slot)
mt3k::BeamKArgs beam_args(mt3_engine* e, int row0, int rows, int k, int done_slot = 0) {
  mt3k::BeamKArgs b{};
  b.vocab = e->cfg.vocab_size;
  b.k = k;
  b.elems = rows / k;
  b.st = slot_state(e, row0, done_slot);
  b.in = input_row(e, row0);
  b.live = e->bk_live + row0;
  b.fin_score = e->bk_fin_score + row0;
  b.fin_step = e->bk_fin_step + row0;
  b.fin_beam = e->bk_fin_beam + row0;
  b.hist_par = e->bk_par + row0;
  b.hist_tok = e->bk_tok + row0;
  b.hist_stride = e->cfg.max_batch;
  b.fork_src = e->bk_fork_src + row0;
  b.fork_count = e->bk_forks;
  b.bp = e->beam_cfg;
  return b;
}

// A residual stream: M f32 rows of emb columns and, in the split form, what travels with them -- per row the sums of
// squares of every 16-column group and (bf16) a compute-type copy, kept up to date by every producer of the rows -- so
// that the norm-fused GEMMs read compute-type operands and need no statistics pass of their own
struct Resid {
  float* y = nullptr;        // [M][emb]
  void* ct = nullptr;        // split, bf16: [M][emb] (f32 engine: none)
  float* ss = nullptr;       // split: [M][emb / 16]
  bool split = false;
  bool x6 = false;           // products of this stream run on the three-plane tile (f32 engine, encoder-sized passes)
  int M = 0;
  // the rows as a norm-fused GEMM reads them.  Split form of the f32 engine: the compute-type rows ARE the f32 rows, and
  // no copy is written
  const void* a() const { return split && ct ? ct : y; }
};

// the decode step's rows: `rows` slots from the one `in` starts at (input_row)
Resid decode_rows(const mt3_engine* e, const mt3k::InputRow& in, int rows) {
  return Resid{in.y, in.y_ct, in.y_ss, e->y_split, false, rows};
}

// an encoder pass of M rows
Resid encoder_rows(const mt3_engine* e, int M, bool small) {
  const mt3_engine_config& c = e->cfg;
  const int emb = c.emb_dim;
  // (gemm_x6_kernel addresses its operands with 32-bit byte offsets: a batch whose widest f32 activation matrix reaches
  // 4 GB -- 4096 segments at the MT3 shape -- takes the f32-instruction tiles instead of failing)
  const int widest = std::max(std::max(c.input_depth, emb), std::max(e->HD(), c.mlp_dim));
  const bool x6_fits = static_cast<size_t>(M) * widest * 4 < (1ull << 32);
  // the split residual form feeds the LDS-DMA tile (K <= 1024); the decode-sized tile a small batch selects holds the
  // partial sums of K <= 512 or K = 768 only, so a small batch of a wider model stays on the single f32 stream
  const bool xs = e->x_split && !(small && !(emb <= 512 || emb == 768));
  return Resid{e->x, xs ? e->x_ct : nullptr, xs ? e->x_ss : nullptr, xs, e->x6 && x6_fits, M};
}

bool score_split(const mt3_engine* e) {
  const int emb = e->cfg.emb_dim;
  return e->cfg.compute_dtype == MT3_BF16 && emb % 64 == 0 && emb <= 1024;
}

// a chunk of M rows of the score workspace
Resid score_rows(const mt3_engine* e, int M) {
  const bool split = score_split(e);
  return Resid{e->sc_y, split ? e->sc_y_ct : nullptr, split ? e->sc_y_ss : nullptr, split, e->x6, M};
}

mt3k::GemmArgs gemm_args(const void* A, const Dense& W, void* out, int M, int ldo) {
  return gemm_args(A, W.w, out, M, W.N, W.K, ldo);
}

// g (made by gemm_args from W) on the three-plane tile (x6: W's planes, f32 A and f32 outputs) or on launch_gemm's tiles
int dense_gemm(mt3_engine* e, bool x6, mt3k::GemmArgs g, const Dense& W, bool a_f32, int norm, int epi, bool small,
               hipStream_t s) {
  if (!x6) return mt3k::launch_gemm(e->cfg.compute_dtype, g, a_f32, norm, epi, small, s);
  g.Wt = W.p[0];
  return mt3k::launch_gemm_x6(g, W.p[1], W.p[2], norm != 0, epi == MT3_EPI_F32 ? MT3_EPI_STORE : epi, s);
}

// What a decode-step launch carries beside the plain product (GemmArgs): N > 0: the launch's output columns where they
// are not W.N; columns [n_split, N) are a second product that goes to out2 (kEpiStoreQ / kEpiResidQ / kEpiGegluP);
// concurrent: the launch runs beside other row groups' launches
struct GemmExtra {
  int N = 0;
  float* out2 = nullptr;
  int ld2 = 0, n_split = 0, concurrent = 0;
};

mt3k::GemmArgs gemm_args(const void* A, const Dense& W, void* out, int M, int ldo, const GemmExtra& x) {
  mt3k::GemmArgs g = gemm_args(A, W, out, M, ldo);
  if (x.N) g.N = x.N;
  g.out2 = x.out2;
  g.ld2 = x.ld2;
  g.n_split = x.n_split;
  g.concurrent = x.concurrent;
  return g;
}

// the normalised rows of R into a projection: out = epi(rmsnorm(R) . W^T) (the norm's scale is folded into W's rows)
int normed_gemm(mt3_engine* e, const Resid& R, const Dense& W, void* out, int ldo, int epi, bool small, hipStream_t s,
                const GemmExtra& x = {}) {
  mt3k::GemmArgs g = gemm_args(R.a(), W, out, R.M, ldo, x);
  g.a_ss = R.ss;
  return dense_gemm(e, R.x6, g, W, !R.split, R.split ? 2 : 1, epi, small, s);
}

// a product added back into the rows of R: R += A . W^T, every form of R kept up to date
int resid_gemm(mt3_engine* e, const Dense& W, const void* A, const Resid& R, bool small, hipStream_t s,
               const GemmExtra& x = {}) {
  mt3k::GemmArgs g = gemm_args(A, W, R.y, R.M, e->cfg.emb_dim, x);
  g.out_ct = R.ct;
  g.out_ss = R.ss;
  return dense_gemm(e, R.x6, g, W, false, 0, x.out2 ? mt3k::kEpiResidQ : MT3_EPI_RESID, small, s);
}

int enqueue_chain_op(mt3_engine* e, int row0, int rows, int B_total, int skip, int op, hipStream_t s, int done_slot = 0) {
  const mt3_engine_config& c = e->cfg;
  const int dt = c.compute_dtype, emb = c.emb_dim, hd = e->HD(), H = c.num_heads, T = c.input_length;
  const int Lmax = c.max_decode_len;
  const size_t es = e->esize, kes = e->kv_esize;
  const int nl = c.num_decoder_layers;
  const bool fold = e->qkv_fold;
  // row retirement: the step's slots [row0, row0 + rows) reach their cache rows / id rows through e->slot_row, so the
  // cache and id base pointers stay those of the whole batch
  const bool retire = (skip & kVarRetire) != 0;
  const size_t crow0 = retire ? 0 : static_cast<size_t>(row0);
  // the decoder input row of this step (Embed(tok) + FixedEmbed[t]) is already in `y`: written by the
  // embed launch before the first step and by the previous step's argmax kernel afterwards
  const mt3k::InputRow in = input_row(e, row0);
  const Resid R = decode_rows(e, in, rows);
  float* y_ss = in.y_ss;
  // this step belongs to one of several row groups / graph chains (GemmArgs::concurrent: every residual add and the
  // GEGLU launch).  Under row retirement rows < B_total also holds for a LONE stream after a compaction, hence the
  // explicit bit.  Graph chains never carry the bit (kVarBeside is set only for a job of several row groups,
  // run_one_group, and a chains job is one group), so under row retirement they take the lone stream's tiles: meant so.
  GemmExtra ex;
  ex.concurrent = ((skip & kVarBeside) || (!retire && rows < B_total)) ? 1 : 0;
  char* qkv_d = static_cast<char*>(e->qkv_d) + static_cast<size_t>(row0) * 3 * hd * es;
  char* attn_d = static_cast<char*>(e->attn_d) + static_cast<size_t>(row0) * hd * es;
  char* q_d = static_cast<char*>(e->q_d) + static_cast<size_t>(row0) * hd * es;
  char* h_d = static_cast<char*>(e->h_d) + static_cast<size_t>(row0) * c.mlp_dim * es;
  float* qkvf = in.rp.q_out;
  float* logits = e->logits + static_cast<size_t>(row0) * c.vocab_size;
  int* step = e->step + row0;                    // per-row position counters
  if (op == 8 * nl) {
    if (fold) return MT3_OK;                  // the logits projection rode in the last layer's MLP out-projection launch
    return normed_gemm(e, R, e->logits_w, logits, c.vocab_size, MT3_EPI_F32, true, s);
  }
  if (op == 8 * nl + 1 && (skip & kVarBeams)) {
    // k-beam search: the beam step, then the cache-row copies of the beams that forked
    mt3k::BeamKArgs b = beam_args(e, row0, rows, (skip >> kVarBeamsShift) & 15, done_slot);
    b.logits = logits;
    b.max_len = (skip & kVarStream) ? e->stream_max_len : 0;
    const mt3k::LogitScale ls{fold ? y_ss : nullptr, emb / 16, emb};
    // both tables are indexed by the element's segment in flight, by element row0 / k + block in a batch call
    const bool streaming = (skip & kVarStream) != 0;
    const size_t seg0 = streaming ? 0 : static_cast<size_t>(row0 / b.k);
    const int* slot_seg = streaming ? e->slot_seg + row0 : nullptr;
    const mt3k::TokenMask tm = (skip & kVarMask) ? seg_view(e->tm, seg0, slot_seg) : mt3k::TokenMask{};
    const mt3k::TokenPrompt tp = (skip & kVarPrompt) ? seg_view(e->tp, seg0, slot_seg) : mt3k::TokenPrompt{};
    MT3_TRY(mt3k::launch_beam_step(b, ls, tm, tp, (skip & kVarGrammar) ? e->gr : mt3k::TokenGrammar{},
                                   (skip & kVarNotes) ? e->nt : mt3k::TokenNotes{}, s));
    mt3k::BeamReorderArgs r{};
    r.n_layers = nl;
    r.H = H;
    r.cap = Lmax;
    r.kv_esize = static_cast<int>(kes);
    r.slots = rows;
    for (int l = 0; l < nl; ++l) {                   // cache bases of the whole batch: slot_row holds batch rows
      r.k[l] = static_cast<char*>(e->dec[l].self_k);
      r.v[l] = static_cast<char*>(e->dec[l].self_v);
      r.scale[l] = e->kv_fp8 ? e->dec[l].self_scale : nullptr;
    }
    r.fork_src = e->bk_fork_src + row0;
    r.slot_row = e->slot_row + row0;
    r.step = step;
    r.done = e->done + row0;
    return mt3k::launch_beam_reorder(r, s);
  }
  if (op == 8 * nl + 1) {
    mt3k::ArgmaxStepArgs a{};
    a.logits = logits;
    a.vocab = c.vocab_size;
    a.ids = e->ids + crow0 * Lmax;
    a.ids_stride = Lmax;
    a.st = slot_state(e, row0, done_slot);
    a.in = in;
    if (skip & kVarBeam) a.beam = beam1_state(e, row0, crow0);
    if (skip & kVarForced) a.forced = e->forced + static_cast<size_t>(row0) * Lmax;
    a.forced_stride = Lmax;
    // folded logits arrive unnormalised: the row scale comes from the final residual row's partial sums
    a.ls = mt3k::LogitScale{fold ? y_ss : nullptr, emb / 16, emb};
    const bool streaming = (skip & kVarStream) != 0;
    a.rt = mt3k::StepRetire{retire ? 1 : 0, retire ? a.st.slot_row : nullptr, (skip & kVarEos) ? e->eos_at + crow0 : nullptr,
                            streaming ? a.st.slot_seg : nullptr, streaming ? e->stream_max_len : 0};
    a.B = rows;
    // both tables are indexed as eos_at is: by segment, or by the row the slot decodes (a.rt says which)
    if (skip & kVarMask) a.tm = seg_view(e->tm, crow0, nullptr);
    if (skip & kVarPrompt) a.tp = seg_view(e->tp, crow0, nullptr);
    if (skip & kVarGrammar) a.gr = e->gr;
    if (skip & kVarNotes) a.nt = e->nt;
    if (skip & kVarSample) {
      // the stream table is indexed as the masks are; without one the stream is the row / segment index itself
      mt3k::SampleStepArgs sa{a, e->samp, e->sstream.n ? seg_view(e->sstream, crow0, nullptr) : mt3k::SampleStream{},
                              static_cast<int>(crow0),
                              e->sseed.n ? seg_view(e->sseed, crow0, nullptr) : mt3k::SampleStream{}};
      return mt3k::launch_sample_step(sa, s);
    }
    return mt3k::launch_argmax_step(a, s);
  }
  LayerDev& L = e->dec[op >> 3];
  switch (op & 7) {
    case 0:
      if (fold) return MT3_OK;                // rode in the previous layer's MLP out-projection launch / the row's producer
      if (e->q_fold) {
        GemmExtra q;
        q.out2 = e->qf + static_cast<size_t>(row0) * hd;
        q.n_split = 3 * hd;
        return normed_gemm(e, R, L.wqkv_ext, qkv_d, 3 * hd, mt3k::kEpiStoreQ, true, s, q);
      }
      return normed_gemm(e, R, L.wqkv, qkv_d, 3 * hd, MT3_EPI_STORE, true, s);
    case 1: {
      if (skip & 1) return MT3_OK;
      mt3k::DecAttnArgs a{};
      a.q = qkv_d;
      a.q_stride = 3 * hd;
      a.kcache = static_cast<char*>(L.self_k) + crow0 * H * Lmax * 64 * kes;
      a.vcache = static_cast<char*>(L.self_v) + crow0 * H * Lmax * 64 * kes;
      a.kv_scale = e->kv_fp8 ? L.self_scale + crow0 * H * Lmax : nullptr;
      if (retire) {
        a.done = e->done + row0;
        a.cache_row = e->slot_row + row0;
      }
      a.cap = Lmax;
      a.new_k = qkv_d + static_cast<size_t>(hd) * es;
      a.new_v = qkv_d + static_cast<size_t>(2 * hd) * es;
      a.kv_stride = 3 * hd;
      if (fold) {                             // unnormalised f32 q | k | v + the input row's partial sums of squares
        a.q = nullptr;
        a.q_f32 = qkvf;
        a.q_stride = a.kv_stride = 4 * hd;
        a.new_k = qkvf + hd;
        a.new_v = qkvf + 2 * hd;
        a.q_ss = y_ss;
        a.q_ss_n = emb / 16;
      }
      a.step = step;
      a.out = attn_d;
      a.B = rows;
      a.H = H;
      return mt3k::launch_decode_attention(dt, a, s);
    }
    case 2:
      if (e->q_fold) {
        ex.out2 = fold ? qkvf + 3 * hd : e->qf + static_cast<size_t>(row0) * hd;
        ex.ld2 = fold ? 4 * hd : 0;
        ex.n_split = emb;
        return resid_gemm(e, L.wo_ext, attn_d, R, true, s, ex);
      }
      return resid_gemm(e, L.wo, attn_d, R, true, s, ex);
    case 3:
      if (e->q_fold) return MT3_OK;           // folded into ops 0 and 2
      return normed_gemm(e, R, L.wq_x, q_d, hd, MT3_EPI_STORE, true, s);
    case 4: {
      if (skip & 2) return MT3_OK;
      mt3k::DecAttnArgs x{};
      x.q = q_d;
      x.q_stride = hd;
      if (e->q_fold) {
        x.q = nullptr;                          // one query form per launch (launch_decode_attention refuses both)
        x.q_f32 = fold ? qkvf + 3 * hd : e->qf + static_cast<size_t>(row0) * hd;
        if (fold) x.q_stride = 4 * hd;
        x.q_ss = y_ss;
        x.q_ss_n = emb / 16;
      }
      x.kcache = static_cast<char*>(L.cross_kv) + crow0 * H * T * 64 * kes;
      x.vcache = static_cast<char*>(L.cross_kv) + (static_cast<size_t>(B_total) + crow0) * H * T * 64 * kes;
      x.kv_scale = e->kv_fp8 ? L.cross_scale + crow0 * H * T : nullptr;
      if (retire) {
        x.done = e->done + row0;
        x.cache_row = e->slot_row + row0;
      }
      x.cap = T;
      x.n_keys = T;
      x.out = attn_d;
      x.B = rows;
      x.H = H;
      return mt3k::launch_decode_attention(dt, x, s);
    }
    case 5:
      return resid_gemm(e, L.wo_x, attn_d, R, true, s, ex);
    case 6:
      if (fold) {
        // what consumes the row this layer is about to finish, unnormalised -- the NEXT layer's q | k | v | cross-q (4HD
        // columns of qkvf), after the last layer the logits -- is y2 . Wext + h . (Wo_mlp . Wext).  The first term needs
        // only the row this launch reads: it is computed here, in extra column tiles, on CUs the GEGLU tiles of this
        // row group leave idle (this layer's qkvf is dead: q | k | v went into op 1, the cross query into op 4; the
        // previous step's logits into its arg-max), and op 7 adds the second term.
        const bool last = (op >> 3) + 1 == nl;
        const int nx = last ? c.vocab_size : 4 * hd;
        ex.N = 2 * c.mlp_dim + (nx + 63) / 64 * 64;
        ex.out2 = last ? logits : qkvf;
        ex.ld2 = nx;
        ex.n_split = 2 * c.mlp_dim;
        return normed_gemm(e, R, L.wi, h_d, c.mlp_dim, mt3k::kEpiGegluP, true, s, ex);
      }
      return normed_gemm(e, R, L.wi, h_d, c.mlp_dim, MT3_EPI_GEGLU, true, s, ex);
    default:
      if (fold) {
        // MLP out-projection + residual, and -- as extra output columns over the same K = mlp -- h . (Wo_mlp . Wext),
        // added to the part of the next consumer's row that op 6 left in qkvf / logits
        const bool last = (op >> 3) + 1 == nl;
        const int nx = last ? c.vocab_size : 4 * hd;
        ex.out2 = last ? logits : qkvf;
        ex.ld2 = nx;
        ex.n_split = emb;
        return resid_gemm(e, L.w_fold, h_d, R, true, s, ex);
      }
      return resid_gemm(e, L.wo_mlp, h_d, R, true, s, ex);
  }
}

// rows of chain k when `B` rows are dealt to `n` chains
inline void chain_rows(int B, int n, int k, int* row0, int* rows) {
  const int q = B / n, r = B % n;
  *row0 = k * q + (k < r ? k : r);
  *rows = q + (k < r ? 1 : 0);
}

// chain k of the step of slots [row0, row0 + rows) of a B_total-row decode that is dealt to `chains` chains, on stream s
int enqueue_chain_step(mt3_engine* e, int row0, int rows, int B_total, int skip, int chains, int k, hipStream_t s,
                       int done_slot) {
  int r0, n;
  chain_rows(rows, chains, k, &r0, &n);
  for (int op = 0, ops = chain_num_ops(e); op < ops; ++op)
    MT3_TRY(enqueue_chain_op(e, row0 + r0, n, B_total, skip, op, s, done_slot));
  return MT3_OK;
}

// the whole step on ONE stream, chains back to back: the direct launch, and what the capture of a one-chain step records
int enqueue_step(mt3_engine* e, int row0, int rows, int B_total, int skip, int chains, hipStream_t s, int done_slot) {
  for (int k = 0; k < chains; ++k) MT3_TRY(enqueue_chain_step(e, row0, rows, B_total, skip, chains, k, s, done_slot));
  return MT3_OK;
}

int chains_for(const mt3_engine* e, int B, int requested) {
  int n = requested > 0 ? requested : (e->cfg.decode_chains > 0 ? e->cfg.decode_chains : 1);
  if (n > kMaxChains) n = kMaxChains;
  while (n > 1 && B / n < 16) --n;          // keep at least one MFMA row-fragment per chain
  return n;
}

}  // namespace

extern "C" {

static void workers_stop(mt3_engine* e);
static void drop_group_graphs(mt3_engine* e);

int mt3_engine_create(const mt3_engine_config* cfg, mt3_engine** out) {
  if (!cfg || !out) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: null argument");
  if (cfg->head_dim != 64) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: head_dim must be 64");
  if (cfg->compute_dtype != MT3_BF16 && cfg->compute_dtype != MT3_F32)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: compute_dtype must be MT3_BF16 or MT3_F32");
  if (cfg->input_length != 256 && cfg->input_length != 512)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: input_length must be 256 (mt3) or 512 (ismir2021)");
  if (cfg->emb_dim % 128 || cfg->mlp_dim % 128 || cfg->vocab_size % 128 || cfg->input_depth % 64 ||
      (cfg->num_heads * 64) % 128)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: emb/mlp/vocab/heads*64 must be multiples of 128");
  if (cfg->decode_chains < 0 || cfg->decode_chains > kMaxChains)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: decode_chains must be in [0, 8]");
  if (cfg->max_batch <= 0 || cfg->max_decode_len <= 0 || cfg->max_decode_len > kMaxPos ||
      cfg->num_encoder_layers <= 0 || cfg->num_decoder_layers <= 0)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: bad sizes");
  if (cfg->kv_cache_dtype != 0 && cfg->kv_cache_dtype != MT3_FP8_E4M3)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: kv_cache_dtype must be 0 (= compute dtype) or MT3_FP8_E4M3");
  if (cfg->kv_cache_dtype == MT3_FP8_E4M3 && cfg->compute_dtype != MT3_BF16)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: the fp8 K/V caches go with compute_dtype MT3_BF16");
  if (cfg->dense_dtype != 0 && cfg->dense_dtype != MT3_FP8_E4M3)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: dense_dtype must be 0 (= compute dtype) or MT3_FP8_E4M3");
  if (cfg->dense_dtype == MT3_FP8_E4M3 && (cfg->compute_dtype != MT3_BF16 || cfg->emb_dim > 1024))
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: the MXFP8 dense path goes with compute_dtype MT3_BF16 and emb_dim <= 1024");
  if (cfg->options & ~(MT3_OPT_SINGLE_RESIDUAL_STREAM | MT3_OPT_SEPARATE_PROJECTIONS | MT3_OPT_ENCODER_SINGLE_RESIDUAL_STREAM |
                       MT3_OPT_SEPARATE_QKV_PROJECTION | MT3_OPT_NO_ROW_GROUPS | MT3_OPT_ENCODER_F32_MFMA | MT3_OPT_SPIN_WAITS))
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_create: unknown bit in options");
  mt3_engine* e = new (std::nothrow) mt3_engine();
  if (!e) return mt3::fail(MT3_ERR_INVALID, "out of host memory");
  e->cfg = *cfg;
  if (hipGetDevice(&e->device) != hipSuccess) {
    (void)hipGetLastError();
    e->device = 0;                 // no GPU: the failure is reported by the first call that needs one (finalize)
  }
  e->dense_fp8 = cfg->dense_dtype == MT3_FP8_E4M3;
  e->x6 = cfg->compute_dtype == MT3_F32 && !(cfg->options & MT3_OPT_ENCODER_F32_MFMA);
  e->spin_waits = (cfg->options & MT3_OPT_SPIN_WAITS) != 0;
  e->esize = cfg->compute_dtype == MT3_BF16 ? 2 : 4;
  e->kv_fp8 = cfg->kv_cache_dtype == MT3_FP8_E4M3;
  e->kv_esize = e->kv_fp8 ? 1 : e->esize;
  *out = e;
  return MT3_OK;
}

void mt3_engine_destroy(mt3_engine* e) {
  if (!e) return;
  workers_stop(e);                 // joins a decode that is still in flight
  drop_group_graphs(e);
  for (int k = 0; k < kMaxChains; ++k) {
    if (e->cap_stream[k]) (void)hipStreamDestroy(e->cap_stream[k]);
    if (e->cap_event[k]) (void)hipEventDestroy(e->cap_event[k]);
  }
  for (int g = 0; g < kMaxGroups; ++g)
    if (e->part_stream[g]) (void)hipStreamDestroy(e->part_stream[g]);
  if (e->part_begin) (void)hipEventDestroy(e->part_begin);
  for (auto& pair : e->wait_ev)
    for (hipEvent_t ev : pair)
      if (ev) (void)hipEventDestroy(ev);
  if (e->h_pinned) (void)hipHostFree(e->h_pinned);
  for (void* p : e->allocs) (void)hipFree(p);
  delete e;
}

int mt3_engine_load_weight(mt3_engine* e, const char* name, const float* h_data, const int64_t* shape, int32_t ndim) {
  if (!e || !name || !h_data || !shape || ndim < 1 || ndim > 2)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_load_weight: bad arguments");
  if (e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_load_weight: engine already finalized");
  HostWeight w;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] <= 0) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_load_weight: bad shape");
    w.shape.push_back(shape[i]);
    n *= static_cast<size_t>(shape[i]);
  }
  w.data.assign(h_data, h_data + n);
  e->raw[name] = std::move(w);
  return MT3_OK;
}

int64_t mt3_engine_device_bytes(const mt3_engine* e) { return e ? e->device_bytes : 0; }

int mt3_engine_finalize(mt3_engine* e) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_finalize: null engine");
  if (e->finalized) return MT3_OK;
  const mt3_engine_config& c = e->cfg;
  const int emb = c.emb_dim, hd = e->HD(), Bm = c.max_batch, T = c.input_length, L = c.max_decode_len;
  int rc;

  // ---- encoder
  {
    const HostWeight* w = find(e, "encoder/continuous_inputs_projection/kernel", c.input_depth, emb);
    if (!w) return MT3_ERR_MISSING;
    std::vector<float> t(static_cast<size_t>(emb) * c.input_depth);
    put_transposed(t, c.input_depth, 0, *w, nullptr);
    if ((rc = upload_dense(e, t, emb, c.input_depth, kFormPlanes, &e->enc_in))) return rc;
  }
  e->enc.resize(c.num_encoder_layers);
  for (int l = 0; l < c.num_encoder_layers; ++l) {
    const std::string P = "encoder/layers_" + std::to_string(l);
    const float* s1 = scale_of(e, P + "/pre_attention_layer_norm/scale");
    const float* s2 = scale_of(e, P + "/pre_mlp_layer_norm/scale");
    if (!s1 || !s2) return MT3_ERR_MISSING;
    if ((rc = build_attention(e, P + "/attention", s1, false, &e->enc[l], true))) return rc;
    if ((rc = build_mlp(e, P + "/mlp", s2, &e->enc[l], true))) return rc;
  }
  {
    const HostWeight* w = find(e, "encoder/encoder_norm/scale", emb, -1);
    if (!w) return MT3_ERR_MISSING;
    if ((rc = upload_f32(e, w->data, &e->enc_norm))) return rc;
  }
  // ---- decoder
  {
    const HostWeight* w = find(e, "decoder/token_embedder/embedding", c.vocab_size, emb);
    if (!w) return MT3_ERR_MISSING;
    if ((rc = upload_f32(e, w->data, &e->embedding))) return rc;
  }
  e->dec.resize(c.num_decoder_layers);
  const bool single_stream = (c.options & MT3_OPT_SINGLE_RESIDUAL_STREAM) != 0;
  // (emb = 768, the ismir2022/base.gin shape: the split residual form exists for the bf16 tiles only -- their 48 partial
  // sums fit the NPV = 16 registers; an f32 engine of that shape keeps the single f32 stream with in-kernel statistics)
  const bool q_fold = emb % 64 == 0 && (emb <= 512 || (emb == 768 && c.compute_dtype == MT3_BF16)) && !single_stream &&
                      !(c.options & MT3_OPT_SEPARATE_PROJECTIONS);
  e->q_fold = q_fold;
  // qkv-fold (the fold launch's 32-column tiles need whole tiles of logits columns)
  e->qkv_fold = q_fold && !(c.options & MT3_OPT_SEPARATE_QKV_PROJECTION) && emb % 512 == 0 && c.mlp_dim % 512 == 0 &&
                c.vocab_size % 32 == 0;
  std::vector<std::vector<float>> dec_wi(e->qkv_fold ? c.num_decoder_layers : 0);
  for (int l = 0; l < c.num_decoder_layers; ++l) {
    const std::string P = "decoder/layers_" + std::to_string(l);
    const float* s1 = scale_of(e, P + "/pre_self_attention_layer_norm/scale");
    const float* s2 = scale_of(e, P + "/pre_cross_attention_layer_norm/scale");
    const float* s3 = scale_of(e, P + "/pre_mlp_layer_norm/scale");
    if (!s1 || !s2 || !s3) return MT3_ERR_MISSING;
    if ((rc = build_attention(e, P + "/self_attention", s1, false, &e->dec[l]))) return rc;
    if ((rc = build_attention(e, P + "/encoder_decoder_attention", s2, true, &e->dec[l]))) return rc;
    if (q_fold && (rc = build_q_fold(e, l, s2, &e->dec[l]))) return rc;
    if ((rc = build_mlp(e, P + "/mlp", s3, &e->dec[l], false, e->qkv_fold ? &dec_wi[l] : nullptr))) return rc;
    const size_t kvb = static_cast<size_t>(Bm) * c.num_heads * L * 64 * e->kv_esize;
    if ((rc = dmalloc(e, &e->dec[l].self_k, kvb))) return rc;
    if ((rc = dmalloc(e, &e->dec[l].self_v, kvb))) return rc;
    // zero-filled once: the decode-attention kernels request their first key group before they know the row's
    // length and mask what lies past it -- those bytes must be finite (0 x NaN would poison the accumulators)
    MT3_HIP_CHECK(hipMemset(e->dec[l].self_k, 0, kvb));
    MT3_HIP_CHECK(hipMemset(e->dec[l].self_v, 0, kvb));
    if ((rc = dmalloc(e, &e->dec[l].cross_kv, static_cast<size_t>(2) * Bm * c.num_heads * T * 64 * e->kv_esize)))
      return rc;
    if (e->kv_fp8) {
      if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->dec[l].self_scale),
                        static_cast<size_t>(Bm) * c.num_heads * L * sizeof(float2))))
        return rc;
      MT3_HIP_CHECK(hipMemset(e->dec[l].self_scale, 0, static_cast<size_t>(Bm) * c.num_heads * L * sizeof(float2)));
      if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->dec[l].cross_scale),
                        static_cast<size_t>(Bm) * c.num_heads * T * sizeof(float2))))
        return rc;
    }
  }
  if (e->kv_fp8 && (rc = dmalloc(e, &e->cross_stage, static_cast<size_t>(2) * Bm * c.num_heads * T * 64 * 2))) return rc;
  {
    const float* sn = scale_of(e, "decoder/decoder_norm/scale");
    const HostWeight* w = find(e, "decoder/logits_dense/kernel", emb, c.vocab_size);
    if (!sn || !w) return MT3_ERR_MISSING;
    std::vector<float> t(static_cast<size_t>(c.vocab_size) * emb);
    put_transposed(t, emb, 0, *w, sn);
    if ((rc = upload_dense(e, t, c.vocab_size, emb, 0, &e->logits_w))) return rc;
  }
  // ---- sinusoidal table (layers.py:51-82): [sin | cos] halves, scale = -ln(10000)/(emb/2 - 1)
  {
    std::vector<float> pe(static_cast<size_t>(kMaxPos) * emb);
    const int half = emb / 2;
    const double sf = -std::log(10000.0) / (half - 1);
    for (int p = 0; p < kMaxPos; ++p)
      for (int j = 0; j < half; ++j) {
        const double div = std::exp(j * sf);
        pe[static_cast<size_t>(p) * emb + j] = static_cast<float>(std::sin(p * div));
        pe[static_cast<size_t>(p) * emb + half + j] = static_cast<float>(std::cos(p * div));
      }
    if ((rc = upload_f32(e, pe, &e->pos_table))) return rc;
  }
  // ---- qkv-fold (needs the embedding and the position table on the device, and the raw weights still on the host)
  if (e->qkv_fold && (rc = build_qkv_fold(e, dec_wi))) return rc;
  dec_wi.clear();
  // ---- workspaces
  const size_t M = static_cast<size_t>(Bm) * T;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->x), M * emb * 4))) return rc;
  e->x_split = c.compute_dtype == MT3_BF16 && emb % 64 == 0 && emb <= 1024 &&
               !(c.options & MT3_OPT_ENCODER_SINGLE_RESIDUAL_STREAM) && !e->dense_fp8;
  if (e->x_split) {
    if ((rc = dmalloc(e, &e->x_ct, M * emb * 2))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->x_ss), M * (emb / 16) * 4))) return rc;
  }
  if (e->dense_fp8) {
    if (!e->x_ss && (rc = dmalloc(e, reinterpret_cast<void**>(&e->x_ss), M * (emb / 16) * 4))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->x_q), M * emb))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->x_sc), M * (emb / 32)))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->attn_q), M * hd))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->attn_sc), M * (hd / 32)))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->h_q), M * c.mlp_dim))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->h_sc), M * (c.mlp_dim / 32)))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->enc_q), M * emb))) return rc;
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->enc_sc), M * (emb / 32)))) return rc;
  }
  if ((rc = dmalloc(e, &e->qkv, M * 3 * hd * e->esize))) return rc;
  if ((rc = dmalloc(e, &e->attn, M * hd * e->esize))) return rc;
  if ((rc = dmalloc(e, &e->hbuf, M * c.mlp_dim * e->esize))) return rc;
  if ((rc = dmalloc(e, &e->enc_out, M * emb * e->esize))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->y), static_cast<size_t>(Bm) * emb * 4))) return rc;
  // the split residual form in the decode loop.  bf16: f32 rows + bf16 copy + per-16-column sums of squares; f32 (round
  // 3): the compute-type rows ARE the f32 rows, so only the sums travel with them (y_ct aliases y and is never written
  // as a copy) -- the norm-fused GEMMs then need no statistics pass and the folded projections work as in bf16
  e->y_split = emb % 64 == 0 && (emb <= 512 || (emb == 768 && c.compute_dtype == MT3_BF16)) && !single_stream;
  if (e->y_split) {
    if (c.compute_dtype == MT3_BF16) {
      if ((rc = dmalloc(e, &e->y_ct, static_cast<size_t>(Bm) * emb * 2))) return rc;
    } else {
      e->y_ct = e->y;
    }
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->y_ss), static_cast<size_t>(Bm) * (emb / 16) * 4))) return rc;
  }
  if (e->q_fold && !e->y_split) e->q_fold = false;
  if (!e->q_fold) e->qkv_fold = false;
  if (e->q_fold && (rc = dmalloc(e, reinterpret_cast<void**>(&e->qf), static_cast<size_t>(Bm) * hd * 4))) return rc;
  if (e->qkv_fold && (rc = dmalloc(e, reinterpret_cast<void**>(&e->qkvf), static_cast<size_t>(Bm) * 4 * hd * 4))) return rc;
  if ((rc = dmalloc(e, &e->qkv_d, static_cast<size_t>(Bm) * 3 * hd * e->esize))) return rc;
  if ((rc = dmalloc(e, &e->attn_d, static_cast<size_t>(Bm) * hd * e->esize))) return rc;
  if ((rc = dmalloc(e, &e->q_d, static_cast<size_t>(Bm) * hd * e->esize))) return rc;
  if ((rc = dmalloc(e, &e->h_d, static_cast<size_t>(Bm) * c.mlp_dim * e->esize))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->logits), static_cast<size_t>(Bm) * c.vocab_size * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->ids), static_cast<size_t>(Bm) * L * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->cur_tok), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->done), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->step), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->n_done), 4 * kMaxChains))) return rc;   // one counter per row group
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->forced), static_cast<size_t>(Bm) * L * 4))) return rc;
  // row retirement: slot map, synthetic EOS schedule, compaction scratch
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->slot_row), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->eos_at), static_cast<size_t>(Bm) * 4))) return rc;
  e->eos_cap = Bm;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->slot_seg), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->cs_seg), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->refill_plan), (static_cast<size_t>(Bm) + kMaxChains) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->cs_y), static_cast<size_t>(Bm) * emb * 4))) return rc;
  if (e->y_split && c.compute_dtype == MT3_BF16 && (rc = dmalloc(e, &e->cs_y_ct, static_cast<size_t>(Bm) * emb * 2))) return rc;
  if (e->y_split && (rc = dmalloc(e, reinterpret_cast<void**>(&e->cs_y_ss), static_cast<size_t>(Bm) * (emb / 16) * 4))) return rc;
  if (e->qkv_fold && (rc = dmalloc(e, reinterpret_cast<void**>(&e->cs_qkvf), static_cast<size_t>(Bm) * 4 * hd * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->cs_int), static_cast<size_t>(Bm) * mt3k::kCompactInts * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->gram), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->cs_beam), static_cast<size_t>(Bm) * 2 * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->cs_perm), (static_cast<size_t>(Bm) + kMaxChains) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->beam_f), static_cast<size_t>(2) * Bm * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->beam_len), static_cast<size_t>(Bm) * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->beam_len_row), static_cast<size_t>(Bm) * 4))) return rc;
  {
    // beam_cfg[0]: loop bound of the current call; beam_cfg[1 + n] = brevity_penalty(n), n = 0 .. L + 1
    const std::vector<float> bp = mt3k::brevity_table(L);
    if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->beam_cfg), bp.size() * 4))) return rc;
    MT3_HIP_CHECK(hipMemcpy(e->beam_cfg, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
  }
  MT3_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_pinned), 64, hipHostMallocDefault));
  e->h_pinned[kForksPinned] = 0;
  e->raw.clear();
  e->finalized = true;
  return MT3_OK;
}

// Where an encoder pass leaves the cross-attention K/V of its batch: the engine's caches (rows 0 .. batch - 1: what
// mt3_engine_encode does), or a staging chunk of mt3_engine_transcribe ([2][batch][H][T][64] per layer, scales [batch][H][T])
struct CrossDst {
  void* const* kv = nullptr;         // per decoder layer (nullptr: the caches)
  float2* const* scale = nullptr;
};

static int encode_impl(mt3_engine* e, const float* d_inputs, int32_t batch, float* d_encoded_f32, const CrossDst& dst,
                       hipStream_t s) {
  const mt3_engine_config& c = e->cfg;
  auto ckv = [&](int l) -> void* { return dst.kv ? dst.kv[l] : e->dec[l].cross_kv; };
  auto csc = [&](int l) -> float2* { return dst.scale ? dst.scale[l] : e->dec[l].cross_scale; };
  const int dt = c.compute_dtype, emb = c.emb_dim, hd = e->HD(), T = c.input_length;
  const int M = batch * T;
  const bool small = M < 2048;
  // f32 engine (R.x6): every dense layer and the attention on the bf16 pipes with three planes per operand (gemm.hip,
  // gemm_x6_kernel: at least as exact as the f32 matrix instruction, 2.7x its rate).  Since round 5 at EVERY batch size
  // (up to round 4 passes of fewer than 2048 rows took the f32 instruction's decode-sized tiles, so a segment's f32
  // encoder output depended on the batch it sat in by ~1e-7 -- ADVICE r4): a file's last short batch, a refill chunk of
  // mt3_engine_transcribe and a 1250-segment corpus call now give a segment the same bits
  const Resid R = encoder_rows(e, M, small);
  {
    mt3k::GemmArgs g = gemm_args(d_inputs, e->enc_in, e->x, M, emb);
    g.aux = e->pos_table;
    g.seq_len = T;
    MT3_TRY(dense_gemm(e, R.x6, g, e->enc_in, true, 0, MT3_EPI_POS, small, s));
  }
  if (e->dense_fp8) {
    // MXFP8 encoder: x travels as f32 rows + e4m3/E8M0 copy + per-16-column sums of squares; every GEMM operand is
    // MXFP8, written in that form by its producer (the quantiser below, the RESID / GEGLU epilogues)
    auto mx = [&](const uint8_t* A, const uint8_t* a_sc, const Dense& W) {
      mt3k::Mx8Args g{};
      g.A = A;
      g.a_sc = a_sc;
      g.W = W.q;
      g.w_sc = W.sc;
      g.M = M;
      g.N = W.N;
      g.K = W.K;
      g.ldo = W.N;
      return g;
    };
    auto mx_add = [&](const uint8_t* A, const uint8_t* a_sc, const Dense& W) {
      mt3k::Mx8Args g = mx(A, a_sc, W);
      g.out = e->x;
      g.out_q = e->x_q;
      g.out_sc = e->x_sc;
      g.out_ss = e->x_ss;
      return mt3k::launch_gemm_mx8(g, MT3_EPI_RESID, s);
    };
    MT3_TRY(mt3k::launch_mx8_quantize(e->x, true, M, emb, e->x_q, e->x_sc, e->x_ss, s));
    for (int l = 0; l < c.num_encoder_layers; ++l) {
      LayerDev& L = e->enc[l];
      {
        mt3k::Mx8Args g = mx(e->x_q, e->x_sc, L.wqkv);
        g.out = e->qkv;
        g.a_ss = e->x_ss;
        MT3_TRY(mt3k::launch_gemm_mx8(g, MT3_EPI_STORE, s));
      }
      MT3_TRY(mt3k::launch_encoder_attention(dt, e->qkv, e->attn, batch, T, c.num_heads, s));
      MT3_TRY(mt3k::launch_mx8_quantize(e->attn, false, M, hd, e->attn_q, e->attn_sc, nullptr, s));
      MT3_TRY(mx_add(e->attn_q, e->attn_sc, L.wo));
      {
        mt3k::Mx8Args g = mx(e->x_q, e->x_sc, L.wi);
        g.ldo = c.mlp_dim;
        g.a_ss = e->x_ss;
        g.out_q = e->h_q;
        g.out_sc = e->h_sc;
        MT3_TRY(mt3k::launch_gemm_mx8(g, MT3_EPI_GEGLU, s));
      }
      MT3_TRY(mx_add(e->h_q, e->h_sc, L.wo_mlp));
    }
    MT3_TRY(mt3k::launch_rmsnorm(dt, e->x, e->enc_norm, e->enc_out, d_encoded_f32, M, emb, s));
    MT3_TRY(mt3k::launch_mx8_quantize(e->enc_out, false, M, emb, e->enc_q, e->enc_sc, nullptr, s));
    for (int l = 0; l < c.num_decoder_layers; ++l) {
      mt3k::Mx8Args g = mx(e->enc_q, e->enc_sc, e->dec[l].wkv_x);
      g.out = e->kv_fp8 ? e->cross_stage : ckv(l);
      g.seq_len = T;
      MT3_TRY(mt3k::launch_gemm_mx8(g, MT3_EPI_HEADS, s));
      if (e->kv_fp8)
        MT3_TRY(mt3k::launch_kv_quantize_fp8(e->cross_stage, ckv(l), csc(l),
                                             batch * c.num_heads * T, s));
    }
    return MT3_OK;
  }
  if (R.split) MT3_TRY(mt3k::launch_residual_split(e->x, e->x_ct, e->x_ss, M, emb, s));
  for (int l = 0; l < c.num_encoder_layers; ++l) {
    LayerDev& L = e->enc[l];
    MT3_TRY(normed_gemm(e, R, L.wqkv, e->qkv, 3 * hd, MT3_EPI_STORE, small, s));
    if (R.x6) MT3_TRY(mt3k::launch_encoder_attention_x6(e->qkv, e->attn, batch, T, c.num_heads, s));
    else MT3_TRY(mt3k::launch_encoder_attention(dt, e->qkv, e->attn, batch, T, c.num_heads, s));
    MT3_TRY(resid_gemm(e, L.wo, e->attn, R, small, s));
    MT3_TRY(normed_gemm(e, R, L.wi, e->hbuf, c.mlp_dim, MT3_EPI_GEGLU, small, s));
    MT3_TRY(resid_gemm(e, L.wo_mlp, e->hbuf, R, small, s));
  }
  MT3_TRY(mt3k::launch_rmsnorm(dt, e->x, e->enc_norm, e->enc_out, d_encoded_f32, M, emb, s));
  for (int l = 0; l < c.num_decoder_layers; ++l) {
    const Dense& W = e->dec[l].wkv_x;
    mt3k::GemmArgs g = gemm_args(e->enc_out, W, e->kv_fp8 ? e->cross_stage : ckv(l), M, 2 * hd);
    g.seq_len = T;
    MT3_TRY(dense_gemm(e, R.x6, g, W, false, 0, MT3_EPI_HEADS, small, s));
    if (e->kv_fp8)     // bf16 [2][B][H][T][64] -> e4m3 rows + one power-of-two scale per (row, head, position)
      MT3_TRY(mt3k::launch_kv_quantize_fp8(e->cross_stage, ckv(l), csc(l),
                                           batch * c.num_heads * T, s));
  }
  return MT3_OK;
}

int mt3_engine_encode(mt3_engine* e, const float* d_inputs, int32_t batch, float* d_encoded_f32, void* stream) {
  if (!e || !e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_encode: engine not finalized");
  if (!d_inputs || batch <= 0 || batch > e->cfg.max_batch)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_encode: batch out of range");
  if (e->pending.active)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_encode: a decode is in flight (MT3_DECODE_ASYNC): call mt3_engine_decode_wait first");
  MT3_TRY(encode_impl(e, d_inputs, batch, d_encoded_f32, CrossDst{}, static_cast<hipStream_t>(stream)));
  e->cur_batch = batch;
  return MT3_OK;
}

// ---------------------------------------------------------------------------------------------- the decode loop
// Row groups of the product decode schedule (mt3_engine::part_stream).  Measured on MI355X, ms per 1024-step decode,
// 1 / 2 / 4 groups (profiles/r3_ab_row_groups_*.txt): bf16 B = 256: 626 / 588 / 608, B = 512: 1113 / 1048 / 1013;
// f32 B = 128: 747 / 684 / 737, B = 256: 1178 / 1132 / 1098 -- groups of ~128 rows for bf16 operands, ~64 for f32.
// (Three groups are never better than two or four.  EIGHT groups of 32 rows -- round 4, f32, B = 256: 2307 ms against
// 1098 with four, the EOS-schedule decode 1052 against 380 ms, profiles/r4_ab_eight_row_groups.txt.  The cliff is at
// exactly FIVE: 5 / 6 groups 2421 / 2306 ms against 1106 with four (3: 1144), the same with GPU_MAX_HW_QUEUES=8 in the
// environment, profiles/r4_ab_five_six_row_groups.txt -- as if a fifth busy queue shared one of four compute pipes with
// another one and the two took turns (the decode waits for a group running at half speed).  Four it is.)
// Under MT3_DECODE_EARLY_EXIT (the ragged regime: rows retire, the step is launch latency, not bandwidth) f32 follows
// the bf16 rule: at B = 256 two groups 370.5 ms, four 380.7, one stream 377.5 (profiles/r4_ab_tall_tiles_groups_wait.txt,
// profiles/r4_bench_driver_like.json eos_schedule); bf16 two groups 212.3 against 220.0 on one stream.
static int row_groups_for(const mt3_engine_config& c, int batch, bool early_exit = false) {
  const bool f32 = c.compute_dtype != MT3_BF16;
  // (round 6, with the dense tiles' priority in place: four groups under early exit from 256 f32 rows on -- 368-372 ms per
  // EOS-schedule decode against 362-367 with two: profiles/r6_ab_priorities_and_kernarg_pin.txt, block 4; the rule stays)
  if (batch >= (f32 && !early_exit ? 256 : 512)) return 4;
  return batch >= 128 ? 2 : 1;
}

// Row groups of a streaming job (mt3_engine_transcribe, _transcribe_beams, _transcribe_draws) over `units` units of `unit` slots:
// in-flight batching keeps every group's rows full, so the rule of the canonical full-length schedule applies, not the
// ragged one's; a group holds whole units and at least 16 slots (groups_override > 0: mt3_debug_engine_transcribe's choice)
static int stream_groups_for(const mt3_engine_config& c, int flags, int units, int unit, int groups_override) {
  const bool one = (flags & MT3_DECODE_SINGLE_STREAM) || (c.options & MT3_OPT_NO_ROW_GROUPS);
  int groups = groups_override > 0 ? groups_override : one ? 1 : row_groups_for(c, units * unit);
  while (groups > 1 && (units / groups) * unit < 16) --groups;
  return groups;
}

// ---- persistent group workers
static void worker_main(Worker* w, int dev) {
  (void)hipSetDevice(dev);
  std::unique_lock<std::mutex> lk(w->mu);
  for (;;) {
    w->cv.wait(lk, [&] { return w->has_job || w->quit; });
    if (!w->has_job) return;                       // quit (a posted job is always run first)
    std::function<void()> job = std::move(w->job);
    lk.unlock();
    try {
      job();
    } catch (...) {                                // nothing may leave a thread of a C library
    }
    lk.lock();
    w->has_job = false;
    w->cv.notify_all();
  }
}

// false: the worker thread could not be created (the caller falls back to the calling thread)
static bool worker_post(mt3_engine* e, int g, std::function<void()> fn) {
  if (!e->workers[g]) {
    Worker* w = new (std::nothrow) Worker();
    if (!w) return false;
    try {
      w->th = std::thread(worker_main, w, e->device);
    } catch (...) {
      delete w;
      return false;
    }
    e->workers[g] = w;
  }
  Worker* w = e->workers[g];
  {
    std::lock_guard<std::mutex> lk(w->mu);
    w->job = std::move(fn);
    w->has_job = true;
  }
  w->cv.notify_all();
  return true;
}

static void worker_wait(mt3_engine* e, int g) {
  Worker* w = e->workers[g];
  if (!w) return;
  std::unique_lock<std::mutex> lk(w->mu);
  w->cv.wait(lk, [&] { return !w->has_job; });
}

static void workers_stop(mt3_engine* e) {
  for (int g = 0; g < kMaxGroups; ++g) {
    Worker* w = e->workers[g];
    if (!w) continue;
    {
      std::unique_lock<std::mutex> lk(w->mu);
      w->cv.wait(lk, [&] { return !w->has_job; });
      w->quit = true;
    }
    w->cv.notify_all();
    if (w->th.joinable()) w->th.join();
    delete w;
    e->workers[g] = nullptr;
  }
}

// every captured step graph: what a setup call does when a graph may hold an address or a constant it replaces
static void drop_group_graphs(mt3_engine* e) {
  for (GroupGraph& g : e->group_graphs) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
  }
  e->group_graphs.clear();
}

// One row group's decode loop: slots [row0, row0 + rows) of a `batch`-row decode on stream `s` (the single-stream
// schedule is the group [0, batch) on the caller's stream).
struct GroupRun {
  int row0, rows, batch, variant, num_steps, slot;
  bool early, use_graph;
  hipStream_t s;
  float* d_first_logits;      // single-stream schedule only
  float* d_step_logits;
  int ran;
  bool used_graph;
  int chains = 1;             // graph chains of every step (GroupJob::chains)
};

// The captured step of the first `rows` slots of group r (nullptr: capture failed, the caller launches directly).
// Captured on engine-owned streams in thread-local mode -- several group threads may be here at once, so graph_mu is held
// throughout: it guards the cache and the capture streams.  A step of one chain is captured on the group's own stream.
// A step of several is the only graph here with parallel branches: chain k is captured on cap_stream[k], which joins the
// capture by waiting for an event of the origin (cap_stream[0]) and is joined back to it through an event of its own.
static hipGraphExec_t group_graph(mt3_engine* e, const GroupRun& r, int rows) {
  std::lock_guard<std::mutex> lk(e->graph_mu);
  const int max_len = (r.variant & kVarStream) ? e->stream_max_len : 0;    // baked into the step's token kernel
  for (const GroupGraph& g : e->group_graphs)
    if (g.variant == r.variant && g.batch == r.batch && g.row0 == r.row0 && g.rows == rows && g.slot == r.slot &&
        g.max_len == max_len && g.chains == r.chains)
      return g.exec;
  const int n = r.chains;
  hipStream_t* cs = e->cap_stream + (n > 1 ? 0 : r.slot);
  hipError_t he = hipSuccess;
  for (int k = 0; k < n && he == hipSuccess; ++k) {
    if (!cs[k]) he = hipStreamCreateWithFlags(&cs[k], hipStreamNonBlocking);
    if (n > 1 && !e->cap_event[k] && he == hipSuccess) he = hipEventCreateWithFlags(&e->cap_event[k], hipEventDisableTiming);
  }
  if (he != hipSuccess || hipStreamBeginCapture(cs[0], hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  int rc = MT3_OK;
  if (n > 1) he = hipEventRecord(e->cap_event[0], cs[0]);                                        // fork
  for (int k = 1; k < n && he == hipSuccess; ++k) he = hipStreamWaitEvent(cs[k], e->cap_event[0], 0);
  for (int k = 0; k < n && he == hipSuccess && rc == MT3_OK; ++k)
    rc = enqueue_chain_step(e, r.row0, rows, r.batch, r.variant, n, k, cs[k], r.slot);
  for (int k = 1; k < n && he == hipSuccess && rc == MT3_OK; ++k) {                              // join
    he = hipEventRecord(e->cap_event[k], cs[k]);
    if (he == hipSuccess) he = hipStreamWaitEvent(cs[0], e->cap_event[k], 0);
  }
  hipGraph_t g = nullptr;
  hipGraphExec_t x = nullptr;
  const hipError_t end = hipStreamEndCapture(cs[0], &g);       // (fails, and ends the capture, if a chain was left unjoined)
  if (rc != MT3_OK || he != hipSuccess || end != hipSuccess || hipGraphInstantiate(&x, g, nullptr, nullptr, 0) != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    return nullptr;
  }
  e->group_graphs.push_back(GroupGraph{r.variant, r.batch, r.row0, rows, r.slot, max_len, n, g, x});
  return x;
}

// ---- sleeping waits (mt3_engine::wait_ev)
static hipEvent_t wait_event(mt3_engine* e, int slot, int which) {
  hipEvent_t& ev = e->wait_ev[slot][which];
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    ev = nullptr;
  }
  return ev;
}

// The calling thread SLEEPS until `ev` has happened: hipEventQuery between naps of 20 .. 200 us (measured in round 5:
// hipEventSynchronize spins a core for the length of the wait on this runtime even on an event created with
// hipEventBlockingSync -- the CPU seconds of a decode did not move -- so the nap is explicit).  The naps start short so
// that a poll's answer is picked up within tens of microseconds and grow while nothing happens.
static hipError_t sleep_until(hipEvent_t ev) {
  long nap_ns = 20000;
  for (;;) {
    const hipError_t he = hipEventQuery(ev);
    if (he != hipErrorNotReady) return he;
    (void)hipGetLastError();                               // NotReady is sticky in the thread's last-error slot
    std::this_thread::sleep_for(std::chrono::nanoseconds(nap_ns));
    if (nap_ns < 200000) nap_ns += nap_ns / 2;
  }
}

// everything enqueued on `s` so far has run; the calling thread sleeps meanwhile (spins with MT3_OPT_SPIN_WAITS or when
// no event could be created)
static hipError_t wait_stream(mt3_engine* e, int slot, hipStream_t s) {
  hipEvent_t ev = e->spin_waits ? nullptr : wait_event(e, slot, 0);
  if (!ev) return hipStreamSynchronize(s);
  hipError_t he = hipEventRecord(ev, s);
  return he == hipSuccess ? sleep_until(ev) : he;
}

// after step t has been enqueued: at the end of every window, sleep until the window before it is done (at most two
// windows of kThrottleWindow steps are ever enqueued ahead of the device: the runtime's own back-pressure, which spins,
// is never reached)
struct Throttle {
  mt3_engine* e;
  int slot;
  hipStream_t s;
  int recorded = 0;
  hipError_t tick(long t) {
    if (e->spin_waits || t % kThrottleWindow != kThrottleWindow - 1) return hipSuccess;
    hipEvent_t ev = wait_event(e, slot, 1);
    if (!ev) return hipSuccess;
    hipError_t he = hipSuccess;
    if (recorded) he = sleep_until(ev);                  // the window recorded one window ago
    if (he == hipSuccess) he = hipEventRecord(ev, s);
    recorded = 1;
    return he;
  }
};

static int compact_group(mt3_engine* e, const GroupRun& r, int cur) {
  const size_t r0 = static_cast<size_t>(r.row0);
  mt3k::CompactArgs a{};
  a.st = slot_state(e, r.row0, r.slot);
  a.in = input_row(e, r.row0);
  const size_t emb = a.in.dim, n4 = a.in.rp.q_n;
  if (r.variant & kVarBeam) {
    a.beam = beam1_state(e, r.row0, 0);
    a.s_beam = e->cs_beam + 2 * r0;
  }
  // scratch for the forms in use
  a.s_y = e->cs_y + r0 * emb;
  if (a.in.y_ct) a.s_y_ct = static_cast<char*>(e->cs_y_ct) + r0 * emb * 2;
  if (a.in.y_ss) a.s_y_ss = e->cs_y_ss + r0 * (emb / 16);
  if (a.in.rp.q_out) a.s_qkvf = e->cs_qkvf + r0 * n4;
  a.s_int = e->cs_int + mt3k::kCompactInts * r0;
  if (a.st.note) a.s_held = e->cs_held + r0 * a.st.held_words;
  a.perm = e->cs_perm + r0 + r.slot;
  a.rows = cur;
  if (r.variant & kVarStream) a.s_seg = e->cs_seg + r0;
  else a.st.slot_seg = nullptr;                           // no segments: the map does not travel
  return mt3k::launch_compact(a, r.s);
}

static int run_group(mt3_engine* e, GroupRun& r) {
  const mt3_engine_config& c = e->cfg;
  const bool retire = (r.variant & kVarRetire) != 0;
  const bool whole = r.row0 == 0 && r.rows == r.batch;
  int cur = r.rows;                              // slots in use: shrinks with the live rows in 32-row (GEMM tile) steps
  hipGraphExec_t exec = nullptr;
  int exec_rows = -1;
  r.ran = 0;
  r.used_graph = r.use_graph;
  const int wslot = r.s == e->part_stream[r.slot] ? r.slot : kMaxGroups;
  Throttle throttle{e, wslot, r.s};
  for (int t = 0; t < r.num_steps; ++t) {
    if (r.use_graph && exec_rows != cur) {
      exec = group_graph(e, r, cur);
      exec_rows = cur;
      if (!exec) {                               // direct launches give the same ids; the fallback is RECORDED
        r.use_graph = r.used_graph = false;
        ++e->graph_fallbacks;
      }
    }
    if (r.use_graph) MT3_HIP_CHECK(hipGraphLaunch(exec, r.s));
    else MT3_TRY(enqueue_step(e, r.row0, cur, r.batch, r.variant, r.chains, r.s, r.slot));
    ++r.ran;
    if (whole && t == 0 && r.d_first_logits)
      MT3_HIP_CHECK(hipMemcpyAsync(r.d_first_logits, e->logits, static_cast<size_t>(r.batch) * c.vocab_size * 4,
                                   hipMemcpyDeviceToDevice, r.s));
    if (whole && r.d_step_logits)
      MT3_HIP_CHECK(hipMemcpyAsync(r.d_step_logits + static_cast<size_t>(t) * r.batch * c.vocab_size, e->logits,
                                   static_cast<size_t>(r.batch) * c.vocab_size * 4, hipMemcpyDeviceToDevice, r.s));
    if (!r.early) MT3_HIP_CHECK(throttle.tick(t));
    if (r.early && t % 32 == 31) {
      // the poll: how many rows of THIS group are finished (every group stops as soon as its own rows are)
      MT3_HIP_CHECK(hipMemcpyAsync(e->h_pinned + r.slot, e->n_done + r.slot, 4, hipMemcpyDeviceToHost, r.s));
      MT3_HIP_CHECK(wait_stream(e, wslot, r.s));
      const int live = r.rows - e->h_pinned[r.slot];
      if (live <= 0) break;
      // beam groups stay where they are (their rows are k-slot units), and so do graph chains (the deal of the rows is
      // part of the captured step)
      if (retire && !(r.variant & kVarBeams) && r.chains == 1) {
        int want = (live + 31) & ~31;
        if (want > r.rows) want = r.rows;
        if (want < cur) {                        // the live rows fit fewer GEMM row tiles: move them to the front
          MT3_TRY(compact_group(e, r, cur));
          cur = want;
          ++e->compactions_now;
        }
      }
    }
  }
  return MT3_OK;
}

// hardware-queue streams of the row groups (see mt3_engine::part_stream); MT3_ERR_CAPACITY = could not be set up
static int ensure_group_streams(mt3_engine* e, int groups) {
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || n_cu < 2 * groups)
    return MT3_ERR_CAPACITY;
  for (int g = 0; g < groups; ++g) {
    if (e->part_stream[g]) continue;
    // a mask of ALL compute units: the stream is created through the CU-mask entry point for the hardware queue of
    // its own that comes with it, not to restrict it (see mt3_engine::part_stream)
    std::vector<uint32_t> mask((n_cu + 31) / 32, 0u);
    for (int i = 0; i < n_cu; ++i) mask[i >> 5] |= 1u << (i & 31);
    if (hipExtStreamCreateWithCUMask(&e->part_stream[g], static_cast<uint32_t>(mask.size()), mask.data()) != hipSuccess) {
      e->part_stream[g] = nullptr;
      (void)hipGetLastError();
      return MT3_ERR_CAPACITY;
    }
  }
  if (!e->part_begin && hipEventCreateWithFlags(&e->part_begin, hipEventDisableTiming) != hipSuccess)
    return MT3_ERR_CAPACITY;
  return MT3_OK;
}

using mt3feed::Feed;       // csrc/feed.h: the segment queue of the streaming jobs
using mt3feed::FeedRange;
using mt3feed::feed_fail;
using mt3feed::feed_pop;
using mt3feed::feed_release;
using mt3feed::feed_wait;

// ---- the scaffold every row-group job shares (mt3_engine_decode, _decode_beams, _transcribe, _transcribe_beams,
// _transcribe_draws)
// A job deals `units` units of `unit` slots each to `groups` row groups: greedy and beam-1 jobs have unit = 1, k-beam jobs
// unit = k, so that every group boundary is an element boundary.
struct GroupJob {
  int units, unit, groups, variant, num_steps;
  bool early, use_graph;
  bool own_streams;           // group g runs on part_stream[g] behind part_begin; false: the one group, on the caller's stream
  hipStream_t s;              // the caller's stream
  float* d_first_logits;      // (GroupRun: the caller's-stream schedule only)
  float* d_step_logits;
  int chains = 1;             // graph chains: every step of the one group on the caller's stream deals its rows to `chains`
                              // parallel branches of its graph (chains_for; launched directly they run back to back)
};

// What tells the three streaming entry points apart (run_stream_job; the k-beam job is the one whose variant has kVarBeams)
struct StreamJob {
  const char* who;            // the entry point's name
  int unit;                   // slots per element: k in the beam job, else 1
  int per;                    // feed entries per encoded segment: the draws of each in mt3_engine_transcribe_draws, else 1
  bool from_ring;             // every entry, the first ones included, reaches its slots through the staging ring: the groups
                              // start with every slot finished and empty (false: the first ones sit in the caches already)
  int32_t* d_ids;             // the caller's outputs, rows by feed entry ...
  int32_t* d_all_ids;         // ... and what only the beam job has (each may be nullptr)
  float* d_scores;
  int poll;                   // steps between refill polls
  bool skip_encoder;          // mt3_debug_engine_transcribe's differential timing (produce_chunks)
};

// Starts a job: the step-graph cache is trimmed (no worker is running here; the bound covers every kind of step graph,
// those of graph chains included) and e->pending is the job's
static PendingDecode& begin_job(mt3_engine* e) {
  if (e->group_graphs.size() > 96) drop_group_graphs(e);
  e->pending = PendingDecode();
  return e->pending;
}

// Group g of job j, on the calling thread: `loop` (run_group or run_group_stream) on the group's GroupRun; what it did
// goes to e->pending, and is returned.
using GroupLoop = std::function<int(GroupRun&)>;
static int run_one_group(mt3_engine* e, const GroupJob& j, int g, const GroupLoop& loop) {
  PendingDecode& q = e->pending;
  GroupRun r{};
  chain_rows(j.units, j.groups, g, &r.row0, &r.rows);
  r.row0 *= j.unit;
  r.rows *= j.unit;
  r.batch = j.units * j.unit;
  r.variant = j.variant | (j.groups > 1 ? kVarBeside : 0);
  r.chains = j.chains;
  r.num_steps = j.num_steps;
  r.slot = g;
  r.early = j.early;
  r.use_graph = j.use_graph;
  r.s = j.own_streams ? e->part_stream[g] : j.s;
  r.d_first_logits = j.d_first_logits;
  r.d_step_logits = j.d_step_logits;
  hipError_t he = j.own_streams ? hipStreamWaitEvent(r.s, e->part_begin, 0) : hipSuccess;
  if (he == hipSuccess) {
    q.rcs[g] = loop(r);
    if (q.rcs[g] != MT3_OK) q.errs[g] = mt3_last_error();
  }
  q.ran[g] = r.ran;
  q.used_graph[g] = r.used_graph;
  // The group's host thread WAITS for its stream.  Measured (r3, f32, B = 256, 4 groups): 1095 ms per 1024-step
  // decode when every group stream has a host thread in hipStreamSynchronize, 1166-1170 ms when only the
  // caller's stream (waiting for events of the groups) is synchronised -- a stream nobody waits on retires its
  // commands through the runtime's interrupt path.  (The caller's stream is the caller's to wait for.)
  if (j.own_streams && he == hipSuccess) he = wait_stream(e, g, r.s);
  if (q.rcs[g] == MT3_OK && he != hipSuccess) {
    q.rcs[g] = MT3_ERR_HIP;
    q.errs[g] = hipGetErrorString(he);
  }
  return q.rcs[g];
}

// Hands every group of job j to its worker thread.  feed == nullptr (the decodes): a group whose worker could not be
// started runs on the calling thread, after the posted ones started.  Otherwise (the streaming jobs, whose calling thread
// is the feed's producer): a group that fails fails the feed -- nobody may wait for its entries any more -- and false is
// returned as soon as a worker could not be started.
static bool post_groups(mt3_engine* e, const GroupJob& j, const GroupLoop& loop, Feed* feed) {
  PendingDecode& p = e->pending;
  p.groups = j.groups;
  p.active = true;                                       // every other entry point of the engine refuses meanwhile
  for (int g = 0; g < j.groups; ++g) {
    auto body = [e, j, g, loop, feed]() {
      if (run_one_group(e, j, g, loop) != MT3_OK && feed) feed_fail(*feed);
    };
    if (worker_post(e, g, body)) p.posted = g + 1;
    else if (feed) return false;
    else body();
  }
  return true;
}

// Joins the job in flight, entry point `who`'s: waits for its workers and folds what the groups left in e->pending into one
// outcome -- the first failed group's error, *most = the steps of the group that ran longest, and the engine's record of
// the most recent job (compactions, last_groups, last_used_graph)
static int join_groups(mt3_engine* e, const std::string& who, int* most) {
  PendingDecode& p = e->pending;
  for (int g = 0; g < p.posted; ++g) worker_wait(e, g);
  p.active = false;
  e->compactions = e->compactions_now.exchange(0);
  e->last_groups = p.groups;
  e->last_used_graph = 1;
  *most = 0;
  int rc = MT3_OK;
  for (int g = 0; g < p.groups; ++g) {
    if (rc == MT3_OK && p.rcs[g] != MT3_OK)
      rc = mt3::fail(p.rcs[g], who + " (row group " + std::to_string(g) + "): " + p.errs[g]);
    *most = p.ran[g] > *most ? p.ran[g] : *most;
    if (!p.used_graph[g]) e->last_used_graph = 0;
  }
  return rc;
}

// Joins the decode that is in flight, then (on the caller's stream) the beam-1 finalisation and the copy of the ids.
// Every group thread has waited for its stream, so the caller's stream needs no event.
static int decode_finish(mt3_engine* e, int32_t* h_steps_run) {
  PendingDecode& p = e->pending;
  if (!p.active) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_decode_wait: no decode in flight");
  int most = 0;
  MT3_TRY(join_groups(e, "mt3_engine_decode", &most));
  const int L = e->cfg.max_decode_len;
  if (p.beams) {
    // k-beam search: the results are walked back from the history straight into the caller's buffers
    mt3k::BeamKArgs b = beam_args(e, 0, p.batch * p.beams, p.beams);
    MT3_TRY(mt3k::launch_beam_finalize(b, L, p.num_steps, p.d_ids, p.d_all_ids, p.d_scores, p.s));
    MT3_HIP_CHECK(hipMemcpyAsync(e->h_pinned + kForksPinned, e->bk_forks, 4, hipMemcpyDeviceToHost, p.s));
  } else {
    if (p.beam1) MT3_TRY(mt3k::launch_beam1_finalize(e->ids, L, e->beam_len_row, p.batch, p.s));
    MT3_HIP_CHECK(hipMemcpyAsync(p.d_ids, e->ids, static_cast<size_t>(p.batch) * L * 4, hipMemcpyDeviceToDevice, p.s));
  }
  if (h_steps_run) *h_steps_run = most;
  return MT3_OK;
}

// ---- the start of a job, on the caller's stream
// the grammar state a slot starts in at position 0 (no grammar set: 0, which nothing reads)
static int grammar_initial(const mt3_engine* e) { return e->gr.on ? mt3g_initial(&e->gr.g) : 0; }

// Position 0 and BOS (= 0) for slots [0, n); `counters`: nothing finished (done flags, the groups' counters of finished
// slots), `ids`: zeroed id rows -- the jobs that start from the ring start every slot FINISHED (start_empty) and the
// k-beam jobs keep their ids in the history
static int reset_slots(mt3_engine* e, int n, bool counters, bool ids, hipStream_t s) {
  MT3_HIP_CHECK(hipMemsetAsync(e->step, 0, static_cast<size_t>(n) * 4, s));
  if (counters) MT3_HIP_CHECK(hipMemsetAsync(e->n_done, 0, 4 * kMaxChains, s));
  if (counters) MT3_HIP_CHECK(hipMemsetAsync(e->done, 0, static_cast<size_t>(n) * 4, s));
  MT3_HIP_CHECK(hipMemsetAsync(e->cur_tok, 0, static_cast<size_t>(n) * 4, s));
  if (e->gr.on)
    MT3_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->gram), grammar_initial(e), static_cast<size_t>(n), s));
  if (e->nt.on) {                // program 0, velocity non-zero, nothing held
    MT3_HIP_CHECK(hipMemsetAsync(e->note, 0, static_cast<size_t>(n) * 4, s));
    MT3_HIP_CHECK(hipMemsetAsync(e->nrow, 0, static_cast<size_t>(n) * MT3_NOTE_ROW_WORDS * 4, s));
    MT3_HIP_CHECK(hipMemsetAsync(e->held, 0, static_cast<size_t>(n) * mt3n_table_words(&e->nt.n) * 4, s));
  }
  if (ids) MT3_HIP_CHECK(hipMemsetAsync(e->ids, 0, static_cast<size_t>(n) * e->cfg.max_decode_len * 4, s));
  return MT3_OK;
}

// decoder input of step 0 for slots [0, n): Embed(BOS) + FixedEmbed[0]; later steps get theirs from the argmax kernel
static int embed_bos(mt3_engine* e, int n, hipStream_t s) {
  return mt3k::launch_embed(input_row(e, 0), e->cur_tok, e->step, n, s);
}

// t5x beam_search(alpha = 0.6) with one beam (MT3_DECODE_BEAM1): live log-prob 0, nothing finished; the loop bound uses
// the brevity penalty of num_steps + 1 (the dummy start token extends the length by one).  The value travels as a
// kernel argument: no host buffer has to stay alive behind an asynchronous copy.
static int reset_beam1_state(mt3_engine* e, int num_steps, hipStream_t s) {
  const size_t Bm = static_cast<size_t>(e->cfg.max_batch);
  MT3_TRY(mt3k::launch_set_float(e->beam_cfg, brevity_penalty(num_steps + 1), s));
  MT3_HIP_CHECK(hipMemsetAsync(e->beam_f, 0, 2 * Bm * 4, s));
  MT3_HIP_CHECK(hipMemsetAsync(e->beam_len, 0xFF, Bm * 4, s));   // -1
  MT3_HIP_CHECK(hipMemsetAsync(e->beam_len_row, 0xFF, Bm * 4, s));
  return MT3_OK;
}

// The masks, then the prompts, against a job of `n` rows / elements / segments: a step needs `need` candidates among a
// mask's allowed tokens, and a segment at least one free step of `num_steps` after its prompt; with a grammar set, every
// mask in use must leave `need` ids in the tie-section state and in the worst state after it (grammar_room).  MT3_OK and
// *var = the kVarMask / kVarPrompt / kVarGrammar bits of the job's step variant.
static int seg_tables_fit(const mt3_engine* e, const char* who, int n, int need, int num_steps, int* var) {
  MT3_TRY(fits(e->tm, who, n, need, INT_MAX, "the token masks'", ": a token mask in use allows fewer than 2 * num_beams tokens"));
  MT3_TRY(fits(e->tp, who, n, 0, num_steps - 1, "the prompts'", ": num_steps must exceed the longest prompt in use"));
  if (e->gr.on) {
    const int vocab = e->cfg.vocab_size;
    std::vector<char> seen(static_cast<size_t>(e->tm.n) + 1, 0);
    for (int i = 0; i < (e->tm.n && e->tm.seg_on ? n : 1); ++i) {
      const int r = !e->tm.n ? -1 : (e->tm.seg_on ? e->tm.seg_host[i] : 0);          // -1: no mask, the grammar alone
      if (seen[r + 1]) continue;
      seen[r + 1] = 1;
      int in_tie = 0, after = 0;
      mt3k::grammar_room(e->gr.g, r < 0 ? nullptr : e->tm.rows_host.data() + static_cast<size_t>(r) * e->tm.stride, vocab,
                         &in_tie, &after);
      if ((e->gr.g.with_ties && in_tie < need) || after < need)
        return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": the grammar and a token mask in use leave fewer than 2 * "
                                                             "num_beams ids in the tie section or after a shift");
      // the note rule's worst state after the tie section has no pitch and no drum id either
      if (e->nt.on &&
          mt3k::note_room_after(e->nt.n, r < 0 ? nullptr : e->tm.rows_host.data() + static_cast<size_t>(r) * e->tm.stride,
                                vocab) < need)
        return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": the note rule and a token mask in use leave fewer than 2 * "
                                                             "num_beams ids after a note-off marker with nothing held");
    }
  }
  *var = (e->tm.n ? kVarMask : 0) | (e->tp.n ? kVarPrompt : 0) | (e->gr.on ? kVarGrammar : 0) | (e->nt.on ? kVarNotes : 0);
  return MT3_OK;
}

// Temperature sampling against a greedy-path job of `n` rows / segments (the beam calls, teacher forcing and scoring ignore
// it): beam-1 does not sample, and a stream table and a seed table must cover the job.  MT3_OK and *var |= kVarSample where it is set.
static int sampling_fits(const mt3_engine* e, const char* who, int n, bool beam1, int* var) {
  if (!e->samp_on) return MT3_OK;
  if (beam1) return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": MT3_DECODE_BEAM1 does not sample (clear sampling first)");
  MT3_TRY(fits(e->sstream, who, n, 0, 0, "the sampling streams'", ": a sampling stream is out of range"));
  MT3_TRY(fits(e->sseed, who, n, 0, 0, "the sampling seeds'", ": a sampling seed is out of range"));
  *var |= kVarSample;
  return MT3_OK;
}

// ---- the preconditions the job entry points share, each refused as MT3_ERR_INVALID in the name of the entry point `who`
static int invalid(const char* who, const char* what) { return mt3::fail(MT3_ERR_INVALID, std::string(who) + ": " + what); }

// ready: finalized, and no job in flight
static int engine_ready(const mt3_engine* e, const char* who) {
  if (!e || !e->finalized) return invalid(who, "engine not finalized");
  if (e->pending.active) return invalid(who, "a decode is in flight (MT3_DECODE_ASYNC): call mt3_engine_decode_wait first");
  return MT3_OK;
}

static int steps_fit(const mt3_engine* e, const char* who, int num_steps) {
  if (num_steps <= 0 || num_steps > e->cfg.max_decode_len) return invalid(who, "num_steps out of range");
  return MT3_OK;
}

// what the beam step takes: 1 .. 8 beams that fit the engine, 2k candidates in a vocabulary of at most 2048 ids, and no
// more layers than a cache-row copy holds
static int beams_fit(const mt3_engine* e, const char* who, int k) {
  const mt3_engine_config& c = e->cfg;
  if (k < 1 || k > mt3k::kBeamMaxK) return invalid(who, "num_beams must be 1 .. 8");
  if (k > c.max_batch) return invalid(who, "num_beams exceeds max_batch");
  if (c.vocab_size > 2048 || c.vocab_size < 2 * k) return invalid(who, "the beam step needs 2 * num_beams <= vocab <= 2048");
  if (c.num_decoder_layers > mt3k::kRefillMaxLayers) return invalid(who, "more than 16 decoder layers");
  return MT3_OK;
}

// what a greedy-path streaming job of n feed entries takes: no more layers than a refill holds, and a synthetic EOS
// schedule (where one is set) with an entry for each
static int stream_fits(const mt3_engine* e, const char* who, int n) {
  if (e->cfg.num_decoder_layers > mt3k::kRefillMaxLayers) return invalid(who, "at most 16 decoder layers");
  if (e->eos_on && n > e->eos_cap) return invalid(who, "the synthetic EOS schedule is shorter than the job");
  return MT3_OK;
}

// The ending the two decodes share, for job j -- one group so far, its slots started on j.s.  Row groups on streams of
// their own where the slots, the flags and the engine's options allow it (caller_stream_only: the call needs what lives on
// the caller's stream), each group a whole number of units; else the one group on the caller's stream, on the calling
// thread -- or with MT3_DECODE_ASYNC on worker 0, if there is one to be had.  Then the job is joined (decode_finish), or
// with MT3_DECODE_ASYNC left to mt3_engine_decode_wait.
static int run_decode_job(mt3_engine* e, GroupJob j, int flags, bool caller_stream_only, int32_t* h_steps_run) {
  const mt3_engine_config& c = e->cfg;
  const bool async = (flags & MT3_DECODE_ASYNC) != 0;
  const GroupLoop loop = [e](GroupRun& r) { return run_group(e, r); };
  int groups = row_groups_for(c, j.units * j.unit, j.early);
  if (groups > j.units) groups = 1;
  if (groups > 1 && !caller_stream_only && !(flags & MT3_DECODE_SINGLE_STREAM) && !(c.options & MT3_OPT_NO_ROW_GROUPS)) {
    if (ensure_group_streams(e, groups) == MT3_OK) {
      MT3_HIP_CHECK(hipEventRecord(e->part_begin, j.s));
      j.groups = groups;
      j.own_streams = true;
    } else {
      ++e->part_failed;                           // the masked streams could not be created: single stream, recorded
    }
  }
  if (j.own_streams || async) {
    post_groups(e, j, loop, nullptr);
  } else {
    e->pending.active = true;
    run_one_group(e, j, 0, loop);
  }
  return async ? MT3_OK : decode_finish(e, h_steps_run);
}

// shared body of mt3_engine_decode / mt3_engine_decode_forced
static int decode_impl(mt3_engine* e, int32_t batch, int32_t num_steps, int32_t flags, int32_t debug_skip,
                       const int32_t* d_forced, float* d_step_logits, int32_t* d_ids, float* d_first_logits,
                       int32_t* h_steps_run, void* stream) {
  const char* who = "mt3_engine_decode";
  MT3_TRY(engine_ready(e, who));
  if (batch <= 0 || batch != e->cur_batch) return invalid(who, "batch must equal the batch of the preceding encode");
  const mt3_engine_config& c = e->cfg;
  MT3_TRY(steps_fit(e, who, num_steps));
  if (!d_ids) return invalid(who, "null ids");
  if (flags & ~(MT3_DECODE_NO_GRAPH | MT3_DECODE_EARLY_EXIT | MT3_DECODE_BEAM1 | MT3_DECODE_SINGLE_STREAM |
                MT3_DECODE_ASYNC | MT3_DECODE_CHAINS(0xF)))
    return invalid(who, "unknown flag bit");
  const bool beam1 = (flags & MT3_DECODE_BEAM1) != 0, early = (flags & MT3_DECODE_EARLY_EXIT) != 0;
  const bool async = (flags & MT3_DECODE_ASYNC) != 0;
  if (d_forced && (beam1 || early || async))
    return invalid("mt3_engine_decode_forced", "not combinable with BEAM1 / EARLY_EXIT / ASYNC");
  int seg_var = 0;                                       // teacher forcing ignores token masks and prompts
  if (!d_forced) MT3_TRY(seg_tables_fit(e, who, batch, 2, num_steps, &seg_var));
  if (!d_forced) MT3_TRY(sampling_fits(e, who, batch, beam1, &seg_var));
  hipStream_t s = static_cast<hipStream_t>(stream);
  MT3_TRY(reset_slots(e, batch, true, true, s));
  if (d_forced)    // engine-owned copy: the step graph holds ITS address, whatever buffer the caller passes
    MT3_HIP_CHECK(hipMemcpyAsync(e->forced, d_forced, static_cast<size_t>(batch) * c.max_decode_len * 4,
                                 hipMemcpyDeviceToDevice, s));
  MT3_TRY(embed_bos(e, batch, s));
  // Row retirement comes with the early exit: rows that have finished cost nothing from then on (mt3_hip.h).  Without
  // EARLY_EXIT every row runs every step -- the canonical full-length schedule the headline is quoted on.
  const bool retire = early && debug_skip == 0;
  if (retire) MT3_TRY(mt3k::launch_iota(e->slot_row, batch, s));

  // step variant: bits 1 / 2 = mt3_debug_engine_decode's skipped kernels (mt3_hip_debug.h; never set by the product
  // entry points), then kVar*
  const int variant = (debug_skip & 3) | (beam1 ? kVarBeam : 0) | (d_forced ? kVarForced : 0) | (retire ? kVarRetire : 0) |
                      (e->eos_on && !d_forced ? kVarEos : 0) | seg_var;
  if (beam1) MT3_TRY(reset_beam1_state(e, num_steps, s));
  PendingDecode& p = begin_job(e);
  p.beam1 = beam1;
  p.batch = batch;
  p.d_ids = d_ids;
  p.s = s;
  const bool use_graph = !(flags & MT3_DECODE_NO_GRAPH);
  // Graph chains come from the flags or the engine's decode_chains.  The row-group schedule (see mt3_engine::part_stream)
  // unless the caller asked for chains (one chain included) or gets them, or for what lives on the caller's stream:
  // skipped kernels, teacher forcing, logits
  const int req_chains = (flags >> 8) & 0xF, chains = chains_for(e, batch, req_chains);
  const GroupJob j{batch, 1, 1, variant, num_steps, early, use_graph, false, s, d_first_logits, d_step_logits, chains};
  return run_decode_job(e, j, flags,
                        req_chains != 0 || chains > 1 || debug_skip != 0 || d_forced || d_step_logits || d_first_logits,
                        h_steps_run);
}

// ----------------------------------------------------------------------------------------------- k-beam search
// mt3_engine_decode_beams: a GroupJob of k-slot units on run_group's loop, with the beam step (decode_ops.hip:
// beam_step_kernel + beam_reorder_kernel) as the last launches of every step.  Slots b*k .. b*k + k - 1 are the beams of element b; the
// slot -> cache-row map of row retirement is always in use (a beam takes over its parent's cache row), compaction
// never is (beam groups stay in place), and a retired element's k slots are `done` from the step after it retired.
static int ensure_beam_state(mt3_engine* e) {
  if (e->bk_live) return MT3_OK;
  const size_t Bm = static_cast<size_t>(e->cfg.max_batch), L = static_cast<size_t>(e->cfg.max_decode_len);
  int rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->bk_fin_score), Bm * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->bk_fin_step), Bm * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->bk_fin_beam), Bm * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->bk_fork_src), Bm * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->bk_forks), 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->bk_par), L * Bm * 4))) return rc;
  if ((rc = dmalloc(e, reinterpret_cast<void**>(&e->bk_tok), L * Bm * 4))) return rc;
  return dmalloc(e, reinterpret_cast<void**>(&e->bk_live), Bm * 4);     // last: it marks the set as complete
}

// The start the two k-beam entry points share, on stream s: the beam state allocated, `slots` slots at position 0 on BOS
// (`counters`: as reset_slots) with no fork counted yet, then the entry point's own `init` of its beams, then the loop
// bound (the brevity penalty of num_steps + 1, as reset_beam1_state)
static int start_beams(mt3_engine* e, int slots, bool counters, int num_steps, hipStream_t s, const std::function<int()>& init) {
  MT3_TRY(ensure_beam_state(e));
  MT3_TRY(reset_slots(e, slots, counters, false, s));
  MT3_HIP_CHECK(hipMemsetAsync(e->bk_forks, 0, 4, s));
  MT3_TRY(embed_bos(e, slots, s));
  MT3_TRY(init());
  return mt3k::launch_set_float(e->beam_cfg, brevity_penalty(num_steps + 1), s);
}

static int decode_beams_impl(mt3_engine* e, int32_t batch, int32_t k, int32_t num_steps, int32_t flags, int32_t* d_ids,
                             int32_t* d_all_ids, float* d_scores, int32_t* h_steps_run, hipStream_t s) {
  const char* who = "mt3_engine_decode_beams";
  MT3_TRY(engine_ready(e, who));
  MT3_TRY(beams_fit(e, who, k));
  if (flags & ~(MT3_DECODE_NO_GRAPH | MT3_DECODE_EARLY_EXIT | MT3_DECODE_SINGLE_STREAM))
    return invalid(who, "flags other than NO_GRAPH / EARLY_EXIT / SINGLE_STREAM");
  if (batch <= 0 || static_cast<int64_t>(batch) * k > e->cfg.max_batch)
    return invalid(who, "batch * num_beams must be 1 .. max_batch");
  if (batch * k != e->cur_batch)
    return invalid(who, "the preceding encode must hold each of the batch's segments num_beams times in a row "
                        "(batch * num_beams rows)");
  MT3_TRY(steps_fit(e, who, num_steps));
  if (!d_ids) return invalid(who, "null ids");
  int seg_var = 0;
  MT3_TRY(seg_tables_fit(e, who, batch, 2 * k, num_steps, &seg_var));
  const int slots = batch * k;
  MT3_TRY(start_beams(e, slots, true, num_steps, s, [&] {
    MT3_TRY(mt3k::launch_iota(e->slot_row, slots, s));
    return mt3k::launch_beam_init(e->bk_live, e->bk_fin_score, e->bk_fin_step, e->bk_fin_beam, slots, k, s);
  }));
  const int variant = kVarRetire | kVarBeams | (k << kVarBeamsShift) | seg_var;
  PendingDecode& p = begin_job(e);
  p.beams = k;
  p.num_steps = num_steps;
  p.batch = batch;
  p.d_ids = d_ids;
  p.d_all_ids = d_all_ids;
  p.d_scores = d_scores;
  p.s = s;
  const GroupJob j{batch, k, 1, variant, num_steps, (flags & MT3_DECODE_EARLY_EXIT) != 0, !(flags & MT3_DECODE_NO_GRAPH), false,
                   s, nullptr, nullptr};
  // (an engine configured for graph chains keeps every decode on the caller's stream, this one too -- in one chain)
  MT3_TRY(run_decode_job(e, j, flags, e->cfg.decode_chains > 1, h_steps_run));
  MT3_HIP_CHECK(wait_stream(e, kMaxGroups, s));    // complete on return: the fork count is in host memory
  return MT3_OK;
}

// ------------------------------------------------------------------------------------------- in-flight batching
// mt3_engine_transcribe, _transcribe_beams, _transcribe_draws (mt3_hip.h): the engine's max_batch decode slots stay full
// while there are segments left.  The queue between the encoder passes (producer: the calling thread, produce_chunks) and
// the row groups (consumers: run_group_stream) is csrc/feed.h; run_stream_job runs the two sides of one job, and
// stream_call is the body the three entry points share behind their argument checks.
static int ensure_stage(mt3_engine* e) {
  if (e->stage_cap) return MT3_OK;
  const mt3_engine_config& c = e->cfg;
  const int cap = c.max_batch < kStageChunkCap ? c.max_batch : kStageChunkCap;
  const size_t row = static_cast<size_t>(c.num_heads) * c.input_length * 64;
  e->stage_kv.assign(c.num_decoder_layers, nullptr);
  e->stage_scale.assign(c.num_decoder_layers, nullptr);
  for (int l = 0; l < c.num_decoder_layers; ++l) {
    MT3_TRY(dmalloc(e, &e->stage_kv[l], static_cast<size_t>(kStageChunks) * 2 * cap * row * e->kv_esize));
    if (e->kv_fp8)
      MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->stage_scale[l]),
                      static_cast<size_t>(kStageChunks) * cap * c.num_heads * c.input_length * sizeof(float2)));
  }
  e->stage_cap = cap;
  return MT3_OK;
}

// Chunk `chunk` of the staging ring, layer l: K/V rows [2][stage_cap][H][T][64] cache elements, and (e4m3 caches) the
// scale rows [stage_cap][H][T]
static char* stage_chunk_base(const mt3_engine* e, int l, int chunk) {
  const size_t row_bytes = static_cast<size_t>(e->cfg.num_heads) * e->cfg.input_length * 64 * e->kv_esize;
  return static_cast<char*>(e->stage_kv[l]) + static_cast<size_t>(chunk % kStageChunks) * 2 * e->stage_cap * row_bytes;
}
static float2* stage_chunk_scale(const mt3_engine* e, int l, int chunk) {
  if (!e->kv_fp8) return nullptr;
  return e->stage_scale[l] + static_cast<size_t>(chunk % kStageChunks) * e->stage_cap * e->cfg.num_heads * e->cfg.input_length;
}

// the staged run `rg` (sequence number -> ring chunk) and the caches of a `dst_batch`-row decode it is copied into
// (per > 1, mt3_engine_transcribe_draws: the run counts draws, `per` of which share one staged entry)
static void fill_staged_cross(const mt3_engine* e, const FeedRange& rg, int dst_batch, mt3k::StagedCross* x, int per) {
  const mt3_engine_config& c = e->cfg;
  x->n_layers = c.num_decoder_layers;
  x->row_bytes = static_cast<size_t>(c.num_heads) * c.input_length * 64 * e->kv_esize;
  x->sc_bytes = static_cast<size_t>(c.num_heads) * c.input_length * sizeof(float2);
  for (int l = 0; l < c.num_decoder_layers; ++l) {
    x->src[l] = stage_chunk_base(e, l, rg.seq);
    x->dst[l] = static_cast<char*>(e->dec[l].cross_kv);
    x->src_sc[l] = reinterpret_cast<const char*>(stage_chunk_scale(e, l, rg.seq));
    x->dst_sc[l] = e->kv_fp8 ? reinterpret_cast<char*>(e->dec[l].cross_scale) : nullptr;
  }
  x->src_batch = rg.batch;
  x->src_entry0 = rg.entry0;
  x->dst_batch = dst_batch;
  x->per = per;
}

// the refill launches of one run of staged segments for row group `r` (rg == nullptr: finished slots only hand their
// ids over -- the queue is empty)
static int refill_group(mt3_engine* e, const GroupRun& r, int cur, const FeedRange* rg, const StreamJob& sj) {
  const mt3_engine_config& c = e->cfg;
  const size_t r0 = static_cast<size_t>(r.row0);
  mt3k::RefillArgs a{};
  a.st = slot_state(e, r.row0, r.slot);
  a.in = input_row(e, r.row0);
  if (r.variant & kVarBeam) a.beam = beam1_state(e, r.row0, 0);
  a.ids = e->ids;
  a.ids_stride = c.max_decode_len;
  a.out_ids = sj.d_ids;
  a.plan = e->refill_plan + r0 + r.slot;
  a.rows = cur;
  a.gram0 = grammar_initial(e);
  if (rg) {
    a.n_new = rg->n;
    a.first_seg = rg->first_seg;
    fill_staged_cross(e, *rg, r.batch, &a.x, sj.per);
  }
  return mt3k::launch_refill(a, r.s);
}

// the beam counterpart of refill_group: finished ELEMENTS of row group `r` hand their k decodes over (the caller's
// buffers, rows by segment) and restart on the run `rg` of staged segments (rg == nullptr: hand-over only)
static int refill_beam_group(mt3_engine* e, const GroupRun& r, const FeedRange* rg, const StreamJob& sj) {
  const mt3_engine_config& c = e->cfg;
  mt3k::BeamRefillArgs a{};
  a.b = beam_args(e, r.row0, r.rows, sj.unit, r.slot);
  a.plan = e->refill_plan + r.row0 + r.slot;
  a.L = c.max_decode_len;
  a.num_steps = r.num_steps;
  a.out_ids = sj.d_ids;
  a.out_all = sj.d_all_ids;
  a.out_scores = sj.d_scores;
  a.gram0 = grammar_initial(e);
  if (rg) {
    a.n_new = rg->n;
    a.first_seg = rg->first_seg;
    fill_staged_cross(e, *rg, r.batch, &a.x, sj.per);
  }
  return mt3k::launch_beam_refill(a, r.s);
}

// One row group's loop of mt3_engine_transcribe: as run_group, but a finished slot restarts on the next staged segment
// at the poll, and the loop ends when the queue is empty for good and every slot of the group has finished.
// The beam job (mt3_engine_transcribe_beams): the unit of refill is an ELEMENT of sj.unit slots -- the snapshot, the
// watchdog and `refillable` count slots, the feed counts segments = elements -- and the group is never compacted.
// sj.from_ring (the beam job and mt3_engine_transcribe_draws, whose feed counts DRAWS, sj.per of which share one staged
// entry): the group starts with every slot finished and empty and takes its first entries off the feed before its first
// step.
static int run_group_stream(mt3_engine* e, GroupRun& r, Feed& f, const StreamJob& sj) {
  const bool beams = (r.variant & kVarBeams) != 0;
  const int unit = sj.unit, kPoll = sj.poll;
  auto refill = [&](int cur_rows, const FeedRange* rg) {
    return beams ? refill_beam_group(e, r, rg, sj) : refill_group(e, r, cur_rows, rg, sj);
  };
  int cur = r.rows;
  hipGraphExec_t exec = nullptr;
  int exec_rows = -1, flushed_at = -1;
  std::vector<FeedRange> held, got(kStageChunks + 2);
  r.ran = 0;
  r.used_graph = r.use_graph;
  // The poll is PIPELINED: at the end of interval j the group's counter of finished slots is copied to pinned memory and
  // an event recorded behind the copy -- and the host goes straight on to enqueue interval j + 1; it looks at snapshot j
  // only after that (sleeping until the event if need be), so the device always has an interval of steps queued and never
  // waits for the host's answer (round 5: with drained polls a sleeping host cost 1.3 % at 256 slots).  What the
  // snapshot triggers -- refills, the hand-over of finished ids, a compaction -- is enqueued BEHIND interval j + 1 and in
  // front of snapshot j + 1, so every snapshot already accounts for it.  The kernels act on the device's state when they
  // run (decode_ops.hip: the plan kernels scan the done flags), the snapshot only says how many staged segments to hand
  // out: it may be an interval stale, never wrong (finished slots stay finished until a refill restarts them).
  int parity = 0;
  bool pending = false;
  // Watchdog on PROGRESS, not on the step count (a group that is starved by a slow encoder keeps stepping its live
  // slots, so its counter grows with wall time): a live slot finishes within num_steps steps of its (re)start and a
  // snapshot is at most two poll intervals old, so `stall_limit` steps without a refill, a newly finished slot or a
  // compaction can only mean a slot that never terminates.
  const long stall_limit = static_cast<long>(r.num_steps) + 4L * kPoll + 64;
  long last_progress = 0;
  int seen_fin = 0;
  if (sj.from_ring) {
    // every element is finished and empty: the first refill comes before the first step interval
    int n_fin = r.rows;
    bool dry = false;
    while (!dry && n_fin == r.rows) {
      feed_wait(f);                              // (sleeps until the first encoder pass is on offer)
      if (mt3feed::feed_failed(f)) return MT3_OK;
      const int nr = feed_pop(f, n_fin / unit, got.data(), static_cast<int>(got.size()), &dry);
      for (int i = 0; i < nr; ++i) {
        MT3_TRY(refill(cur, &got[i]));
        held.push_back(got[i]);
        n_fin -= got[i].n * unit;
      }
    }
    if (n_fin == r.rows) return MT3_OK;          // the other groups took every segment: nothing to decode here
    seen_fin = n_fin;
  }
  for (long t = 0;; ++t) {
    if (t - last_progress > stall_limit)
      return mt3::fail(MT3_ERR_INVALID, "mt3_engine_transcribe: a row group made no progress for num_steps + 4 polls");
    if (r.use_graph && exec_rows != cur) {
      exec = group_graph(e, r, cur);
      exec_rows = cur;
      if (!exec) {
        r.use_graph = r.used_graph = false;
        ++e->graph_fallbacks;
      }
    }
    if (r.use_graph) MT3_HIP_CHECK(hipGraphLaunch(exec, r.s));
    else MT3_TRY(enqueue_step(e, r.row0, cur, r.batch, r.variant, r.chains, r.s, r.slot));
    ++r.ran;
    if (t % kPoll != kPoll - 1) continue;
    // ---- the previous interval's snapshot
    if (pending) {
      hipEvent_t pev = wait_event(e, r.slot, 2 + (parity ^ 1));
      MT3_HIP_CHECK(e->spin_waits ? hipEventSynchronize(pev) : sleep_until(pev));
      feed_release(f, held);                     // what was taken one snapshot ago was copied out in front of this one
      held.clear();
      int n_fin = e->h_pinned[r.slot + kMaxGroups * (parity ^ 1)];   // finished slots among the group's r.rows (dropped ones included)
      if (n_fin != seen_fin) last_progress = t;
      bool dry = false;
      for (;;) {
        if (mt3feed::feed_failed(f)) return MT3_OK;           // somebody else reports the error
        const int refillable = (n_fin - (r.rows - cur)) / unit;
        const int nr = feed_pop(f, refillable, got.data(), static_cast<int>(got.size()), &dry);
        for (int i = 0; i < nr; ++i) {
          MT3_TRY(refill(cur, &got[i]));
          held.push_back(got[i]);
          n_fin -= got[i].n * unit;
          last_progress = t;
        }
        if (dry || n_fin < r.rows) break;
        feed_wait(f);                            // nothing live and the encoder is behind: sleep, do not spin through empty steps
      }
      if (dry) {
        // the queue is empty for good: finished slots hand over their ids, the live ones are compacted as under EARLY_EXIT
        const int live = r.rows - n_fin;
        int want = (live + 31) & ~31;
        if (want > r.rows) want = r.rows;
        const bool compact = !beams && live > 0 && want < cur;    // beam groups stay where they are (run_group)
        // (the hand-over runs on the device's own done flags, directly in front of a compaction or of the exit: no slot
        // that finished after the snapshot can be dropped with its ids still in the engine)
        if ((n_fin - (r.rows - cur) > 0 && n_fin != flushed_at) || compact || live <= 0) {
          MT3_TRY(refill(cur, nullptr));
          flushed_at = n_fin;
        }
        if (live <= 0) break;
        if (compact) {
          MT3_TRY(compact_group(e, r, cur));
          cur = want;
          ++e->compactions_now;
          last_progress = t;
        }
      }
      seen_fin = n_fin;
    }
    // ---- this interval's snapshot
    hipEvent_t ev = wait_event(e, r.slot, 2 + parity);
    if (!ev) return mt3::fail(MT3_ERR_HIP, "mt3_engine_transcribe: could not create a poll event");
    MT3_HIP_CHECK(hipMemcpyAsync(e->h_pinned + r.slot + kMaxGroups * parity, e->n_done + r.slot, 4, hipMemcpyDeviceToHost, r.s));
    MT3_HIP_CHECK(hipEventRecord(ev, r.s));
    pending = true;
    parity ^= 1;
  }
  MT3_HIP_CHECK(wait_stream(e, r.slot, r.s));
  feed_release(f, held);
  return MT3_OK;
}

// the producer side of the feed (calling thread, caller's stream).  sj.per > 1 (mt3_engine_transcribe_draws): the feed counts
// draws, `per` of every segment: a claim is one of up to stage_cap * per draws, so that `first`, `n` and `pad` are multiples
// of `per` and the pass encodes the (pad + n) / per segments from (first - pad) / per on, each ONCE.
static int produce_chunks(mt3_engine* e, Feed& f, const float* d_inputs, hipStream_t s, const StreamJob& sj) {
  const mt3_engine_config& c = e->cfg;
  const int per = sj.per;
  const size_t seg_floats = static_cast<size_t>(c.input_length) * c.input_depth;
  const int min_batch = e->stage_cap < kStageMinBatch ? e->stage_cap : kStageMinBatch;
  std::vector<void*> kv(c.num_decoder_layers);
  std::vector<float2*> sc(c.num_decoder_layers, nullptr);
  int rc = MT3_OK;
  for (int q = 0; rc == MT3_OK; ++q) {
    int first, n, pad;
    // (in draws, never above the job: stage_cap * per itself may not fit an int)
    const long long total = f.n_total;
    const int cap = static_cast<int>(std::min(static_cast<long long>(e->stage_cap) * per, total));
    const int least = static_cast<int>(std::min(static_cast<long long>(min_batch) * per, total));
    if (!mt3feed::feed_claim(f, q, cap, least, &first, &n, &pad)) break;
    for (int l = 0; l < c.num_decoder_layers; ++l) {
      kv[l] = stage_chunk_base(e, l, q);
      sc[l] = stage_chunk_scale(e, l, q);
    }
    CrossDst dst;
    dst.kv = kv.data();
    dst.scale = e->kv_fp8 ? sc.data() : nullptr;
    // (skip_encoder: mt3_debug_engine_transcribe's differential timing -- the chunk goes on offer with whatever the staging
    // ring holds; under an imposed EOS schedule the decode does exactly the same work)
    if (!sj.skip_encoder)
      rc = encode_impl(e, d_inputs + static_cast<size_t>((first - pad) / per) * seg_floats, (pad + n) / per, nullptr, dst, s);
    if (rc == MT3_OK && wait_stream(e, kMaxGroups, s) != hipSuccess) rc = mt3::fail(MT3_ERR_HIP, "mt3_engine_transcribe: encoder pass failed");
    if (rc != MT3_OK) break;
    mt3feed::feed_publish(f, q, first, n, pad);
  }
  mt3feed::feed_finish(f, rc != MT3_OK);
  return rc;
}

// what a streaming job did, in slots: the feed's counters and the longest group's steps; `initial` of the feed's refills
// were the first fill of the slots (a job that starts from the ring), which the caller did not ask about
static mt3_transcribe_stats stream_stats(const mt3_engine* e, const GroupJob& j, const Feed& f, int most, int initial) {
  mt3_transcribe_stats st{};
  st.slots = j.units * j.unit;
  st.groups = j.groups;
  st.steps_run = most;
  st.polls = f.polls;
  st.refills = (f.refills - initial) * j.unit;
  st.starved_polls = f.starved;
  st.encoder_chunks = f.produced;
  st.compactions = e->compactions;              // (beam groups are never compacted: 0)
  st.used_graph = e->last_used_graph;
  return st;
}

// The streaming job sj / j over n feed entries, from its posting to its end: the row groups run run_group_stream on their
// workers while the calling thread encodes what is not in the caches yet into the staging ring (everything if
// sj.from_ring, else the entries from j.units on); then the groups are joined and *st says what ran.  The device-side
// start of the slots is enqueued on j.s before this and closed with part_begin.
static int run_stream_job(mt3_engine* e, const StreamJob& sj, const GroupJob& j, const float* d_inputs, int n,
                          mt3_transcribe_stats* st) {
  Feed feed;
  feed.n_total = n;
  feed.next_seg = sj.from_ring ? 0 : j.units;
  feed.finished = feed.next_seg == n;
  begin_job(e);
  int rc = MT3_OK;
  if (!post_groups(e, j, [e, &feed, &sj](GroupRun& r) { return run_group_stream(e, r, feed, sj); }, &feed)) {
    feed_fail(feed);
    rc = mt3::fail(MT3_ERR_HIP, std::string(sj.who) + ": could not start a row group's worker thread");
  } else if (!feed.finished) {
    rc = produce_chunks(e, feed, d_inputs, j.s, sj);
  }
  const std::string producer_err = rc != MT3_OK ? mt3_last_error() : "";
  int most = 0;
  const int joined = join_groups(e, sj.who, &most);
  *st = stream_stats(e, j, feed, most, sj.from_ring ? j.units : 0);
  return rc != MT3_OK ? mt3::fail(rc, producer_err) : joined;      // the producer's message wins over a group's
}

// ---- the two starts of a streaming job's slots, on the caller's stream
// mt3_engine_transcribe's direct first pass: the first j.units of the n segments go straight into the caches, slot i
// starts on segment i
static int start_direct(mt3_engine* e, const StreamJob& sj, const GroupJob& j, const float* d_inputs, int n) {
  const int S = j.units;
  hipStream_t s = j.s;
  MT3_TRY(encode_impl(e, d_inputs, S, nullptr, CrossDst{}, s));
  MT3_HIP_CHECK(hipMemsetAsync(sj.d_ids, 0, static_cast<size_t>(n) * e->cfg.max_decode_len * 4, s));
  MT3_TRY(reset_slots(e, S, true, true, s));
  MT3_TRY(embed_bos(e, S, s));
  MT3_TRY(mt3k::launch_iota(e->slot_row, S, s));
  MT3_TRY(mt3k::launch_iota(e->slot_seg, S, s));
  if (j.variant & kVarBeam) MT3_TRY(reset_beam1_state(e, j.num_steps, s));
  return MT3_OK;
}

// a job that starts from the ring: every slot finished and empty, with a valid (BOS) input row so that the dense launches
// of empty slots read numbers, and every group's counter of finished slots = its slots.  The beam job's form is one
// launch behind the beam start; the greedy form (mt3_engine_transcribe_draws; slot i on cache row i) is memsets.
static int start_empty(mt3_engine* e, const StreamJob& sj, const GroupJob& j, int n) {
  const int slots = j.units * j.unit;
  hipStream_t s = j.s;
  mt3k::GroupSlots gs{};
  for (int g = 0; g < j.groups; ++g) {
    int u0, un;
    chain_rows(j.units, j.groups, g, &u0, &un);
    gs.n[g] = un * j.unit;
  }
  if (j.variant & kVarBeams)
    return start_beams(e, slots, false, j.num_steps, s, [&] {
      return mt3k::launch_beam_stream_init(e->done, e->slot_seg, e->bk_fork_src, e->slot_row, e->n_done, slots, j.groups, gs, s);
    });
  MT3_HIP_CHECK(hipMemsetAsync(sj.d_ids, 0, static_cast<size_t>(n) * e->cfg.max_decode_len * 4, s));
  MT3_TRY(reset_slots(e, slots, false, true, s));
  MT3_TRY(embed_bos(e, slots, s));
  MT3_TRY(mt3k::launch_iota(e->slot_row, slots, s));
  MT3_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->done), 1, static_cast<size_t>(slots), s));
  MT3_HIP_CHECK(hipMemsetAsync(e->slot_seg, 0xFF, static_cast<size_t>(slots) * 4, s));   // -1: no segment
  for (int g = 0; g < j.groups; ++g)
    MT3_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->n_done + g), gs.n[g], 1, s));
  return MT3_OK;
}

// The body the three streaming entry points share behind their argument checks: job sj over n feed entries (segments;
// draws) in units = min(n, max_batch / sj.unit) units of slots.  `variant`: the entry point's bits of the step variant;
// groups_override: stream_groups_for.  h_stats (may be nullptr) is written as mt3_hip.h says: by the beam job only when
// it succeeds, by the other two also for a job that failed once it was running.
static int stream_call(mt3_engine* e, const StreamJob& sj, const float* d_inputs, int n, int num_steps, int flags, int variant,
                       int groups_override, mt3_transcribe_stats* h_stats, hipStream_t s) {
  const mt3_engine_config& c = e->cfg;
  const bool beams = (variant & kVarBeams) != 0;
  const int units = n < c.max_batch / sj.unit ? n : c.max_batch / sj.unit;
  if (sj.from_ring || n > units) MT3_TRY(ensure_stage(e));
  const int groups = stream_groups_for(c, flags, units, sj.unit, groups_override);
  if (ensure_group_streams(e, groups) != MT3_OK)
    return mt3::fail(MT3_ERR_HIP, std::string(sj.who) + ": could not create the row groups' streams");
  const GroupJob j{units, sj.unit, groups, variant | kVarRetire | kVarStream, num_steps, true, !(flags & MT3_DECODE_NO_GRAPH),
                   true, s, nullptr, nullptr};
  MT3_TRY(sj.from_ring ? start_empty(e, sj, j, n) : start_direct(e, sj, j, d_inputs, n));
  e->cur_batch = units * sj.unit;
  e->stream_max_len = num_steps;
  MT3_HIP_CHECK(hipEventRecord(e->part_begin, s));
  mt3_transcribe_stats st{};
  const int rc = run_stream_job(e, sj, j, d_inputs, n, &st);
  if (beams) {
    MT3_TRY(rc);
    // every group thread has waited for its stream: the fork count of the job is final
    MT3_HIP_CHECK(hipMemcpyAsync(e->h_pinned + kForksPinned, e->bk_forks, 4, hipMemcpyDeviceToHost, s));
    MT3_HIP_CHECK(wait_stream(e, kMaxGroups, s));
  }
  if (h_stats) *h_stats = st;
  return rc;
}

// flags within `allowed`, buffers, a job, steps in range: the arguments every streaming entry point takes
static int stream_args_fit(const mt3_engine* e, const char* who, int flags, int allowed, const float* d_inputs,
                           const int32_t* d_ids, int n_segments, int num_steps) {
  if (flags & ~allowed)
    return invalid(who, allowed & MT3_DECODE_BEAM1 ? "flags are MT3_DECODE_NO_GRAPH | MT3_DECODE_BEAM1 | MT3_DECODE_SINGLE_STREAM"
                                                   : "flags are MT3_DECODE_NO_GRAPH | MT3_DECODE_SINGLE_STREAM");
  if (!d_inputs || !d_ids || n_segments <= 0) return invalid(who, "null buffer or no segments");
  return steps_fit(e, who, num_steps);
}
constexpr int kStreamFlags = MT3_DECODE_NO_GRAPH | MT3_DECODE_SINGLE_STREAM;

// poll_steps / groups_override: 0 = the product's choice (mt3_debug_engine_transcribe sets them for A/B runs)
static int transcribe_impl(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t num_steps, int32_t flags,
                           int32_t* d_ids, mt3_transcribe_stats* h_stats, void* stream, int poll_steps, int groups_override,
                           bool skip_encoder) {
  const char* who = "mt3_engine_transcribe";
  MT3_TRY(engine_ready(e, who));
  MT3_TRY(stream_args_fit(e, who, flags, kStreamFlags | MT3_DECODE_BEAM1, d_inputs, d_ids, n_segments, num_steps));
  MT3_TRY(stream_fits(e, who, n_segments));
  const bool beam1 = (flags & MT3_DECODE_BEAM1) != 0;
  int seg_var = 0;
  MT3_TRY(seg_tables_fit(e, who, n_segments, 2, num_steps, &seg_var));
  MT3_TRY(sampling_fits(e, who, n_segments, beam1, &seg_var));
  const StreamJob sj{who, 1, 1, false, d_ids, nullptr, nullptr, poll_steps > 0 ? poll_steps : kStreamPollSteps, skip_encoder};
  return stream_call(e, sj, d_inputs, n_segments, num_steps, flags, (beam1 ? kVarBeam : 0) | (e->eos_on ? kVarEos : 0) | seg_var,
                     groups_override, h_stats, static_cast<hipStream_t>(stream));
}

int mt3_engine_transcribe(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t num_steps, int32_t flags,
                          int32_t* d_ids, mt3_transcribe_stats* h_stats, void* stream) {
  return transcribe_impl(e, d_inputs, n_segments, num_steps, flags, d_ids, h_stats, stream, 0, 0, false);
}

int mt3_debug_engine_transcribe(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t num_steps, int32_t flags,
                                int32_t poll_steps, int32_t row_groups, int32_t skip_encoder_passes, int32_t* d_ids,
                                mt3_transcribe_stats* h_stats, void* stream) {
  if (poll_steps < 0 || poll_steps > 1024 || row_groups < 0 || row_groups > kMaxGroups)
    return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_transcribe: poll_steps in [0, 1024], row_groups in [0, 4]");
  return transcribe_impl(e, d_inputs, n_segments, num_steps, flags, d_ids, h_stats, stream, poll_steps, row_groups,
                         skip_encoder_passes != 0);
}

// mt3_engine_transcribe_beams: in-flight batching of the k-beam search, a GroupJob of E = min(n_segments, max_batch / k)
// units of k slots each; EVERY segment, the first E included, reaches its element through the staging ring (one code path, and no
// k-fold copy of the inputs for a direct first encode): the groups start with every element finished and empty, and the
// feed starts at segment 0.
int mt3_engine_transcribe_beams(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t num_beams,
                                int32_t num_steps, int32_t flags, int32_t* d_ids, int32_t* d_all_ids, float* d_scores,
                                mt3_transcribe_stats* h_stats, void* stream) {
  const char* who = "mt3_engine_transcribe_beams";
  const int k = num_beams;
  if (!e) return invalid(who, "null engine");
  MT3_TRY(stream_args_fit(e, who, flags, kStreamFlags, d_inputs, d_ids, n_segments, num_steps));
  MT3_TRY(beams_fit(e, who, k));
  MT3_TRY(engine_ready(e, who));
  if (e->eos_on) return invalid(who, "the synthetic EOS schedule drives the greedy / beam-1 token kernel only");
  int seg_var = 0;
  MT3_TRY(seg_tables_fit(e, who, n_segments, 2 * k, num_steps, &seg_var));
  const StreamJob sj{who, k, 1, true, d_ids, d_all_ids, d_scores, kStreamPollSteps, false};
  return stream_call(e, sj, d_inputs, n_segments, num_steps, flags, kVarBeams | (k << kVarBeamsShift) | seg_var, 0, h_stats,
                     static_cast<hipStream_t>(stream));
}

// mt3_engine_transcribe_draws: mt3_engine_transcribe's greedy path on a job of D = n_segments * per draws in
// S = min(D, max_batch) slots, every segment encoded ONCE.  As in the beam job EVERY draw, the first S included, reaches its
// slot through the staging ring: the groups start with every slot finished and empty and the feed -- which counts draws --
// starts at 0; `per` consecutive draws copy the same staged entry (StagedCross::per).
int mt3_engine_transcribe_draws(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t per, int32_t num_steps,
                                int32_t flags, int32_t* d_ids, mt3_transcribe_stats* h_stats, void* stream) {
  const char* who = "mt3_engine_transcribe_draws";
  if (!e) return invalid(who, "null engine");
  MT3_TRY(stream_args_fit(e, who, flags, kStreamFlags, d_inputs, d_ids, n_segments, num_steps));   // (beam-1 does not sample)
  if (per < 1) return invalid(who, "per must be at least 1");
  if (static_cast<long long>(n_segments) * per > INT32_MAX / e->cfg.max_decode_len)
    return invalid(who, "n_segments * per exceeds INT32_MAX / max_decode_len");
  const int D = n_segments * per;
  MT3_TRY(stream_fits(e, who, D));
  MT3_TRY(engine_ready(e, who));
  int seg_var = 0;
  MT3_TRY(seg_tables_fit(e, who, D, 2, num_steps, &seg_var));
  MT3_TRY(sampling_fits(e, who, D, false, &seg_var));
  const StreamJob sj{who, 1, per, true, d_ids, nullptr, nullptr, kStreamPollSteps, false};
  return stream_call(e, sj, d_inputs, D, num_steps, flags, (e->eos_on ? kVarEos : 0) | seg_var, 0, h_stats,
                     static_cast<hipStream_t>(stream));
}

int mt3_engine_decode(mt3_engine* e, int32_t batch, int32_t num_steps, int32_t flags, int32_t* d_ids,
                      float* d_first_logits, int32_t* h_steps_run, void* stream) {
  return decode_impl(e, batch, num_steps, flags, 0, nullptr, nullptr, d_ids, d_first_logits, h_steps_run, stream);
}

int mt3_engine_decode_beams(mt3_engine* e, int32_t batch, int32_t num_beams, int32_t num_steps, int32_t flags,
                            int32_t* d_ids, int32_t* d_all_ids, float* d_scores, int32_t* h_steps_run, void* stream) {
  return decode_beams_impl(e, batch, num_beams, num_steps, flags, d_ids, d_all_ids, d_scores, h_steps_run,
                           static_cast<hipStream_t>(stream));
}

int mt3_engine_decode_wait(mt3_engine* e, int32_t* h_steps_run) {
  if (!e || !e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_decode_wait: engine not finalized");
  return decode_finish(e, h_steps_run);
}

int mt3_engine_decode_forced(mt3_engine* e, int32_t batch, int32_t num_steps, int32_t flags,
                             const int32_t* d_forced_ids, float* d_step_logits, int32_t* d_ids, void* stream) {
  if (!d_forced_ids) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_decode_forced: null forced ids");
  return decode_impl(e, batch, num_steps, flags, 0, d_forced_ids, d_step_logits, d_ids, nullptr, nullptr, stream);
}

// ---------------------------------------------------------------------------------------------- teacher-forced scoring
// Rows of the score workspace by default: 32 segments at L = 1024 (about 0.7 GB in f32); a chunk is that many segments.
constexpr int kScoreRows = 32768;

static int score_default_chunk(const mt3_engine* e) {
  const int Lp = (e->cfg.max_decode_len + 63) / 64 * 64;
  return std::max(1, std::min(e->cfg.max_batch, kScoreRows / Lp));
}

static int ensure_score_workspace(mt3_engine* e, int segs) {
  if (e->score_cap >= segs) return MT3_OK;
  const mt3_engine_config& c = e->cfg;
  const int Lp = (c.max_decode_len + 63) / 64 * 64;
  const size_t R = static_cast<size_t>(segs) * Lp, es = e->esize, hd = e->HD(), emb = c.emb_dim;
  // (a grown workspace replaces the old one; the old buffers stay in the engine's allocation list until destroy)
  MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->sc_y), R * emb * 4));
  if (score_split(e)) {
    MT3_TRY(dmalloc(e, &e->sc_y_ct, R * emb * 2));
    MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->sc_y_ss), R * (emb / 16) * 4));
  }
  MT3_TRY(dmalloc(e, &e->sc_qkv, R * 3 * hd * es));
  MT3_TRY(dmalloc(e, &e->sc_attn, R * hd * es));
  MT3_TRY(dmalloc(e, &e->sc_q, R * hd * es));
  MT3_TRY(dmalloc(e, &e->sc_h, R * c.mlp_dim * es));
  MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->sc_logits), R * c.vocab_size * 4));
  MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->sc_tgt), R * 4));
  MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->sc_tok), R * 4));
  e->score_cap = segs;
  e->score_Lp = Lp;
  return MT3_OK;
}

// f32 engine on the three-plane tile: plane copies of the decoder matrices it scores with (built once, on the device,
// from the f32 matrices finalize uploaded -- the same split upload_dense makes on the host)
static int ensure_score_planes(mt3_engine* e, hipStream_t s) {
  if (!e->x6 || e->score_planes) return MT3_OK;
  std::vector<Dense*> all;
  for (LayerDev& L : e->dec) all.insert(all.end(), {&L.wqkv, &L.wo, &L.wq_x, &L.wo_x, &L.wi, &L.wo_mlp});
  all.push_back(&e->logits_w);
  for (Dense* D : all) {
    const size_t n = static_cast<size_t>(D->N) * D->K;
    for (int k = 0; k < 3; ++k) MT3_TRY(dmalloc(e, &D->p[k], n * 2));
    MT3_TRY(mt3k::launch_planes(static_cast<const float*>(D->w), D->p[0], D->p[1], D->p[2], n, s));
  }
  MT3_HIP_CHECK(hipStreamSynchronize(s));     // later calls may come on other streams
  e->score_planes = true;
  return MT3_OK;
}

// The prefill and the reduction of `batch` rows whose cross-K/V sit in cache rows row0 .. of the last encoder pass, `per`
// consecutive rows on each cache row (row i reads cache row row0 + i / per; per = 1: one row each); the caller arrays
// start at the first of them.  d_top1_ids / d_top1_scores (either): the reduction is launch_score_stats instead of
// launch_score_reduce (same token and sequence scores)
static int score_impl(mt3_engine* e, int32_t batch, int32_t length, int32_t row0, int32_t per, const int32_t* d_targets,
                      const int32_t* d_decoder_inputs, const float* d_weights, float* d_sequence_scores,
                      float* d_token_scores, int32_t* d_top1_ids, float* d_top1_scores, float* d_logits, hipStream_t s) {
  const mt3_engine_config& c = e->cfg;
  const int dt = c.compute_dtype, emb = c.emb_dim, hd = e->HD(), H = c.num_heads, T = c.input_length, V = c.vocab_size;
  const int Lp = (length + 63) / 64 * 64;
  const int chunk = e->score_chunk_req > 0 ? e->score_chunk_req : score_default_chunk(e);
  MT3_TRY(ensure_score_workspace(e, chunk));
  MT3_TRY(ensure_score_planes(e, s));
  const size_t es = e->esize;
  int chunks = 0;
  for (int seg0 = 0; seg0 < batch; seg0 += chunk, ++chunks) {
    const int C = std::min(chunk, batch - seg0), M = C * Lp;
    {
      mt3k::ScoreEmbedArgs a{e->embedding, e->pos_table, d_targets, d_decoder_inputs, e->sc_tgt, e->sc_y,
                             M, Lp, length, seg0, emb, V};
      MT3_TRY(mt3k::launch_score_embed(a, s));
    }
    // three planes (f32 engine), the bf16 LDS-DMA tile from the split rows, or the encoder-sized tile with in-kernel
    // statistics
    const Resid R = score_rows(e, M);
    if (R.split) MT3_TRY(mt3k::launch_residual_split(e->sc_y, e->sc_y_ct, e->sc_y_ss, M, emb, s));
    for (int l = 0; l < c.num_decoder_layers; ++l) {
      LayerDev& L = e->dec[l];
      MT3_TRY(normed_gemm(e, R, L.wqkv, e->sc_qkv, 3 * hd, MT3_EPI_STORE, false, s));
      {
        mt3k::ScoreAttnArgs a{};
        a.q = e->sc_qkv;
        a.q_stride = 3 * hd;
        a.k = static_cast<const char*>(e->sc_qkv) + static_cast<size_t>(hd) * es;
        a.v = static_cast<const char*>(e->sc_qkv) + static_cast<size_t>(2 * hd) * es;
        a.kv_stride = 3 * hd;
        a.kv_bstride = static_cast<long long>(Lp) * 3 * hd;
        a.kv_hstride = 64;
        a.key_tgt = e->sc_tgt;
        a.out = e->sc_attn;
        a.out_stride = hd;
        a.B = C;
        a.H = H;
        a.Lq = Lp;
        a.n_keys = Lp;
        a.causal = 1;
        MT3_TRY(mt3k::launch_score_attention(dt, a, s));
      }
      MT3_TRY(resid_gemm(e, L.wo, e->sc_attn, R, false, s));
      MT3_TRY(normed_gemm(e, R, L.wq_x, e->sc_q, hd, MT3_EPI_STORE, false, s));
      {
        // the cross K/V cache of the encoded batch: [2][cur_batch][H][T][64]; the chunk's rows start at cache row
        // row0 + seg0 / per, seg0 % per rows into its group of `per`
        const size_t head = static_cast<size_t>(T) * 64;
        const int kv0 = row0 + seg0 / per;
        mt3k::ScoreAttnArgs a{};
        a.q = e->sc_q;
        a.q_stride = hd;
        a.k = static_cast<const char*>(L.cross_kv) + static_cast<size_t>(kv0) * H * head * es;
        a.v = static_cast<const char*>(L.cross_kv) + (static_cast<size_t>(e->cur_batch) + kv0) * H * head * es;
        a.kv_share = per;
        a.kv_b0 = seg0 % per;
        a.kv_stride = 64;
        a.kv_bstride = static_cast<long long>(H) * head;
        a.kv_hstride = static_cast<long long>(head);
        a.out = e->sc_attn;
        a.out_stride = hd;
        a.B = C;
        a.H = H;
        a.Lq = Lp;
        a.n_keys = T;
        a.causal = 0;
        MT3_TRY(mt3k::launch_score_attention(dt, a, s));
      }
      MT3_TRY(resid_gemm(e, L.wo_x, e->sc_attn, R, false, s));
      MT3_TRY(normed_gemm(e, R, L.wi, e->sc_h, c.mlp_dim, MT3_EPI_GEGLU, false, s));
      MT3_TRY(resid_gemm(e, L.wo_mlp, e->sc_h, R, false, s));
    }
    MT3_TRY(normed_gemm(e, R, e->logits_w, e->sc_logits, V, MT3_EPI_F32, false, s));     // decoder_norm folded
    {
      mt3k::ScoreReduceArgs a{e->sc_logits, e->sc_tgt, d_weights, e->sc_tok, d_token_scores, d_sequence_scores,
                              M, Lp, length, seg0, V};
      if (d_top1_ids || d_top1_scores) MT3_TRY(mt3k::launch_score_stats(mt3k::ScoreStatsArgs{a, d_top1_ids, d_top1_scores}, s));
      else MT3_TRY(mt3k::launch_score_reduce(a, s));
    }
    if (d_logits) {
      const size_t row = static_cast<size_t>(length) * V * 4;
      MT3_HIP_CHECK(hipMemcpy2DAsync(d_logits + static_cast<size_t>(seg0) * length * V, row, e->sc_logits,
                                     static_cast<size_t>(Lp) * V * 4, row, C, hipMemcpyDeviceToDevice, s));
    }
  }
  e->score_chunks = chunks;
  return MT3_OK;
}

int mt3_engine_score(mt3_engine* e, int32_t batch, int32_t length, const int32_t* d_targets,
                     const int32_t* d_decoder_inputs, const float* d_weights, float* d_sequence_scores,
                     float* d_token_scores, float* d_logits, void* stream) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_score: null engine");
  if (length < 1 || length > e->cfg.max_decode_len)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_score: length must be in 1 .. max_decode_len");
  if (!d_targets || !d_sequence_scores)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_score: null targets or sequence scores");
  if (e->kv_fp8)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_score: engines with e4m3 K/V caches (kv_cache_dtype MT3_FP8_E4M3) cannot score");
  if (!e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_score: engine not finalized");
  if (e->pending.active)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_score: a decode is in flight (MT3_DECODE_ASYNC): call mt3_engine_decode_wait first");
  if (batch <= 0 || batch > e->cur_batch)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_score: batch must be in 1 .. the batch of the preceding encode");
  return score_impl(e, batch, length, 0, 1, d_targets, d_decoder_inputs, d_weights, d_sequence_scores, d_token_scores, nullptr,
                    nullptr, d_logits, static_cast<hipStream_t>(stream));
}

// mt3_engine_score_segments (per = 1) and mt3_engine_score_candidates: `per` target rows on every segment's one encoder
// pass; fn: "<function>: "
static int score_job(mt3_engine* e, const std::string& fn, const float* d_inputs, int32_t n_segments, int32_t per,
                     int32_t length, const int32_t* d_targets, float* d_sequence_scores, float* d_token_scores,
                     int32_t* d_top1_ids, float* d_top1_scores, void* stream) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, fn + "null engine");
  if (!d_inputs || !d_targets || !d_sequence_scores)
    return mt3::fail(MT3_ERR_INVALID, fn + "null inputs, targets or sequence scores");
  if (n_segments < 1) return mt3::fail(MT3_ERR_INVALID, fn + "n_segments must be >= 1");
  if (per < 1) return mt3::fail(MT3_ERR_INVALID, fn + "per must be >= 1");
  if (static_cast<int64_t>(n_segments) * per > INT32_MAX)
    return mt3::fail(MT3_ERR_INVALID, fn + "n_segments * per must fit int32");
  if (length < 1 || length > e->cfg.max_decode_len)
    return mt3::fail(MT3_ERR_INVALID, fn + "length must be in 1 .. max_decode_len");
  if (e->kv_fp8)
    return mt3::fail(MT3_ERR_INVALID, fn + "engines with e4m3 K/V caches (kv_cache_dtype MT3_FP8_E4M3) cannot score");
  if (!e->finalized) return mt3::fail(MT3_ERR_INVALID, fn + "engine not finalized");
  if (e->pending.active)
    return mt3::fail(MT3_ERR_INVALID, fn + "a decode is in flight (MT3_DECODE_ASYNC): call mt3_engine_decode_wait first");
  const mt3_engine_config& c = e->cfg;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t seg_floats = static_cast<size_t>(c.input_length) * c.input_depth;
  // the chunks and their padding are those of the staging passes of mt3_engine_transcribe (feed.h): in bf16 a short last
  // chunk is encoded behind the `pad` segments in front of it, so that its pass takes the tiles of a full one
  const int min_batch = c.compute_dtype == MT3_BF16 ? std::min(c.max_batch, kStageMinBatch) : 0;
  Feed feed;
  feed.n_total = n_segments;
  int chunks = 0, passes = 0;
  for (int q = 0;; ++q, ++passes) {
    int first, n, pad;
    if (!mt3feed::feed_claim(feed, q, c.max_batch, min_batch, &first, &n, &pad)) break;
    MT3_TRY(encode_impl(e, d_inputs + static_cast<size_t>(first - pad) * seg_floats, pad + n, nullptr, CrossDst{}, s));
    e->cur_batch = pad + n;
    const size_t row = static_cast<size_t>(first) * per, at = row * length;
    MT3_TRY(score_impl(e, n * per, length, pad, per, d_targets + at, nullptr, nullptr, d_sequence_scores + row,
                       d_token_scores ? d_token_scores + at : nullptr, d_top1_ids ? d_top1_ids + at : nullptr,
                       d_top1_scores ? d_top1_scores + at : nullptr, nullptr, s));
    chunks += e->score_chunks;
  }
  e->score_chunks = chunks;
  e->score_passes = passes;
  return MT3_OK;
}

int mt3_engine_score_segments(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t length,
                              const int32_t* d_targets, float* d_sequence_scores, float* d_token_scores,
                              int32_t* d_top1_ids, float* d_top1_scores, void* stream) {
  return score_job(e, "mt3_engine_score_segments: ", d_inputs, n_segments, 1, length, d_targets, d_sequence_scores,
                   d_token_scores, d_top1_ids, d_top1_scores, stream);
}

int mt3_engine_score_candidates(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t per, int32_t length,
                                const int32_t* d_targets, float* d_sequence_scores, float* d_token_scores,
                                int32_t* d_top1_ids, float* d_top1_scores, void* stream) {
  return score_job(e, "mt3_engine_score_candidates: ", d_inputs, n_segments, per, length, d_targets, d_sequence_scores,
                   d_token_scores, d_top1_ids, d_top1_scores, stream);
}

// ---- mt3_hip_debug.h
int mt3_debug_engine_decode(mt3_engine* e, int32_t batch, int32_t num_steps, int32_t flags, int32_t skip,
                            int32_t* d_ids, void* stream) {
  if (skip & ~(MT3_DEBUG_SKIP_SELF_ATTN | MT3_DEBUG_SKIP_CROSS_ATTN))
    return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_decode: unknown skip bit");
  if (flags & MT3_DECODE_ASYNC) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_decode: not with MT3_DECODE_ASYNC");
  return decode_impl(e, batch, num_steps, flags, skip, nullptr, nullptr, d_ids, nullptr, nullptr, stream);
}

extern "C++" {
// a device array of at least n elements in *p: a larger one takes the place of one too small, which stays in the engine's
// allocation list until destroy; *replaced is set when a graph may hold the old one's address (there was one)
template <typename T, typename C>
static int grow(mt3_engine* e, T** p, C* cap, size_t n, bool* replaced) {
  if (n <= static_cast<size_t>(*cap)) return MT3_OK;
  T* grown = nullptr;
  MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&grown), n * sizeof(T)));
  *replaced = *replaced || *p != nullptr;
  *p = grown;
  *cap = static_cast<C>(n);
  return MT3_OK;
}

// shared body of mt3_engine_set_token_masks / mt3_engine_set_prompts (fn: "<function>: ", noun: "mask" / "prompt"): n rows
// of `stride` elements and, with h_seg, an index of n_segments entries; h_rows == nullptr or n == 0 clears.  bad_stride:
// what is wrong with the stride (nullptr: nothing); bad_row(row, &stat): what is wrong with a row, or nullptr and its
// statistic.
template <typename T, typename BadRow>
static int set_seg_table(mt3_engine* e, SegTableHost<T>& tb, const std::string& fn, const std::string& noun, const T* h_rows,
                         int n, int stride, const char* bad_stride, const int32_t* h_seg, int n_segments, BadRow bad_row) {
  const bool clear = !h_rows || n == 0;
  std::vector<int> stat;
  // ---- what is wrong with the arguments themselves, then with the engine's state; nothing below touches the device before
  if (n < 0) return mt3::fail(MT3_ERR_INVALID, fn + "n_" + noun + "s must not be negative");
  if (!clear) {
    if (bad_stride) return mt3::fail(MT3_ERR_INVALID, fn + bad_stride);
    if (!h_seg && n > 1) return mt3::fail(MT3_ERR_INVALID, fn + "several " + noun + "s need a per-segment index");
    if (h_seg && n_segments < 1)
      return mt3::fail(MT3_ERR_INVALID, fn + "n_segments must be positive with a per-segment index");
    if (h_seg)
      for (int i = 0; i < n_segments; ++i)
        if (h_seg[i] < -1 || h_seg[i] >= n)
          return mt3::fail(MT3_ERR_INVALID, fn + noun + " index outside [-1, n_" + noun + "s)");
    stat.resize(static_cast<size_t>(n));
    for (int r = 0; r < n; ++r)
      if (const char* bad = bad_row(h_rows + static_cast<size_t>(r) * stride, &stat[r]))
        return mt3::fail(MT3_ERR_INVALID, fn + bad);
  }
  if (!e->finalized) return mt3::fail(MT3_ERR_INVALID, fn + "engine not finalized");
  if (e->pending.active) return mt3::fail(MT3_ERR_INVALID, fn + "a decode is in flight");
  if (clear) {
    tb.n = 0;
    return MT3_OK;
  }
  // a setup call: nothing a caller enqueued earlier may still read the rows this call replaces
  MT3_HIP_CHECK(hipDeviceSynchronize());
  const size_t n_elems = static_cast<size_t>(n) * stride, n_seg = h_seg ? static_cast<size_t>(n_segments) : 0;
  // the table's step graphs hold the addresses of both arrays, the stride and whether the index is in use: when a larger
  // array, another stride or the other form replaces what they captured they go
  bool stale = tb.rows && ((n_seg > 0) != tb.seg_on || stride != tb.stride);
  MT3_TRY(grow(e, &tb.rows, &tb.rows_cap, n_elems, &stale));
  MT3_TRY(grow(e, &tb.seg, &tb.seg_cap, n_seg, &stale));
  if (stale) drop_group_graphs(e);
  tb.n = 0;                       // (a failed copy leaves the table out of use, not half set)
  MT3_HIP_CHECK(hipMemcpy(tb.rows, h_rows, n_elems * sizeof(T), hipMemcpyHostToDevice));
  if (n_seg) MT3_HIP_CHECK(hipMemcpy(tb.seg, h_seg, n_seg * 4, hipMemcpyHostToDevice));
  tb.seg_on = n_seg > 0;
  tb.stride = stride;
  tb.seg_host.assign(h_seg, h_seg + n_seg);
  tb.rows_host.assign(h_rows, h_rows + n_elems);
  tb.stat = stat;
  tb.n = n;
  return MT3_OK;
}
}  // extern "C++"

int mt3_debug_engine_set_eos_schedule(mt3_engine* e, const int32_t* h_lengths, int32_t n) {
  if (!e || !e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_set_eos_schedule: engine not finalized");
  if (e->pending.active) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_set_eos_schedule: a decode is in flight");
  if (!h_lengths) {
    e->eos_on = false;
    return MT3_OK;
  }
  if (n <= 0) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_set_eos_schedule: n must be positive");
  // a schedule per SEGMENT of an mt3_engine_transcribe call: a larger array (the captured step graphs hold the old
  // address, so they go)
  bool stale = false;
  MT3_TRY(grow(e, &e->eos_at, &e->eos_cap, static_cast<size_t>(n), &stale));
  if (stale) drop_group_graphs(e);
  std::vector<int32_t> h(static_cast<size_t>(e->eos_cap), 0x7fffffff);       // rows / segments past n: never
  for (int i = 0; i < n; ++i) {
    if (h_lengths[i] < 1) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_set_eos_schedule: lengths must be >= 1");
    h[i] = h_lengths[i];
  }
  MT3_HIP_CHECK(hipMemcpy(e->eos_at, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  e->eos_on = true;
  return MT3_OK;
}

int mt3_engine_set_token_masks(mt3_engine* e, const uint32_t* h_masks, int32_t n_masks, const int32_t* h_seg_mask,
                               int32_t n_segments) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_token_masks: null engine");
  const int vocab = e->cfg.vocab_size;
  return set_seg_table(e, e->tm, "mt3_engine_set_token_masks: ", "mask", h_masks, n_masks, (vocab + 31) / 32, nullptr,
                       h_seg_mask, n_segments,
                       [vocab](const uint32_t* m, int* allowed) { return mt3k::bad_token_mask(m, vocab, allowed); });
}

int mt3_engine_set_prompts(mt3_engine* e, const int32_t* h_prompts, int32_t n_prompts, int32_t stride,
                           const int32_t* h_seg_prompt, int32_t n_segments) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_prompts: null engine");
  const int vocab = e->cfg.vocab_size;
  const char* bad_stride = stride < 1                         ? "stride must be at least 1"
                           : stride >= e->cfg.max_decode_len ? "stride must be below max_decode_len"
                                                             : nullptr;
  return set_seg_table(e, e->tp, "mt3_engine_set_prompts: ", "prompt", h_prompts, n_prompts, stride, bad_stride, h_seg_prompt,
                       n_segments,
                       [=](const int* p, int* len) { return mt3k::bad_prompt(p, stride, vocab, len); });
}

int mt3_engine_set_token_grammar(mt3_engine* e, const mt3_token_grammar* g) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_token_grammar: null engine");
  if (g)
    if (const char* bad = mt3k::bad_token_grammar(*g, e->cfg.vocab_size))
      return mt3::fail(MT3_ERR_INVALID, std::string("mt3_engine_set_token_grammar: ") + bad);
  if (!e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_token_grammar: engine not finalized");
  if (e->pending.active) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_token_grammar: a decode is in flight");
  if (e->nt.on) {                 // the note grammar's `g` is the engine's grammar: it is not this call's to replace or clear
    if (g) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_token_grammar: a note grammar is set (clear it first)");
    return MT3_OK;
  }
  if (!g) {
    e->gr.on = 0;                 // (the descriptor stays: the grammar's step graphs hold it and serve the same one again)
    return MT3_OK;
  }
  // the grammar's step graphs hold the descriptor by value: another one and they go
  if (e->gr_seen && std::memcmp(&e->gr.g, g, sizeof(*g)) != 0) {
    MT3_HIP_CHECK(hipDeviceSynchronize());
    drop_group_graphs(e);
  }
  e->gr.g = *g;
  e->gr.on = 1;
  e->gr_seen = true;
  return MT3_OK;
}

int mt3_engine_set_note_grammar(mt3_engine* e, const mt3_note_grammar* n) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_note_grammar: null engine");
  if (n)
    if (const char* bad = mt3k::bad_note_grammar(*n, e->cfg.vocab_size))
      return mt3::fail(MT3_ERR_INVALID, std::string("mt3_engine_set_note_grammar: ") + bad);
  if (!e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_note_grammar: engine not finalized");
  if (e->pending.active) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_note_grammar: a decode is in flight");
  if (n && e->gr.on && !e->nt.on)
    return mt3::fail(MT3_ERR_INVALID, "mt3_engine_set_note_grammar: a token grammar is set (clear it first)");
  if (!n && !e->nt.on) return MT3_OK;
  if (n && !e->note) {            // the slots' note states: 2 KiB per slot at the largest descriptor, and as much scratch
    const size_t Bm = static_cast<size_t>(e->cfg.max_batch);
    const size_t table = static_cast<size_t>(MT3_NOTE_MAX_PROGRAMS) * MT3_NOTE_ROW_WORDS * 4;
    MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->nrow), Bm * MT3_NOTE_ROW_WORDS * 4));
    MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->held), Bm * table));
    MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->cs_held), Bm * table));
    MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->note), Bm * 4));
  }
  // the step graphs hold the descriptor and the state pointers by value: setting, changing or clearing drops them
  MT3_HIP_CHECK(hipDeviceSynchronize());
  drop_group_graphs(e);
  if (!n) {
    e->nt.on = 0;
    e->gr.on = 0;
    return MT3_OK;
  }
  e->nt.n = *n;
  e->nt.on = 1;
  e->gr.g = n->g;
  e->gr.on = 1;
  e->gr_seen = true;
  return MT3_OK;
}

// The sampled step graphs hold whether the Philox keys come from a seed table: the other form and they go.  Unlike the
// streams' samp_seen there is no "never set" state: a sampled step may have been captured, without a table, before the
// seeds setter was ever called.  table == false takes the table out of use.
static int seed_table_form(mt3_engine* e, bool table) {
  if (!table) e->sseed.n = 0;
  if (e->seed_table != table) {
    MT3_HIP_CHECK(hipDeviceSynchronize());
    drop_group_graphs(e);
  }
  e->seed_table = table;
  return MT3_OK;
}

int mt3_engine_set_sampling_seeds(mt3_engine* e, const uint64_t* h_seg_seed, int32_t n_segments) {
  const std::string fn = "mt3_engine_set_sampling_seeds: ";
  if (!e) return mt3::fail(MT3_ERR_INVALID, fn + "null engine");
  if (h_seg_seed && n_segments < 1) return mt3::fail(MT3_ERR_INVALID, fn + "n_segments must be positive");
  if (h_seg_seed && e->finalized && !e->pending.active && !e->samp_on)
    return mt3::fail(MT3_ERR_INVALID, fn + "sampling is not set (mt3_engine_set_sampling comes first)");
  // a per-segment table of one entry per row behind the identity index, as the streams are; the shared body refuses an
  // engine that is not finalized or has a decode in flight before it touches the device
  const bool table = h_seg_seed != nullptr;
  std::vector<int32_t> ident(table ? static_cast<size_t>(n_segments) : 0);
  for (size_t i = 0; i < ident.size(); ++i) ident[i] = static_cast<int32_t>(i);
  const int rc = set_seg_table(e, e->sseed, fn, "seed", h_seg_seed, table ? n_segments : 0, 1, nullptr,
                               table ? ident.data() : nullptr, n_segments, [](const uint64_t*, int* stat) {
                                 *stat = 0;
                                 return static_cast<const char*>(nullptr);
                               });
  if (rc != MT3_OK) {
    // a copy that failed has left the table out of use (a refusal leaves it as it was): the graphs that hold it go too
    if (!e->sseed.n && e->seed_table) {
      const std::string why = mt3_last_error();
      (void)seed_table_form(e, false);
      return mt3::fail(rc, why);
    }
    return rc;
  }
  return seed_table_form(e, table);
}

int mt3_engine_set_sampling(mt3_engine* e, const mt3_sampling* sp, const uint64_t* h_seg_stream, int32_t n_segments) {
  const std::string fn = "mt3_engine_set_sampling: ";
  if (!e) return mt3::fail(MT3_ERR_INVALID, fn + "null engine");
  if (sp) {
    if (const char* bad = mt3s_bad_params(sp)) return mt3::fail(MT3_ERR_INVALID, fn + bad);
    if (e->cfg.vocab_size > MT3_SAMPLING_MAX_VOCAB)
      return mt3::fail(MT3_ERR_INVALID, fn + "sampling needs a vocabulary of at most 2048");
    if (h_seg_stream && n_segments < 1) return mt3::fail(MT3_ERR_INVALID, fn + "n_segments must be positive with h_seg_stream");
  }
  // the streams are a per-segment table of one entry per row behind the identity index (no streams, or clearing: no table);
  // the shared body refuses an engine that is not finalized or has a decode in flight before it touches the device
  const bool table = sp && h_seg_stream;
  std::vector<int32_t> ident(table ? static_cast<size_t>(n_segments) : 0);
  for (size_t i = 0; i < ident.size(); ++i) ident[i] = static_cast<int32_t>(i);
  MT3_TRY(set_seg_table(e, e->sstream, fn, "stream", table ? h_seg_stream : nullptr, table ? n_segments : 0, 1, nullptr,
                        table ? ident.data() : nullptr, n_segments, [](const uint64_t*, int* stat) {
                          *stat = 0;
                          return static_cast<const char*>(nullptr);
                        }));
  if (!sp) {
    e->samp_on = false;
    return seed_table_form(e, false);        // clearing sampling clears the per-segment seeds too
  }
  e->samp_on = false;             // (a failed copy leaves sampling off, not half set)
  // a setup call: nothing a caller enqueued earlier may still read the parameters this call replaces
  MT3_HIP_CHECK(hipDeviceSynchronize());
  // the sampled step graphs hold whether the streams come from a table: the other form and they go
  if (e->samp_seen && e->samp_table != table) drop_group_graphs(e);
  e->samp_seen = true;
  e->samp_table = table;
  if (!e->samp) MT3_TRY(dmalloc(e, reinterpret_cast<void**>(&e->samp), sizeof(mt3_sampling)));
  MT3_HIP_CHECK(hipMemcpy(e->samp, sp, sizeof(mt3_sampling), hipMemcpyHostToDevice));
  e->samp_on = true;
  return MT3_OK;
}

int mt3_debug_engine_set_score_chunk(mt3_engine* e, int32_t segments) {
  if (!e || !e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_set_score_chunk: engine not finalized");
  if (segments < 0 || segments > e->cfg.max_batch)
    return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_set_score_chunk: segments must be in 0 .. max_batch");
  e->score_chunk_req = segments;
  return MT3_OK;
}

int mt3_debug_engine_poison_caches(mt3_engine* e, int32_t pattern, int32_t cross, void* stream) {
  if (!e || !e->finalized) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_poison_caches: engine not finalized");
  if (e->pending.active) return mt3::fail(MT3_ERR_INVALID, "mt3_debug_engine_poison_caches: a decode is in flight");
  const mt3_engine_config& c = e->cfg;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t heads = static_cast<size_t>(c.max_batch) * c.num_heads;
  for (LayerDev& L : e->dec) {
    const size_t kvb = heads * c.max_decode_len * 64 * e->kv_esize;
    MT3_HIP_CHECK(hipMemsetAsync(L.self_k, pattern, kvb, s));
    MT3_HIP_CHECK(hipMemsetAsync(L.self_v, pattern, kvb, s));
    if (L.self_scale) MT3_HIP_CHECK(hipMemsetAsync(L.self_scale, pattern, heads * c.max_decode_len * sizeof(float2), s));
    if (cross) {
      MT3_HIP_CHECK(hipMemsetAsync(L.cross_kv, pattern, 2 * heads * c.input_length * 64 * e->kv_esize, s));
      if (L.cross_scale) MT3_HIP_CHECK(hipMemsetAsync(L.cross_scale, pattern, heads * c.input_length * sizeof(float2), s));
    }
  }
  return MT3_OK;
}

int mt3_engine_status(const mt3_engine* e, int32_t what) {
  if (!e) return mt3::fail(MT3_ERR_INVALID, "mt3_engine_status: null engine");
  switch (what) {
    case MT3_STATUS_GRAPH_FALLBACKS: return e->graph_fallbacks.load();
    case MT3_STATUS_LAST_DECODE_USED_GRAPH: return e->last_used_graph;
    case MT3_STATUS_RESIDUAL_SPLIT: return e->y_split ? 1 : 0;
    case MT3_STATUS_KV_FP8: return e->kv_fp8 ? 1 : 0;
    case MT3_STATUS_DENSE_FP8: return e->dense_fp8 ? 1 : 0;
    case MT3_STATUS_Q_FOLD: return e->q_fold ? 1 : 0;
    case MT3_STATUS_QKV_FOLD: return e->qkv_fold ? 1 : 0;
    case MT3_STATUS_LAST_DECODE_GROUPS: return e->last_groups;
    case MT3_STATUS_PARTITION_FALLBACKS: return e->part_failed;
    case MT3_STATUS_LAST_DECODE_COMPACTIONS: return e->compactions;
    case MT3_STATUS_LAST_DECODE_FORKS: return e->h_pinned ? e->h_pinned[kForksPinned] : 0;
    case MT3_STATUS_SCORE_CHUNKS: return e->score_chunks;
    case MT3_STATUS_SCORE_ENCODER_PASSES: return e->score_passes;
    case MT3_STATUS_TOKEN_MASKS: return e->tm.n;
    case MT3_STATUS_PROMPTS: return e->tp.n;
    case MT3_STATUS_TOKEN_GRAMMAR: return e->gr.on && !e->nt.on ? 1 : 0;
    case MT3_STATUS_NOTE_GRAMMAR: return e->nt.on ? 1 : 0;
    case MT3_STATUS_SAMPLING: return e->samp_on ? 1 : 0;
    default: return mt3::fail(MT3_ERR_INVALID, "mt3_engine_status: unknown item");
  }
}

}  // extern "C"
