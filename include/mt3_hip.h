/*
 * mt3_hip.h -- C ABI of libmt3hip.so, the MI355X (gfx950) engine for the MT3
 * audio -> notes inference path.
 *
 * The reference (magenta/mt3) has no FFI layer: its boundary is a Python class,
 * `InferenceModel` (colab/music_transcription_with_transformers.ipynb, cell
 * "Imports and Definitions"), plus the t5x write_fn in mt3/inference.py:34-138.
 * Each entry point below replaces the *compiled work* behind one reference call;
 * the Python mirror in mt3_amd/ keeps the reference's names on top of it
 * (see INTEGRATION.md for the ctypes binding a reference maintainer would add).
 *
 * Conventions
 *   - every function returns int: 0 = MT3_OK, negative = mt3_status;
 *     mt3_last_error() gives a message for the calling thread.
 *   - no exception crosses the ABI; no torch / C++ types in signatures.
 *   - `d_*` pointers are DEVICE pointers owned by the caller (torch tensors in
 *     the Python mirror); `h_*` are host pointers.  The library never frees or
 *     reallocates caller memory.  Work is enqueued on `stream` (a hipStream_t
 *     passed as void*) and the call returns without synchronising, EXCEPT:
 *     mt3_engine_load_weight / mt3_engine_finalize (setup), the pure-host
 *     functions, and mt3_engine_decode -- which (a) with MT3_DECODE_EARLY_EXIT
 *     waits for the device at every poll, and (b) on the row-group schedule
 *     (batches of >= 128 rows, see "Schedule" there) returns only when the decode
 *     has FINISHED on the device, unless the caller passes MT3_DECODE_ASYNC and
 *     joins with mt3_engine_decode_wait (the caller's thread is free in between);
 *     and mt3_engine_transcribe, which returns when the whole job is done (the
 *     calling thread drives the encoder passes meanwhile).  While they wait for the
 *     device the engine's threads SLEEP (event polls between naps), they do not spin.
 *   - one engine per (device, stream); an engine is not thread-safe, distinct
 *     engines are independent.  An engine owns up to four worker threads (one
 *     per row group; created with the first decode that needs them, joined by
 *     mt3_engine_destroy) and four streams with hardware queues of their own.
 *     Those streams are BLOCKING streams in HIP's sense: work the application
 *     puts on the legacy NULL stream while a decode runs serialises with them
 *     (pass an explicit stream, as every caller of this header does anyway).
 *     mt3_engine_decode must not be called while `stream` is being captured.
 */
#ifndef MT3_HIP_H_
#define MT3_HIP_H_

#include <math.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mt3_status {
  MT3_OK = 0,
  MT3_ERR_INVALID = -1,   /* bad argument / shape / state                      */
  MT3_ERR_HIP = -2,       /* a HIP runtime call failed (no GPU, OOM, launch)   */
  MT3_ERR_CAPACITY = -3,  /* caller's output buffer too small; size returned   */
  MT3_ERR_MISSING = -4    /* weight not loaded / unknown weight name           */
} mt3_status;

const char* mt3_last_error(void);
int mt3_abi_version(void);

/* ------------------------------------------------------------------ frontend
 * Replaces spectrograms.compute_spectrogram -> spectral_ops.compute_logmel
 * (mt3/spectrograms.py:64-73, mt3/spectral_ops.py:29-88) as called per segment by
 * preprocessors.compute_spectrograms (mt3/preprocessors.py:613-618), plus the
 * zero-fill of short segments done later by the feature converter
 * (mt3/models.py:48-98): frames >= n_frames[s] are written as 0.0, not log(eps).
 */
typedef struct mt3_frontend_config {
  int32_t sample_rate;   /* 16000  spectrograms.py:23 */
  int32_t hop_width;     /* 128    spectrograms.py:24 */
  int32_t num_mel_bins;  /* 512    spectrograms.py:25 */
  int32_t fft_size;      /* 2048   spectrograms.py:28 */
  float lo_hz;           /* 20.0   spectrograms.py:29 */
  float hi_hz;           /* 7600.0 spectral_ops.py:79 */
  int32_t table_dtype;   /* arithmetic the Hann window and the mel matrix are BUILT in.  0 (default): float32 in
                            TensorFlow's op order -- tf.signal.stft's window and linear_to_mel_weight_matrix default to
                            dtype=float32 and the reference passes none (spectral_ops.py:42-47,69-71), so this is the side
                            of the <= 2.8e-3 log-domain gap between the two evaluations the reference most likely sits on
                            [TF's op order restated from memory: still unpinned against TensorFlow itself];
                            1: float64, rounded once (rounds 1-4) */
} mt3_frontend_config;

typedef struct mt3_frontend mt3_frontend;

int mt3_frontend_create(const mt3_frontend_config* cfg, mt3_frontend** out);
void mt3_frontend_destroy(mt3_frontend* fe);
/* number of non-zero mel weights and a copy of the dense [fft/2+1, mel] f32 matrix
 * the kernel was built from (for parity tests) */
int mt3_frontend_mel_matrix(const mt3_frontend* fe, float* h_out /*[(fft/2+1)*mel]*/, int64_t* nnz);
/* d_audio  [n_segments, frames_per_segment*hop] f32 (segment s uses its first
 *          h_n_frames[s]*hop samples; the rest is ignored)
 * d_logmel [n_segments, frames_per_segment, num_mel_bins] f32 */
int mt3_frontend_logmel(mt3_frontend* fe, const float* d_audio, int32_t n_segments,
                        int32_t frames_per_segment, const int32_t* h_n_frames /* may be NULL = all full */,
                        float* d_logmel, void* stream);
/* mt3_frontend_logmel passes h_n_frames to the kernel BY VALUE (1024 counts per launch; longer calls are issued in
 * pieces): the caller's host buffer is free when the call returns, nothing is allocated, copied, locked or waited for on
 * the call path, any number of host threads and streams may call, and a stream may be under capture.
 * mt3_frontend_logmel_dev: the same with the counts already in DEVICE memory (caller-owned, must stay valid until the
 * launch has run). */
int mt3_frontend_logmel_dev(mt3_frontend* fe, const float* d_audio, int32_t n_segments,
                            int32_t frames_per_segment, const int32_t* d_n_frames /* may be NULL */,
                            float* d_logmel, void* stream);

/* ---------------------------------------------------------------- resampler
 * Replaces the host resample inside note_seq.audio_io.wav_data_to_samples_librosa (NB cell 2,
 * `wav_data_to_samples_librosa(wav, sample_rate=16000)` before `inference_model(audio)`), which the Python mirror
 * evaluates as mt3_amd/audio_io.resample: scipy.signal.resample_poly(x, up, down, window=w) with the default padtype
 * (zeros outside x) and resampy's kaiser_best filter.  The device computes exactly
 *   n_out = ceil(n_in * up / down)
 *   y[n]  = float32( sum_k x[k] * h_taps[n*down + half - k*up] ),  n < n_out,  half = (n_taps - 1) / 2
 * (taps whose index falls outside [0, n_taps) and inputs outside [0, n_in) contribute nothing), every product and the
 * sum in float64: the same samples as resample_poly on the host, to the last bit or within one f32 ulp where
 * the two summation orders round differently.
 * mt3_resample_output_length: n_out in int64 (-1 for n_in < 0, up < 1 or down < 1).
 * mt3_resampler_create: h_taps = resample_poly's window ALREADY multiplied by `up` (resample_poly applies w * up), odd
 *   n_taps <= 2^20, up/down in lowest terms; the table is reordered phase-major and uploaded once (setup call,
 *   synchronous).  MT3_ERR_INVALID for a NULL pointer, an even or non-positive n_taps, more than 2^20 taps, up < 1,
 *   down < 1 or gcd(up, down) != 1.
 * mt3_resampler_run: d_in [n_in] f32 -> d_out [out_capacity] f32: y[0 .. n_out) and 0.0 in [n_out, out_capacity),
 *   nothing written at or past out_capacity (so d_out may be the frontend's zero-padded [n_segments, T*hop] buffer).
 *   MT3_ERR_INVALID for a NULL pointer, n_in < 1 or out_capacity < n_out.  Same contract as mt3_frontend_logmel:
 *   one launch enqueued on `stream`, nothing allocated, copied or waited for; a resampler is read-only after create,
 *   so any number of threads and streams may run it.
 */
typedef struct mt3_resampler mt3_resampler;

int64_t mt3_resample_output_length(int64_t n_in, int32_t up, int32_t down);
int mt3_resampler_create(const double* h_taps /* w * up, [n_taps] */, int64_t n_taps, int32_t up, int32_t down,
                         mt3_resampler** out);
void mt3_resampler_destroy(mt3_resampler* r);
int mt3_resampler_run(mt3_resampler* r, const float* d_in, int64_t n_in, float* d_out, int64_t out_capacity,
                      void* stream);

/* --------------------------------------------------------------- PCM decode
 * Replaces the sample decode and the channel mixdown inside note_seq.audio_io.wav_data_to_samples_librosa (NB cell 2),
 * which the Python mirror evaluates as mt3_amd/audio_io.read_wav: scipy.io.wavfile.read, the integer types scaled to
 * [-1, 1) in float32, `mean(axis=1)` over the channels.  The caller uploads the WAV file's data chunk as it is
 * (interleaved little-endian frames, `channels` samples each) and the device computes, per sample,
 *   MT3_PCM_U8   1 byte unsigned            (float(v) - 128) / 128
 *   MT3_PCM_S16  2 bytes                    float(v) / 2^15
 *   MT3_PCM_S24  3 bytes packed             float(int32(b0 << 8 | b1 << 16 | b2 << 24)) / 2^31   (left-justified)
 *   MT3_PCM_S32  4 bytes                    float(v) (round to nearest even) / 2^31
 *   MT3_PCM_F32  4 bytes IEEE               v  (NaN, infinities and -0.0 pass through)
 *   MT3_PCM_F64  8 bytes IEEE               float(v) (round to nearest even)
 * and per frame of C = `channels` samples
 *   C = 1        the sample itself
 *   2 <= C <= 7  acc = +0.0f; acc = acc + s_c for c = 0 .. C-1 in float32; acc / float(C), correctly rounded
 * which is numpy's mean over fewer than 8 addends: the same bits as read_wav on the host.  8 or more channels are not
 * covered (numpy sums those with eight partial accumulators); the Python mirror decodes such files on the host.
 * d_pcm is aligned to the size of one sample; MT3_PCM_S24 needs byte alignment only.
 * mt3_pcm_decode: d_out[0 .. n_frames) = the mono samples, +0.0 in [n_frames, out_capacity), nothing written at or
 *   past out_capacity (d_out may be the frontend's [n_segments, T*hop] buffer: the path of a 16 kHz file).
 * mt3_resampler_run_pcm: what mt3_resampler_run gives on those mono samples, bit for bit; the frames are decoded as
 *   the kernel stages its input, so the mono float32 array never exists in device memory.
 * Both: one launch enqueued on `stream`, nothing allocated, copied or waited for.  MT3_ERR_INVALID, before any HIP
 * call, for a NULL pointer, n_frames < 1, channels outside 1 .. 7, an unknown format, out_capacity below the output
 * length, or sizes whose index arithmetic would leave int64.
 */
enum { MT3_PCM_U8 = 0, MT3_PCM_S16 = 1, MT3_PCM_S24 = 2, MT3_PCM_S32 = 3, MT3_PCM_F32 = 4, MT3_PCM_F64 = 5 };
#define MT3_PCM_MAX_CHANNELS 7

int mt3_pcm_decode(const void* d_pcm, int64_t n_frames, int32_t channels, int32_t format, float* d_out,
                   int64_t out_capacity, void* stream);
int mt3_resampler_run_pcm(mt3_resampler* r, const void* d_pcm, int64_t n_frames, int32_t channels, int32_t format,
                          float* d_out, int64_t out_capacity, void* stream);

/* -------------------------------------------------------------------- engine
 * Replaces network.Transformer (mt3/network.py:265-409, layers in mt3/layers.py)
 * as driven by t5x predict_batch_with_aux through
 * models.ContinuousInputsEncoderDecoderModel (mt3/models.py:121-152):
 * encode once, cross-K/V once, then up to `max_decode_len` cached decode steps.
 */
typedef enum mt3_dtype { MT3_BF16 = 0, MT3_F32 = 1, MT3_FP8_E4M3 = 2 /* K/V caches and the encoder's dense layers only: OCP e4m3fn */ } mt3_dtype;

typedef struct mt3_engine_config {   /* network.T5Config (network.py:25-41), model.gin:47-59 */
  int32_t vocab_size;           /* 1536 (mt3) / 1664 (ismir2021): vocabularies.num_embeddings */
  int32_t emb_dim;              /* 512  */
  int32_t num_heads;            /* 6    */
  int32_t head_dim;             /* 64 (only 64 is supported by the attention kernels) */
  int32_t mlp_dim;              /* 1024 */
  int32_t num_encoder_layers;   /* 8    */
  int32_t num_decoder_layers;   /* 8    */
  int32_t input_depth;          /* 512 = spectrograms.input_depth */
  int32_t input_length;         /* T: 256 (mt3) / 512 (ismir2021) encoder frames */
  int32_t max_decode_len;       /* L: 1024 */
  int32_t max_batch;            /* segments per call the workspaces are sized for */
  int32_t compute_dtype;        /* mt3_dtype: MFMA operand type; accumulation is always f32 */
  int32_t decode_chains;        /* 0/1: one chain; n <= 8: the decode batch is dealt to n independent row groups
                                   that run as parallel branches of the step graph (same results, bit for bit) */
  int32_t kv_cache_dtype;       /* 0: K/V caches in the compute dtype.  MT3_FP8_E4M3 (with MT3_BF16 compute): self- and
                                   cross-attention K/V rows are cached as OCP e4m3 bytes + one power-of-two scale per
                                   (row, head, position) -- half the bytes the HBM-bound decode step streams
                                   (BASELINE configs[4] "fp8 path"; tolerances in DESIGN.md section 4) */
  int32_t dense_dtype;          /* 0: every dense layer in the compute dtype.  MT3_FP8_E4M3 (with MT3_BF16 compute): the
                                   ENCODER's dense layers and the cross-attention K/V projections (the MFMA-bound 99 % of
                                   the encoder's FLOPs) run as MXFP8 -- e4m3 operands with one E8M0 scale per 32 K
                                   elements on v_mfma_scale_f32_16x16x128_f8f6f4, weights quantised once at finalize,
                                   activations by the producing epilogue; the decode step's M = batch GEMMs stay bf16
                                   (they are launch-latency-bound) */
  int32_t options;              /* bit set of MT3_OPT_* below; 0 = the defaults every number in DESIGN.md is quoted on */
} mt3_engine_config;

/* mt3_engine_config.options: numerics-relevant choices of HOW the same function is evaluated (all variants stay inside
 * the tolerances of DESIGN.md section 4; the tests compare them with each other) */
enum {
  /* DECODER: keep the residual stream as ONE f32 stream with in-kernel RMSNorm statistics (the f32 engine always
   * does; the bf16 engine otherwise carries f32 rows + bf16 copy + per-16-column sums of squares) */
  MT3_OPT_SINGLE_RESIDUAL_STREAM = 1,
  /* the same choice for the ENCODER's residual rows (the split form is what feeds the LDS-DMA staged GEMM tile) */
  MT3_OPT_ENCODER_SINGLE_RESIDUAL_STREAM = 4,
  /* decoder: the projections that consume a freshly updated residual row (cross-attention query; next layer's
   * q/k/v) get a launch of their own instead of riding as extra output columns in the neighbouring launches
   * (linearity of the residual update) */
  MT3_OPT_SEPARATE_PROJECTIONS = 2,
  /* decoder: only the q / k / v (+ cross-query) projection of a layer's INPUT row keeps its own launch (otherwise it
   * rides in the previous layer's MLP out-projection launch, and layer 0's comes from two table rows); the
   * cross-attention query stays folded */
  MT3_OPT_SEPARATE_QKV_PROJECTION = 8,
  /* never use the row-group decode schedule (see mt3_engine_decode): every decode stays on the caller's stream */
  MT3_OPT_NO_ROW_GROUPS = 16,
  /* f32 engine: keep the encoder's dense layers and attention on the f32 matrix instruction (v_mfma_f32_16x16x4_f32).  By
   * default they multiply on the bf16 pipes with every f32 operand split EXACTLY into three bf16 terms and the six
   * significant products accumulated in f32 -- at least as exact as the f32 instruction (measured 1.3e-7 against 2.1e-7
   * of sum |p| on a K = 512 dot product) at 2.7x its rate; DESIGN.md section 3 */
  MT3_OPT_ENCODER_F32_MFMA = 32,
  /* host side only (no numerics): the engine's worker threads SPIN while they wait for the device (hipStreamSynchronize,
   * the runtime's own queue back-pressure) as they did up to round 4.  By default a worker keeps at most two windows
   * of 16 decode steps enqueued ahead of the device and, for the older one, POLLS an event (hipEventQuery) between naps of
   * 20 us growing to 200 us (hipEventSynchronize spins on this runtime even for hipEventBlockingSync events, so the nap is
   * explicit); the final wait of a decode and the polls of MT3_DECODE_EARLY_EXIT / mt3_engine_transcribe sleep the same
   * way.  Cost: a completion is noticed up to one nap (<= 200 us) late -- once at the end of a call, and per early-exit
   * poll on the path that decides when to stop (1.25 instead of 5.5 CPU-seconds per 1.10 s decode, same decode time) */
  MT3_OPT_SPIN_WAITS = 64
};

typedef struct mt3_engine mt3_engine;

int mt3_engine_create(const mt3_engine_config* cfg, mt3_engine** out);
void mt3_engine_destroy(mt3_engine* e);
/* Flax parameter names of the reference tree joined by '/', e.g.
 * "encoder/layers_0/attention/query/kernel" (SURVEY.md A.3); h_data is f32,
 * row-major, in the reference's own [in, out] orientation. */
int mt3_engine_load_weight(mt3_engine* e, const char* name, const float* h_data,
                           const int64_t* shape, int32_t ndim);
/* folds norm scales, fuses QKV / gate matrices, converts to compute dtype, uploads */
int mt3_engine_finalize(mt3_engine* e);
int64_t mt3_engine_device_bytes(const mt3_engine* e);

/* Transformer.encode (network.py:275-301) + cross-attention K/V of every decoder
 * layer (layers.py:239-240, hoisted out of the decode loop).
 * d_inputs [batch, T, input_depth] f32.  d_encoded_f32 [batch, T, emb] f32 or NULL.
 * Reproducibility across batch sizes: the f32 engine gives a segment the SAME bits whatever batch it is encoded in (one
 * tile family at every size since round 5).  The bf16 engine has two tile families -- passes of fewer than 2048 rows
 * (8 segments at T = 256) take the decode-sized tiles, whose f32 sums are rounded to bf16 in other places -- so a
 * segment's bf16 encoder output can differ in the last bf16 bit between a pass of < 8 and one of >= 8 segments (both within
 * the bf16 bounds of DESIGN.md section 4); mt3_engine_transcribe pads its chunks to 8 segments for that reason. */
int mt3_engine_encode(mt3_engine* e, const float* d_inputs, int32_t batch,
                      float* d_encoded_f32, void* stream);

/* Autoregressive decode (BOS=0, EOS=1; ids after a row's EOS are 0): the loop t5x
 * `predict_batch_with_aux` drives over Transformer.decode (network.py:303-343).
 * Default: greedy until EOS.  MT3_DECODE_BEAM1: the token selection of t5x
 * `decoding.beam_search` with num_decodes=1, alpha=0.6 (what the reference's
 * InferenceModel.predict_tokens runs): per step the top-2 of log_softmax; the live
 * hypothesis follows the best non-EOS token, an EOS candidate finishes
 * prefix+EOS with score logp/((5+len)/6)^alpha; a row stops once its best finished
 * score exceeds live_logp/((5+L+1)/6)^alpha; the best finished hypothesis is
 * returned, or the live one if none finished.
 * Runs `num_steps` (<= L) steps; each step is one hipGraph replay (per row group) unless
 * flags & MT3_DECODE_NO_GRAPH.  d_ids [batch, L] int32 (columns >= num_steps
 * are zero-filled).  d_first_logits: [batch, vocab] f32 logits of step 0, or NULL.
 * With MT3_DECODE_EARLY_EXIT the host polls a device counter every 32 steps and
 * stops once every row has emitted EOS / finished its search (this synchronises the stream), and finished rows
 * are RETIRED, as the reference's beam_search stops extending finished rows (mt3/models.py:126-127; everything past
 * a row's EOS is cut by _trim_eos anyway, NB:358-363): from the step after a row finishes, the attention kernels stream
 * nothing for it (a wave-uniform exit before the first cache request) and the token kernel skips it; at a poll where
 * the live rows of a row group fit fewer 32-row GEMM tiles than the group occupies, the live rows' per-step state is
 * compacted to the front of the group (a slot -> row map finds their K/V caches, which never move), so attention
 * grids AND the GEMMs' M shrink with the live set.  The ids of every row up to and including its EOS are bit-identical
 * to the schedule without EARLY_EXIT (rows are independent; tests/test_gpu_retire.py).  Without EARLY_EXIT every row
 * runs all `num_steps` steps (the canonical full-length workload bench.py's headline is quoted on).
 * Schedule: a batch of >= 128 rows is decoded as 2 or 4 ROW GROUPS (bf16 operands: 2 from 128 rows, 4 from 512; f32:
 * 2 from 128, 4 from 256 -- with MT3_DECODE_EARLY_EXIT the bf16 rule in f32 as well: the ragged regime is launch latency,
 * two groups measure faster there), each on an engine-owned stream with a hardware queue of its own (created with
 * hipExtStreamCreateWithCUMask and a mask of all compute units: two plain HIP streams serialise)
 * and driven by one of the engine's worker threads (one captured step graph per group, replayed per step;
 * MT3_DECODE_NO_GRAPH: direct launches), so that one group's HBM-bound attention runs beside the other groups'
 * latency-bound GEMMs (+6 % at batch 256 in bf16, +7 % in f32); the groups start after an event on the caller's stream,
 * the ids are bit-identical to the single-stream schedule (rows are independent), and the decode is complete when all
 * groups have FINISHED (each group's thread waits for its stream: a stream nobody waits on runs 7 % slower) -- which is
 * when mt3_engine_decode returns, or, with MT3_DECODE_ASYNC, when mt3_engine_decode_wait does.
 * MT3_DECODE_SINGLE_STREAM / _CHAINS(n), decode_chains > 1 or MT3_OPT_NO_ROW_GROUPS keep everything on `stream`. */
enum {
  MT3_DECODE_NO_GRAPH = 1,
  MT3_DECODE_EARLY_EXIT = 2,
  MT3_DECODE_BEAM1 = 4,
  /* keep the whole decode on the caller's stream (no helper streams): see "Schedule" above */
  MT3_DECODE_SINGLE_STREAM = 8,
  /* return as soon as the decode has been handed to the engine's worker threads; the caller MUST call
   * mt3_engine_decode_wait before it reads d_ids, enqueues anything else on `stream`, or calls any other function of
   * this engine (they fail with MT3_ERR_INVALID while a decode is in flight).  h_steps_run is not written by the
   * asynchronous call (mt3_engine_decode_wait reports it). */
  MT3_DECODE_ASYNC = 16
  /* bits 8..11: number of decode chains for this call (1..8); 0 = the engine's configured default.
   * Any other bit is rejected with MT3_ERR_INVALID (profiling variants live in mt3_hip_debug.h). */
};
#define MT3_DECODE_CHAINS(n) (((n) & 0xF) << 8)
int mt3_engine_decode(mt3_engine* e, int32_t batch, int32_t num_steps, int32_t flags,
                      int32_t* d_ids, float* d_first_logits, int32_t* h_steps_run, void* stream);
/* Joins the decode an MT3_DECODE_ASYNC call started: blocks (sleeping, not spinning) until the engine's worker threads
 * are done, then enqueues the copy of the ids into that call's d_ids on that call's stream (and the beam-1
 * finalisation before it) and reports errors of the decode loop.  MT3_ERR_INVALID when no decode is in flight. */
int mt3_engine_decode_wait(mt3_engine* e, int32_t* h_steps_run);

/* k-beam search: t5x decoding.beam_search(alpha = 0.6) with num_decodes = num_beams = k, 1 <= k <= 8 -- the reference's
 * decode_fn (mt3/models.py:126-127), reached in t5x through predict_batch_with_aux(..., num_decodes=k,
 * return_all_decodes=...).  The rule, written down from memory [from memory: t5x is not at hand; SURVEY.md A.5 has
 * the same status], with NEG_INF = -1e7 and bp(n) = ((5 + n) / 6) ^ 0.6:
 *   start       the k live beams of an element have log-probs [0, NEG_INF, ...] (step 0 expands beam 0 only); the k
 *               finished entries have score NEG_INF (unfilled).
 *   candidates  per step, log_softmax of each live beam's logits plus the beam's log-prob; the top 2k of the k*V
 *               candidates, ties to the lower flattened index beam*V + token (lax.top_k).
 *   finished    a candidate ending in EOS scores logp / bp(t + 1); the k old entries and the new ones are merged and the
 *               k best kept (the old entry on equal scores).
 *   live        the k best candidates not ending in EOS are the new live beams (parent beam + token each).
 *   retirement  an element is retired once its k-th best finished score exceeds its best live log-prob / bp(num_steps + 1):
 *               no later candidate can enter its finished set, so its state is final.  The decode runs num_steps steps, or
 *               with MT3_DECODE_EARLY_EXIT until every element is retired.
 *   result      an element with no finished entry returns its k live beams and their log-probs; one with at least one
 *               returns its finished set only (unfilled entries: score NEG_INF, all-zero ids).  The k decodes come back
 *               in INCREASING order of score, the best last (as t5x returns them); every decode is padded with 0 after
 *               its EOS.  At k = 1 this is MT3_DECODE_BEAM1, and the ids are bit-identical to it.
 * The candidates' log-softmax is computed per beam in the order MT3_DECODE_BEAM1 uses; within a beam the candidates are
 * ranked by logit (lower id on ties), so an exact tie of two rounded scores in one beam goes to the larger logit.
 * Input: the preceding mt3_engine_encode must have encoded batch * num_beams rows, rows b*k .. b*k + k - 1 all holding
 * segment b (each segment encoded k times in a row: its cross-attention K/V then sit in the cache rows of its k beams).
 * d_ids [batch, L] int32: the best decode.  d_all_ids [batch, k, L] int32 or NULL: all k decodes.  d_scores [batch, k]
 * f32 or NULL: their scores (finished: logp / bp(length incl. EOS); live: logp).  h_steps_run (may be NULL): the steps run.
 * flags: MT3_DECODE_NO_GRAPH, MT3_DECODE_EARLY_EXIT, MT3_DECODE_SINGLE_STREAM; any other bit, num_beams outside 1 .. 8,
 * batch * num_beams > max_batch, or a vocabulary larger than 2048 returns MT3_ERR_INVALID.  The step is one captured
 * graph per row group (the schedule of mt3_engine_decode on batch * k rows; every group boundary is a multiple of k).
 * Each step ends with the beam step and a cache-row pass: a beam whose parent has one child takes over the parent's
 * self-attention cache row (only the slot -> row map changes); the further children of a parent take the rows of
 * parents nobody chose and get positions [0, t] of the parent's K/V copied into them, for every layer and head (with
 * e4m3 caches the scale rows as well) -- MT3_STATUS_LAST_DECODE_FORKS counts those copies.  The call returns when the
 * decode is complete on the device. */
int mt3_engine_decode_beams(mt3_engine* e, int32_t batch, int32_t num_beams, int32_t num_steps, int32_t flags,
                            int32_t* d_ids, int32_t* d_all_ids, float* d_scores, int32_t* h_steps_run, void* stream);

/* Streaming transcription with IN-FLIGHT BATCHING: encode + decode of n_segments independent segments (any number;
 * the reference's loop over `.batch(8)` calls of predict_batch_with_aux, NB:295-301, mt3/models.py:121-152) through the
 * engine's max_batch decode SLOTS.  The reference's decode is batch-synchronous -- a batch ends when its LAST row has
 * terminated (t5x decoding.beam_search's while_loop) -- so a finished row idles until then; here a finished slot hands
 * its id row to the caller and restarts at position 0 on the next segment: every slot carries its own position counter
 * (as the reference's cache index does per call, mt3/layers.py:246-314), self-attention cache rows past a slot's
 * position are discarded by position, and the segment's cross-attention K/V arrive from an encoder pass that ran ahead
 * on the caller's stream (chunks of up to 64 segments into a staging ring; the first min(n_segments, max_batch)
 * segments are encoded straight into the caches).  Row count per row group is constant, so ONE captured step graph per
 * group serves the whole job; when the queue of segments is empty the remaining rows are retired and compacted as
 * under MT3_DECODE_EARLY_EXIT.
 * d_inputs  [n_segments, T, input_depth] f32 (log-mel);  d_ids [n_segments, L] int32: row i = the ids of segment i,
 * bit-identical to what mt3_engine_encode + mt3_engine_decode(MT3_DECODE_EARLY_EXIT) return for that segment (ids after
 * a row's EOS are 0; a row without EOS has num_steps ids).  flags: MT3_DECODE_BEAM1, MT3_DECODE_NO_GRAPH,
 * MT3_DECODE_SINGLE_STREAM (one row group); anything else is rejected.  The call BLOCKS until every segment is done
 * (the calling thread drives the encoder passes, the engine's workers the row groups); d_inputs / d_ids must stay
 * valid until it returns.  h_stats (may be NULL) reports what ran. */
typedef struct mt3_transcribe_stats {
  int32_t slots;           /* decode slots in use = min(n_segments, max_batch)                                   */
  int32_t groups;          /* row groups                                                                         */
  int32_t steps_run;       /* decode steps of the group that ran longest                                         */
  int32_t polls;           /* refill polls (all groups)                                                          */
  int32_t refills;         /* slots restarted on a new segment (= n_segments - slots)                            */
  int32_t starved_polls;   /* polls at which finished slots found no encoded segment waiting (queue not empty)   */
  int32_t encoder_chunks;  /* encoder passes after the first                                                     */
  int32_t compactions;     /* live-row compactions once the queue was empty                                      */
  int32_t used_graph;      /* 1: every group replayed a captured step graph                                      */
  int32_t reserved[7];
} mt3_transcribe_stats;
int mt3_engine_transcribe(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t num_steps, int32_t flags,
                          int32_t* d_ids, mt3_transcribe_stats* h_stats, void* stream);

/* In-flight batching of the k-beam search: mt3_engine_transcribe with the token rule of mt3_engine_decode_beams
 * (num_beams = k, 1 <= k <= 8).  An engine of max_batch rows gives E = min(n_segments, max_batch / k) ELEMENTS of k slots
 * each; an element whose search has closed -- retired by the rule above, or out of positions after num_steps steps --
 * hands its k decodes to the caller and restarts at position 0 on the next segment, while the other elements go on.
 * d_inputs [n_segments, T, input_depth] f32: every segment ONCE (the engine puts a segment's cross-attention K/V into the
 * k cache rows of the element that takes it; every segment, the first E included, comes through the staging ring of
 * encoder passes that run ahead on the caller's stream).  d_ids [n_segments, L] int32: the best decode of each segment.
 * d_all_ids [n_segments, k, L] int32 or NULL and d_scores [n_segments, k] f32 or NULL: all k decodes and their scores in
 * INCREASING order of score, exactly as mt3_engine_decode_beams returns them.
 * Contract: segment i's rows of d_ids, d_all_ids and d_scores are BIT-IDENTICAL to what mt3_engine_encode (the segment k
 * times in a row) + mt3_engine_decode_beams(..., MT3_DECODE_EARLY_EXIT) return for it, under the encoder-reproducibility
 * condition mt3_engine_encode documents (f32: always; bf16: every encoder pass of 8 or more segments -- the staging
 * passes are padded to 8 as in mt3_engine_transcribe).  At k = 1 the ids equal mt3_engine_transcribe(MT3_DECODE_BEAM1).
 * Schedule: the row groups of mt3_engine_transcribe on E * k slots, every group boundary on an element boundary; one
 * captured step graph per group for the whole job; beam groups are never compacted -- a closed element costs no
 * attention, and once the queue of segments is empty a group ends when its last element has closed.
 * flags: MT3_DECODE_NO_GRAPH, MT3_DECODE_SINGLE_STREAM.  MT3_ERR_INVALID, before any device work: any other flag bit,
 * num_beams outside 1 .. 8 or above max_batch, a vocabulary outside [2k, 2048], more than 16 decoder layers, NULL d_inputs
 * or d_ids, n_segments < 1, num_steps outside 1 .. L, a decode in flight, or a synthetic EOS schedule being set
 * (mt3_hip_debug.h: that hook drives the greedy / beam-1 token kernel only).
 * h_stats (may be NULL; written only when the call succeeds) as for mt3_engine_transcribe, in slots: slots = E * k,
 * refills = (n_segments - E) * k, encoder_chunks = all encoder passes, compactions = 0.  MT3_STATUS_LAST_DECODE_FORKS
 * reports the cache-row copies of the whole job.  The call BLOCKS until every segment is done. */
int mt3_engine_transcribe_beams(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t num_beams,
                                int32_t num_steps, int32_t flags, int32_t* d_ids, int32_t* d_all_ids /* NULL ok */,
                                float* d_scores /* NULL ok */, mt3_transcribe_stats* h_stats, void* stream);

/* Several DRAWS of every segment in one job, each segment encoded once (n sampled transcriptions of one recording are the
 * use): mt3_engine_transcribe on a job of n_segments * per draws, draw d = s * per + j being sample j of segment s.
 * d_inputs [n_segments, T, input_depth] f32 holds every segment ONCE; d_ids [n_segments * per, L] int32: row s * per + j is
 * draw j of segment s.  "Segment i" of every per-segment table -- token masks, prompts, sampling streams, sampling seeds
 * (mt3_engine_set_sampling_seeds: what tells the draws of a segment apart) and the synthetic EOS schedule -- means DRAW i:
 * the tables cover n_segments * per entries.  Without sampling the `per` draws of a segment are equal; that is legal.
 * Contract: d_ids is BIT-IDENTICAL to mt3_engine_transcribe on the inputs with each segment `per` times in a row and the
 * same tables set, under the encoder-reproducibility condition mt3_engine_encode documents (f32: always; bf16: every
 * encoder pass of 8 or more segments -- the staging passes are padded to 8 as in mt3_engine_transcribe).
 * Schedule: mt3_engine_transcribe's greedy path with min(n_segments * per, max_batch) slots.  As in
 * mt3_engine_transcribe_beams EVERY draw reaches its slot through the staging ring: the slots start finished and empty,
 * an encoder pass covers up to 64 segments (a short last pass is padded with the segments before it), and the `per` draws
 * of a segment copy the same staged entry into their cache rows.
 * flags: MT3_DECODE_NO_GRAPH, MT3_DECODE_SINGLE_STREAM.  MT3_ERR_INVALID, before any device work: any other flag bit
 * (MT3_DECODE_BEAM1 included: beam-1 does not sample), per < 1, n_segments * per above INT32_MAX / L, and the argument
 * errors of mt3_engine_transcribe (NULL d_inputs or d_ids, n_segments < 1, num_steps outside 1 .. L, more than 16 decoder
 * layers, a decode in flight, a per-segment table or EOS schedule shorter than n_segments * per).
 * h_stats (may be NULL) as for mt3_engine_transcribe: slots as above, refills = n_segments * per - slots, encoder_chunks =
 * ALL encoder passes = ceil(n_segments / 64) (ceil(n_segments / max_batch) below 64 slots).  The call BLOCKS until every
 * draw is done. */
int mt3_engine_transcribe_draws(mt3_engine* e, const float* d_inputs, int32_t n_segments, int32_t per, int32_t num_steps,
                                int32_t flags, int32_t* d_ids /* [n_segments * per][L] */, mt3_transcribe_stats* h_stats,
                                void* stream);

/* Constrained decoding: per-segment token masks (allowed instruments are the use: mt3_codec_token_mask).  What a logit
 * mask ahead of t5x decoding.beam_search does [from memory: t5x is not at hand, as for the beam search above]:
 *   mask     a bit set over the vocabulary, words = ceil(vocab / 32) uint32: bit i % 32 of word i / 32 set = token i allowed.
 *   rule     wherever the token rule reads the logit of a disallowed token it reads -inf: the token is never picked, never
 *            a candidate of the beam-1 top 2 or the k-beam top 2k, and contributes exactly 0 to the log-sum-exp -- the
 *            log-probabilities (live / finished scores) are renormalised over the allowed set.  The tie rules, beam-1 and
 *            k-beam retirement, max_len, the synthetic EOS schedule (it still wins) and the next-input-row write are
 *            unchanged.  Applied in the token kernels after the row scale and its write-back: the logits the engine hands
 *            back (d_first_logits, per-step logits, the rows scaled in place) stay the model's own, unmasked.
 *   segments h_seg_mask [n_segments]: the mask index of segment i, -1 = unconstrained; NULL: mask 0 for every segment
 *            (n_masks must be 1).  In mt3_engine_decode "segment i" is batch row i, in mt3_engine_decode_beams element i,
 *            in mt3_engine_transcribe / mt3_engine_transcribe_beams segment i of the job: the mask follows the segment
 *            through compaction and refills.
 * h_masks [n_masks][words] and h_seg_mask are HOST arrays, copied into engine-owned device memory by this call
 * (synchronous, a setup call like mt3_engine_finalize); h_masks == NULL or n_masks == 0 clears.  The masks stay set for
 * every later mt3_engine_decode / _decode_beams / _transcribe / _transcribe_beams until cleared; masked and unmasked steps
 * never share a captured graph, and an unmasked decode runs the kernels, graphs and bits it ran before masks existed.
 * mt3_engine_decode_forced, mt3_engine_score and mt3_engine_score_segments IGNORE masks (note confidences stay the
 * unconstrained model's log-probabilities).  MT3_STATUS_TOKEN_MASKS reports the number of masks set.
 * MT3_ERR_INVALID, before any device work: n_masks < 0; NULL h_seg_mask with n_masks > 1; n_segments < 1 with h_seg_mask;
 * an index outside [-1, n_masks); a mask that forbids EOS (id 1); a mask that allows fewer than 2 tokens; bits at or past
 * vocab set in the last word; an engine that is not finalized; a decode in flight.
 * The decode / transcribe calls return MT3_ERR_INVALID before any device work for more rows / elements / segments than
 * n_segments when a per-segment index is set and, for the beam calls, a mask in use with fewer than 2 * num_beams allowed
 * tokens. */
int mt3_engine_set_token_masks(mt3_engine* e, const uint32_t* h_masks /* [n_masks][words] */, int32_t n_masks,
                               const int32_t* h_seg_mask /* [n_segments] or NULL */, int32_t n_segments);

/* Prompted decoding: per-segment forced token prefixes -- the `inputs=prompt` of t5x's decode function,
 * which MT3 always passes as zeros.  For MT3 the prefix is the tie section that opens a segment
 * (vocabularies.tie_section_prompt).  [from memory: t5x is not at hand, as for the beam search and the masks above]
 *   prompt   a row P[0 .. p-1] of vocabulary ids, 1 <= p <= stride, every id in [2, vocab); id 0 is padding and ends the
 *            prompt, EOS (id 1) cannot be forced.  Step t of a segment is the step at its position counter t; its input is
 *            BOS at t = 0 and otherwise the token emitted at t - 1.  The prompt is ingested as t5x does it: the decode loop
 *            steps through it and the token kernel forces the pick -- caches, position counters and every attention launch
 *            stay what they are, and the ids are those of mt3_engine_decode_forced on the same tokens, bit for bit.
 *   greedy   for t < p, ids[t] = P[t] and the next input row is Embed(P[t]) + pos[t + 1]; the row never finishes inside
 *            its prompt.  From t = p the pick is the unprompted one.
 *   beam-1   (MT3_DECODE_BEAM1) for t < p the live hypothesis takes P[t]; its live log-prob is unchanged (prompt tokens are
 *            not scored); no EOS candidate is made, so the finished score and length are untouched; the stop test is not
 *            evaluated.  From t = p the rule is the unprompted one: an EOS candidate at step t scores logp / bp(t + 1), t + 1
 *            the absolute length with the prompt included, logp the sum over the free tokens only.
 *   k-beam   for t < p all k slots of the element take P[t]; the k live log-probs stay [0, NEG_INF, ...], so step p expands
 *            beam 0 only, exactly as step 0 does without a prompt; no candidate enters the finished set, nothing forks, the
 *            slot -> row map is unchanged (the k cache rows hold the same K/V for positions < p) and the retirement test is
 *            skipped.  From t = p the rule is the unprompted one with the same absolute-length brevity penalty; at k = 1 the
 *            ids are bit-identical to beam-1.
 *   logits   d_first_logits, the per-step logits and the rows scaled in place stay the model's own.
 *   masks    a prompt token is emitted even where the segment's token mask forbids it; masks apply from t = p.  Inside the
 *            prompt the prompt also wins over the synthetic EOS schedule.
 *   bounds   max_len and num_steps mean what they meant; a decode / transcribe call whose num_steps is <= the longest
 *            prompt in use returns MT3_ERR_INVALID before any device work.
 *   segments h_seg_prompt [n_segments]: the prompt index of segment i, -1 = none; NULL: prompt 0 for every segment
 *            (n_prompts must be 1).  "Segment i" is what it is for the masks: batch row i in mt3_engine_decode, element i in
 *            mt3_engine_decode_beams, segment i of the job in mt3_engine_transcribe / _transcribe_beams -- the prompt follows
 *            the segment through compaction and refills (a refilled slot restarts at position 0 on its new segment's prompt).
 * h_prompts [n_prompts][stride] (0-padded) and h_seg_prompt are HOST arrays, copied into engine-owned device memory by
 * this call (synchronous, a setup call); h_prompts == NULL or n_prompts == 0 clears.  The prompts stay set for every later
 * mt3_engine_decode / _decode_beams / _transcribe / _transcribe_beams until cleared; prompted and unprompted steps never
 * share a captured graph, and an unprompted decode runs the kernels, graphs and bits it ran before prompts existed.
 * mt3_engine_decode_forced, mt3_engine_score and mt3_engine_score_segments IGNORE prompts, as they ignore masks.
 * MT3_STATUS_PROMPTS reports the number of prompts set.
 * MT3_ERR_INVALID, before any device work: n_prompts < 0; stride < 1; stride >= max_decode_len; NULL h_seg_prompt with
 * n_prompts > 1; n_segments < 1 with h_seg_prompt; an index outside [-1, n_prompts); an id outside {0} and [2, vocab); a
 * non-zero id after a 0; an empty prompt (a first id of 0); an engine that is not finalized; a decode in flight.
 * The decode / transcribe calls return MT3_ERR_INVALID before any device work for more rows / elements / segments than
 * n_segments when a per-segment index is set. */
int mt3_engine_set_prompts(mt3_engine* e, const int32_t* h_prompts /* [n_prompts][stride], 0-padded */, int32_t n_prompts,
                           int32_t stride, const int32_t* h_seg_prompt /* [n_segments] or NULL */, int32_t n_segments);

/* Well-formed decoding: the event grammar of MT3's output in the token kernels.  The masks and prompts above are static per
 * segment; this rule depends on what the slot has emitted.  It keeps the search off the continuations the note decoder
 * (mt3_notes_decode; run_length_encoding.decode_events with note_sequences.decode_note_event) throws away: a shift that
 * runs backwards ("event time < current time", an invalid event), a shift past the segment's end (every remaining token
 * dropped), a `tie` outside the tie section, anything but program / pitch / tie inside it.
 *   grammar  mt3_token_grammar, vocabulary ids (token id = 3 + event index): the shift of value v is shift_first + v,
 *            v < shift_count; max_steps the largest shift a free pick may take; tie_id; the program and pitch id ranges;
 *            with_ties: segments open with a tie section (MT3_SPEC_TIES).  mt3_codec_token_grammar fills it from a codec.
 *   state    one int32 per slot: bit 31 = inside the tie section, bit 30 = the previous token was a shift, bits 0 .. 29 =
 *            t, the time of the last shift in steps.  A slot starts at {with_ties, 0, 0} at position 0: at the start of a
 *            decode and at every refill (mt3g_initial).
 *   advance  applied to EVERY emitted token, free or forced by a prompt (mt3g_advance): a shift of value v sets
 *            t = prev_shift ? min(t + v, 2^29) : v and prev_shift = 1 (what decode_events does with cur_steps); tie_id
 *            clears the tie-section bit and prev_shift; any other id clears prev_shift.  A slot that has finished keeps the
 *            state its last token left.
 *   allowed  applies to a FREE pick only (mt3g_allowed).  EOS (id 1) is always allowed.  Inside the tie section an id
 *            is allowed iff it is a program id, a pitch id or tie_id.  After it tie_id is not allowed, a shift id of value v
 *            is allowed iff !prev_shift && t <= v <= max_steps, and every other id is allowed (pads, extra ids and the other
 *            event types are the mask's business).
 *   rule     a disallowed id is what a masked id is: -inf wherever the token rule reads the logit -- never picked, never
 *            one of the beam-1 top 2 or the k-beam top 2k, exactly 0 in the log-sum-exp; applied after the row scale and
 *            its write-back, so the logits handed back stay the model's own.  With a token mask set as well the allowed
 *            set is the intersection.
 *   prompts  win inside the prompt, as they win over masks; the state still advances through the forced tokens, so a
 *            tie-section prompt leaves the slot behind the section (and two forced shifts in a row add up).
 *   EOS      the synthetic EOS schedule still wins.
 *   beam-1   the state follows the live hypothesis.
 *   k-beam   the state of new slot j is advance(state[parent_j], tok_j): all k parent states are read before any is written
 *            (one block owns an element); finished candidates carry no state.
 * mt3_engine_set_token_grammar is a synchronous setup call like mt3_engine_set_token_masks, global to the engine (not per
 * segment); g == NULL clears.  The grammar stays set for every later mt3_engine_decode / _decode_beams / _transcribe /
 * _transcribe_beams until cleared; steps with a grammar never share a captured graph with steps without one, and a decode
 * without one runs the kernels, graphs and bits it ran before the grammar existed.  mt3_engine_decode_forced,
 * mt3_engine_score and mt3_engine_score_segments IGNORE the grammar, as they ignore masks.  MT3_STATUS_TOKEN_GRAMMAR
 * reports 0 / 1.
 * MT3_ERR_INVALID, before any device work: a range outside [3, vocab) or empty; overlapping ranges (tie_id counts as a
 * range of one); max_steps outside [1, shift_count - 1]; an engine that is not finalized; a decode in flight.
 * The decode / transcribe calls return MT3_ERR_INVALID before any device work for a token mask in use whose intersection
 * with the grammar leaves fewer than 2 (the beam calls: 2 * num_beams) allowed ids in the tie-section state or in the worst
 * state after it (no shift, no tie). */
typedef struct mt3_token_grammar {
  int32_t shift_first, shift_count, max_steps, tie_id, program_first, program_count, pitch_first, pitch_count, with_ties;
} mt3_token_grammar;
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MT3_RULE_FN static __host__ __device__ __inline__
#else
#define MT3_RULE_FN static inline
#endif
#define MT3_GRAMMAR_TIE_SECTION 0x80000000u
#define MT3_GRAMMAR_PREV_SHIFT 0x40000000u
#define MT3_GRAMMAR_TIME 0x3fffffffu
MT3_RULE_FN int32_t mt3g_initial(const mt3_token_grammar* g) {
  return (int32_t)(g->with_ties ? MT3_GRAMMAR_TIE_SECTION : 0u);
}
MT3_RULE_FN int32_t mt3g_advance(const mt3_token_grammar* g, int32_t state, int32_t tok) {
  const uint32_t s = (uint32_t)state, v = (uint32_t)(tok - g->shift_first);
  if (v < (uint32_t)g->shift_count) {
    uint32_t t = v;
    if (s & MT3_GRAMMAR_PREV_SHIFT) {
      t = (s & MT3_GRAMMAR_TIME) + v;
      if (t > (1u << 29)) t = 1u << 29;
    }
    return (int32_t)((s & MT3_GRAMMAR_TIE_SECTION) | MT3_GRAMMAR_PREV_SHIFT | t);
  }
  if (tok == g->tie_id) return (int32_t)(s & MT3_GRAMMAR_TIME);
  return (int32_t)(s & ~MT3_GRAMMAR_PREV_SHIFT);
}
MT3_RULE_FN int mt3g_allowed(const mt3_token_grammar* g, int32_t state, int32_t id) {
  const uint32_t s = (uint32_t)state, v = (uint32_t)(id - g->shift_first);
  if (id == 1) return 1;
  if (s & MT3_GRAMMAR_TIE_SECTION)
    return id == g->tie_id || (uint32_t)(id - g->program_first) < (uint32_t)g->program_count ||
           (uint32_t)(id - g->pitch_first) < (uint32_t)g->pitch_count;
  if (id == g->tie_id) return 0;
  if (v < (uint32_t)g->shift_count)
    return !(s & MT3_GRAMMAR_PREV_SHIFT) && v >= (s & MT3_GRAMMAR_TIME) && v <= (uint32_t)g->max_steps;
  return 1;
}
/* the three inline functions above (mt3g_*: the one statement of the rule, compiled into the token kernels and the host
 * checks alike) as exported symbols, for bindings that cannot read the header's inline functions */
int32_t mt3_token_grammar_initial(const mt3_token_grammar* g);
int32_t mt3_token_grammar_advance(const mt3_token_grammar* g, int32_t state, int32_t tok);
int32_t mt3_token_grammar_allowed(const mt3_token_grammar* g, int32_t state, int32_t id);
int mt3_engine_set_token_grammar(mt3_engine* e, const mt3_token_grammar* g /* NULL clears */);

/* Note-consistent decoding: the event grammar above plus the set of SOUNDING notes, in the token kernels.  The grammar's
 * three integers cannot see the three events note_sequences.decode_note_event raises on inside one segment: "note-off for
 * inactive pitch/program" (a velocity 0, then a pitch that is not sounding on the current program), "pitch/program is
 * already tied" (the same pair declared twice in one tie section) and "velocity cannot be zero for drum event".  This rule
 * keeps, per slot, the note decoder's own state and forbids exactly those.
 *   descriptor mt3_note_grammar: the token grammar `g` (it IS the grammar while the note grammar is set), the velocity ids
 *              (velocity value v is id velocity_first + v, v < velocity_count; value 0 is the note-off marker) and the drum
 *              ids.  mt3_codec_note_grammar fills it from a codec.  g.with_ties must be 1: without a tie section the
 *              notes begun in an earlier segment are legitimately ended here and only the host's carried-over state knows
 *              them, so a per-segment rule would forbid correct tokens (`ismir2021`-style specs are refused).
 *              g.program_count and g.pitch_count are at most 128 (MT3_NOTE_MAX_PROGRAMS / MT3_NOTE_MAX_PITCHES).
 *   state      beyond the grammar's packed int: `note`, one int32 -- bits 0 .. 7 the current program VALUE (initial 0), bit
 *              31 "the current velocity is zero" (initial clear): the note decoder's initial values, which the training
 *              targets restate before first use; and `held`, a bit set [program_count][ceil(pitch_count / 32)] of uint32,
 *              bit p % 32 of word p / 32 of row `program` set = (program, pitch value p) is sounding; all clear at position
 *              0.  128 x 4 words = 2 KiB per slot at MT3's vocabulary.
 *   advance    on EVERY emitted token, free or forced, after mt3g_advance's own rule and with the tie-section bit from
 *              BEFORE it (mt3n_advance): a program id sets the program; a velocity id sets or clears the zero bit; a pitch
 *              id p inside the tie section sets held[program][p]; after it it sets held[program][p] when the velocity is
 *              non-zero and clears it when it is zero; every other id leaves the note state alone; a finished slot keeps
 *              its state.
 *   allowed    on a FREE pick only, on top of mt3g_allowed (mt3n_allowed): inside the tie section a pitch id is allowed iff
 *              its bit is clear; after it, with velocity zero, a pitch id is allowed iff its bit is set and no drum id is
 *              allowed.  An onset of a pitch that is already held stays allowed (the note decoder ends the old note and
 *              counts nothing).
 *   rule       a disallowed id is what a masked id is (mt3_engine_set_token_grammar: -inf where the token rule reads it,
 *              after the row scale and its write-back; never in the top 2 / top 2k; exactly 0 in the log-sum-exp).  Prompts
 *              win inside the prompt and advance the state; the synthetic EOS schedule still wins; masks intersect.
 *   k-beam     the state of new slot j is advance(state[parent_j], tok_j), table included: all k parents' tables are read
 *              before any is written, and a table is copied only where parent_j != j.
 *   guarantee  every row emitted under the rule is accepted by the per-segment acceptor, for greedy, beam-1, sampled and
 *              k-beam decodes.  The rule knows ONE segment: a tie section it is free to pick may declare a note the host
 *              does not hold ("inactive pitch/program in tie section"), and a later note-off of that same note in the same
 *              segment is then invalid for the host, which never accepted the declaration.  Tied decoding below closes
 *              that: a file's segments decoded in order, each tie section prompted from the last (mt3_op_tie_prompts).
 * mt3_engine_set_note_grammar is a synchronous setup call, global to the engine; n == NULL clears.  Setting both a token
 * grammar and a note grammar on one engine is MT3_ERR_INVALID: clear one first.  Setting, changing or clearing it drops
 * the captured step graphs; steps with it never share a captured graph with other steps, and with it clear every decode
 * runs the kernels, graphs and bits it ran before.  mt3_engine_decode_forced, mt3_engine_score and
 * mt3_engine_score_segments ignore it.  MT3_STATUS_NOTE_GRAMMAR reports 0 / 1.
 * MT3_ERR_INVALID, before any device work: what mt3_engine_set_token_grammar refuses in `g`; g.with_ties == 0; a velocity
 * or drum range that is empty, outside [3, vocab) or overlaps another range; program_count or pitch_count above 128; a
 * token grammar set; an engine that is not finalized; a decode in flight.  The room check of the decode / transcribe calls
 * counts the worst state after the tie section without any pitch or drum id (velocity zero, nothing held). */
typedef struct mt3_note_grammar {
  mt3_token_grammar g;
  int32_t velocity_first, velocity_count, drum_first, drum_count;
} mt3_note_grammar;
#define MT3_NOTE_MAX_PROGRAMS 128
#define MT3_NOTE_MAX_PITCHES 128
#define MT3_NOTE_ROW_WORDS 4 /* ceil(MT3_NOTE_MAX_PITCHES / 32): the words of one program's row at most */
#define MT3_NOTE_VELOCITY_ZERO 0x80000000u
#define MT3_NOTE_PROGRAM 0xffu
MT3_RULE_FN int32_t mt3n_row_words(const mt3_note_grammar* n) { return (n->g.pitch_count + 31) >> 5; }
MT3_RULE_FN int32_t mt3n_table_words(const mt3_note_grammar* n) { return n->g.program_count * mt3n_row_words(n); }
/* the `note` int after `tok` (program and velocity ids; every other id leaves it alone) */
MT3_RULE_FN int32_t mt3n_note_advance(const mt3_note_grammar* n, int32_t note, int32_t tok) {
  const uint32_t s = (uint32_t)note, pv = (uint32_t)(tok - n->g.program_first), vv = (uint32_t)(tok - n->velocity_first);
  if (pv < (uint32_t)n->g.program_count) return (int32_t)((s & ~MT3_NOTE_PROGRAM) | pv);
  if (vv < (uint32_t)n->velocity_count) return (int32_t)(vv == 0 ? (s | MT3_NOTE_VELOCITY_ZERO) : (s & ~MT3_NOTE_VELOCITY_ZERO));
  return note;
}
/* what `tok`, emitted in grammar state `gram_before` and note state `note`, does to held[program of `note`]: 0 nothing,
 * 1 sets and 2 clears the bit of pitch value *pitch */
MT3_RULE_FN int mt3n_pitch_effect(const mt3_note_grammar* n, int32_t gram_before, int32_t note, int32_t tok, int32_t* pitch) {
  const uint32_t p = (uint32_t)(tok - n->g.pitch_first);
  if (p >= (uint32_t)n->g.pitch_count) return 0;
  *pitch = (int32_t)p;
  if ((uint32_t)gram_before & MT3_GRAMMAR_TIE_SECTION) return 1;
  return ((uint32_t)note & MT3_NOTE_VELOCITY_ZERO) ? 2 : 1;
}
/* what the note rule adds to mt3g_allowed; `row` = held[program of `note`], mt3n_row_words words */
MT3_RULE_FN int mt3n_allowed_extra(const mt3_note_grammar* n, int32_t gram, int32_t note, const uint32_t* row, int32_t id) {
  const uint32_t p = (uint32_t)(id - n->g.pitch_first);
  if (p < (uint32_t)n->g.pitch_count) {
    const int bit = (int)((row[p >> 5] >> (p & 31)) & 1u);
    if ((uint32_t)gram & MT3_GRAMMAR_TIE_SECTION) return !bit;
    return ((uint32_t)note & MT3_NOTE_VELOCITY_ZERO) ? bit : 1;
  }
  if (!((uint32_t)gram & MT3_GRAMMAR_TIE_SECTION) && ((uint32_t)note & MT3_NOTE_VELOCITY_ZERO) &&
      (uint32_t)(id - n->drum_first) < (uint32_t)n->drum_count)
    return 0;
  return 1;
}
/* `held` = the slot's whole table, mt3n_table_words words */
MT3_RULE_FN int mt3n_allowed(const mt3_note_grammar* n, int32_t gram, int32_t note, const uint32_t* held, int32_t id) {
  return mt3g_allowed(&n->g, gram, id) &&
         mt3n_allowed_extra(n, gram, note, held + ((uint32_t)note & MT3_NOTE_PROGRAM) * mt3n_row_words(n), id);
}
/* the note state after `tok`: updates `held` in place and returns the new `note`; gram_before = the grammar state `tok` was
 * emitted in (the caller advances that one with mt3g_advance) */
MT3_RULE_FN int32_t mt3n_advance(const mt3_note_grammar* n, int32_t gram_before, int32_t note, uint32_t* held, int32_t tok) {
  int32_t p = 0;
  const int eff = mt3n_pitch_effect(n, gram_before, note, tok, &p);
  if (eff) {
    uint32_t* w = held + ((uint32_t)note & MT3_NOTE_PROGRAM) * mt3n_row_words(n) + (p >> 5);
    *w = eff == 1 ? (*w | (1u << (p & 31))) : (*w & ~(1u << (p & 31)));
  }
  return mt3n_note_advance(n, note, tok);
}
/* the inline functions above as exported symbols (gram_before / gram: the packed grammar state, mt3_token_grammar_*) */
int32_t mt3_note_grammar_table_words(const mt3_note_grammar* n);
int32_t mt3_note_grammar_advance(const mt3_note_grammar* n, int32_t gram_before, int32_t note, uint32_t* held, int32_t tok);
int32_t mt3_note_grammar_allowed(const mt3_note_grammar* n, int32_t gram, int32_t note, const uint32_t* held, int32_t id);
/* MT3_OK, or MT3_ERR_INVALID with what is wrong with the descriptor for a vocabulary of `vocab` ids (what
 * mt3_engine_set_note_grammar checks; no engine and no device needed) */
int mt3_note_grammar_check(const mt3_note_grammar* n, int32_t vocab);
int mt3_engine_set_note_grammar(mt3_engine* e, const mt3_note_grammar* n /* NULL clears */);

/* Tied decoding: what a segment left sounding, as the tie section that opens the file's next segment.  The note rule above
 * knows one segment; MT3's targets open every segment with the notes active at its start, and the host note decoder
 * carries exactly that set from one segment into the next.  This is the step between: emitted id rows in, tie-section
 * prompts for mt3_engine_set_prompts out, on the device.
 *   replay   (mt3n_replay) row[0 .. len-1] is an engine id row: prompt included, 0-padded after EOS.  From gram =
 *            mt3g_initial, note = 0 and an empty table, every id is applied with mt3n_advance (with the grammar state from
 *            before it) and mt3g_advance, up to and without the first id <= 1 or the end of the row.  The table left is the
 *            row's held set.
 *   section  (mt3n_tie_section) the held pairs in ascending (program, pitch) order, a program id then a pitch id per pair;
 *            with MT3_TIE_DROP_REDUNDANT_PROGRAMS a program id only where the program differs from the pair before; then
 *            tie_id -- what vocabularies.tie_section_prompt writes (remove_redundant_programs = the flag).  Nothing held: the
 *            bare tie_id.  More than `cap` pairs held: the first `cap` in that order are kept; the count returned is all of
 *            them.  The row written has 2 * cap + 1 ids, 0 after tie_id.
 * mt3_op_tie_prompts runs both for `rows` rows in one launch, one workgroup per row: the row's end and its first tie_id by
 * block reductions, the last program and velocity id before every position by an inclusive max-scan, the last writer of each
 * (program, pitch) by an LDS table of positions, the section by a popcount scan over the table's program rows.  Rows longer
 * than the workgroup's tile of 1024 ids go through it tile by tile with the state carried over.  Its results are those of
 * mt3n_replay + mt3n_tie_section, bit for bit (mt3_note_grammar_tie_prompt: the two on the host, as an exported symbol).
 *   d_ids [rows][ids_stride] int32; d_prompts [rows][2 * cap + 1] int32; d_count [rows] int32: pairs held, before the cut
 *   to `cap`; d_held [rows][mt3n_table_words] uint32 or NULL: the held tables.  Enqueued on `stream`; no synchronisation.
 * MT3_ERR_INVALID, before any device work: a descriptor mt3_note_grammar_check refuses for every vocabulary; cap < 0 (or
 * above 2^30 - 1); rows < 1; ids_stride < 1; flags other than MT3_TIE_DROP_REDUNDANT_PROGRAMS; a null pointer other than
 * d_held. */
#define MT3_TIE_DROP_REDUNDANT_PROGRAMS 1
/* the held set of row[0 .. len-1] into held[mt3n_table_words] */
MT3_RULE_FN void mt3n_replay(const mt3_note_grammar* n, const int32_t* row, int32_t len, uint32_t* held) {
  int32_t gram = mt3g_initial(&n->g), note = 0;
  for (int32_t w = 0; w < mt3n_table_words(n); ++w) held[w] = 0;
  for (int32_t t = 0; t < len && row[t] > 1; ++t) {
    note = mt3n_advance(n, gram, note, held, row[t]);
    gram = mt3g_advance(&n->g, gram, row[t]);
  }
}
/* the tie section of `held` into out[2 * cap + 1], 0-padded; returns the pairs held */
MT3_RULE_FN int32_t mt3n_tie_section(const mt3_note_grammar* n, const uint32_t* held, int32_t cap, int32_t flags,
                                     int32_t* out) {
  int32_t count = 0, at = 0, last = -1;
  for (int32_t r = 0; r < n->g.program_count; ++r)
    for (int32_t p = 0; p < n->g.pitch_count; ++p) {
      if (!((held[r * mt3n_row_words(n) + (p >> 5)] >> (p & 31)) & 1u)) continue;
      if (count++ >= cap) continue;
      if (!(flags & MT3_TIE_DROP_REDUNDANT_PROGRAMS) || r != last) out[at++] = n->g.program_first + r;
      out[at++] = n->g.pitch_first + p;
      last = r;
    }
  out[at++] = n->g.tie_id;
  while (at < 2 * cap + 1) out[at++] = 0;
  return count;
}
/* mt3n_replay + mt3n_tie_section of one HOST row: h_prompt [2 * cap + 1], h_held [mt3n_table_words] or NULL; returns the
 * pairs held, or MT3_ERR_INVALID for what mt3_op_tie_prompts refuses */
int32_t mt3_note_grammar_tie_prompt(const mt3_note_grammar* n, const int32_t* h_row, int32_t len, int32_t cap, int32_t flags,
                                    int32_t* h_prompt, uint32_t* h_held /* or NULL */);
int mt3_op_tie_prompts(const mt3_note_grammar* n, const int32_t* d_ids, int32_t rows, int32_t ids_stride, int32_t cap,
                       int32_t flags, int32_t* d_prompts, int32_t* d_count, uint32_t* d_held /* or NULL */, void* stream);

/* Temperature sampling with top-k / top-p: t5x decoding.temperature_sample in the greedy token kernel's place.  [from
 * memory] -- t5x is not at hand, as for the beam rule; what binds is that the three statements of the rule agree: the
 * inline functions below (mt3s_*), the token kernel that compiles them, and the numpy restatement mt3_amd/sampling.py.
 *   params   mt3_sampling: temperature > 0 and finite; top_k in 0 .. 256 (0: off); 0 <= top_p < 1 (0: off); not both on
 *            (t5x refuses that too); seed, the Philox key.
 *   noise    counter based, one draw per (seed, stream, position, token id) and nothing else: a segment's sample depends
 *            neither on the slot it decodes in, nor on the batch, the row group, graph replay or in-flight refills.
 *            bits = word 0 of Philox4x32-10 with key (seed lo, seed hi) and counter (stream lo, stream hi, t, id)
 *            (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; all-zero key and counter give
 *            0x6627e8d5); u = ((bits >> 9) + 0.5) * 2^-23, exact in f32 and never 0 or 1 (23 bits, not 24: with the half
 *            added a 24-bit integer needs 25 bits, and f32 would round the largest ones up to u = 1, g = +inf);
 *            g = -logf(-logf(u)) with the accurate logf (the Gumbel trick: arg-max of z + g is a draw from softmax(z)).
 *   stream   h_seg_stream [n_segments] (host): the stream of segment i; NULL: the stream of segment i is i.  "Segment i" is
 *            what it is for masks and prompts: batch row i of mt3_engine_decode, segment i of an mt3_engine_transcribe
 *            job.  The stream follows the segment through compaction and refills.
 *   pick     at a FREE position of a live slot, after the row scale and its write-back and after the mask and the grammar
 *            have put -inf where they do: z_i = x_i / temperature in f32.  The candidates, ids with x_i > -inf, are
 *            ordered larger x first, lower id on ties (the arg-max convention; the order of z but where two different x
 *            round to one z, where x decides -- so that top_k = 1 is the greedy pick whatever the temperature).  Kept set:
 *            top_k = k: the first k candidates; top_p = p: the shortest prefix whose softmax(z) mass is >= p, at least one
 *            (the masses are summed in units of 2^-40 of the largest, exp(z_i - max z) truncated: integers, so no order of
 *            summation shows; candidates below one unit are never needed); neither: every candidate.  The token is the
 *            best of z_i + g_i over the kept set, larger first, lower id on ties.  top_k = 1 is therefore greedy, bit for
 *            bit, ties included, whatever seed and temperature.
 *   else     everything else is the greedy path's: prompts win inside the prompt, the synthetic EOS schedule wins, the
 *            grammar state advances on every emitted token, max_len, early exit, retirement and the next input row are
 *            unchanged, and the logits handed back stay the model's own.
 * mt3_engine_set_sampling is a synchronous setup call like mt3_engine_set_token_masks; s == NULL clears (h_seg_stream and
 * n_segments are then ignored).  Sampling stays set for every later mt3_engine_decode / mt3_engine_transcribe until
 * cleared; sampled steps never share a captured graph with unsampled ones (the parameters live in device memory the graphs
 * point to: another seed needs no new graph), and a decode without sampling runs the kernels, graphs and bits it ran before
 * sampling existed.  mt3_engine_decode_forced, mt3_engine_score, mt3_engine_score_segments, mt3_engine_decode_beams and
 * mt3_engine_transcribe_beams IGNORE it (the last two are t5x's other decoder); MT3_DECODE_BEAM1 with sampling set is
 * MT3_ERR_INVALID.  MT3_STATUS_SAMPLING reports 0 / 1.  A mask / grammar intersection that passes the "at least 2 allowed
 * ids" check of the greedy path needs nothing more.
 * MT3_ERR_INVALID, before any device work: a parameter outside the ranges above; a vocabulary above 2048 (the kernel keeps
 * the row in registers); n_segments < 1 with h_seg_stream; an engine that is not finalized; a decode in flight.  The
 * decode / transcribe calls return MT3_ERR_INVALID before any device work for more rows or segments than n_segments when
 * h_seg_stream was given. */
typedef struct mt3_sampling {
  float temperature;
  int32_t top_k;
  float top_p;
  uint64_t seed;                  /* (8-byte aligned: 4 bytes of padding before it, sizeof == 24) */
} mt3_sampling;
#define MT3_SAMPLING_MAX_TOP_K 256
#define MT3_SAMPLING_MAX_VOCAB 2048
MT3_RULE_FN uint32_t mt3s_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
MT3_RULE_FN uint32_t mt3s_bits(uint64_t seed, uint64_t stream, int32_t t, int32_t id) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = (uint32_t)stream, c1 = (uint32_t)(stream >> 32), c2 = (uint32_t)t, c3 = (uint32_t)id;
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = mt3s_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = mt3s_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}
MT3_RULE_FN float mt3s_uniform(uint32_t bits) { return ((float)(bits >> 9) + 0.5f) * 1.1920928955078125e-7f; }
MT3_RULE_FN float mt3s_gumbel(uint32_t bits) { return -logf(-logf(mt3s_uniform(bits))); }
/* what is wrong with the parameters (NULL: nothing): the one host-side check, for the setter and the scripted driver */
MT3_RULE_FN const char* mt3s_bad_params(const mt3_sampling* s) {
  if (!(s->temperature > 0.f) || !(s->temperature <= 3.4028234663852886e38f)) return "temperature must be positive and finite";
  if (s->top_k < 0 || s->top_k > MT3_SAMPLING_MAX_TOP_K) return "top_k must be in 0 .. 256";
  if (!(s->top_p >= 0.f) || !(s->top_p < 1.f)) return "top_p must be in [0, 1)";
  if (s->top_k > 0 && s->top_p > 0.f) return "top_k and top_p must not both be on";
  return (const char*)0;
}
/* mt3s_bits and mt3s_gumbel as exported symbols (f32, as the device computes them), for bindings that cannot read the
 * header's inline functions */
uint32_t mt3_sampling_bits(uint64_t seed, uint64_t stream, int32_t t, int32_t id);
float mt3_sampling_gumbel(uint32_t bits);
int mt3_engine_set_sampling(mt3_engine* e, const mt3_sampling* s /* NULL clears */,
                            const uint64_t* h_seg_stream /* [n_segments] or NULL */, int32_t n_segments);
/* Per-segment seeds: where this table is set, the Philox key of segment i (row i of mt3_engine_decode, segment i of
 * mt3_engine_transcribe, draw i of mt3_engine_transcribe_draws -- indexed exactly as h_seg_stream is) is h_seg_seed[i] in
 * place of mt3_sampling.seed; everything else of the rule above stays.  Two draws of one segment can therefore sit in one
 * job: same stream, different seeds.  A synchronous setup call like its neighbours; NULL clears the table, and so does
 * mt3_engine_set_sampling(e, NULL, ...).  A sampled step graph captured with the table never serves a job without it, or
 * the reverse; a sampled step without the table runs the kernels and gives the bits it gave before the table existed.
 * MT3_ERR_INVALID, before any device work: n_segments < 1 with h_seg_seed; an engine that is not finalized; a decode in
 * flight; a table while sampling is not set.  The decode / transcribe calls return MT3_ERR_INVALID before any device work
 * for more rows, segments or draws than n_segments. */
int mt3_engine_set_sampling_seeds(mt3_engine* e, const uint64_t* h_seg_seed /* [n_segments] or NULL */, int32_t n_segments);

/* Teacher-forced cached decode: Transformer.decode (mt3/network.py:303-361) on GIVEN decoder inputs, driven one
 * token per call through the same cached step (layers.py:246-314) the autoregressive loop uses -- the input of
 * step 0 is BOS, the input of step t+1 is d_forced_ids[b][t] (i.e. decoder_input_tokens = shift_right(forced),
 * seqio autoregressive_inputs as in mt3/models.py:96).  d_forced_ids [batch, L] int32.  d_step_logits (may be
 * NULL): [num_steps, batch, vocab] f32, the logits of EVERY step (the parity tests compare them with the
 * reference's teacher-forced logits at all cache depths).  d_ids [batch, L]: the arg-max of each step (no EOS
 * bookkeeping).  flags: MT3_DECODE_NO_GRAPH, MT3_DECODE_CHAINS(n); not BEAM1 / EARLY_EXIT.  Token masks
 * (mt3_engine_set_token_masks) are ignored: the arg-max is the unconstrained model's. */
int mt3_engine_decode_forced(mt3_engine* e, int32_t batch, int32_t num_steps, int32_t flags,
                             const int32_t* d_forced_ids, float* d_step_logits, int32_t* d_ids, void* stream);

/* Teacher-forced sequence scoring: t5x EncoderDecoderModel.score_batch, which ContinuousInputsEncoderDecoderModel
 * (mt3/models.py:121-152) inherits and t5x's infer reaches with mode='score'.  The rule, written down from memory
 * [from memory: t5x is not at hand, as for the beam search above]:
 *   logits         Transformer.decode(..., decode=False, enable_dropout=False) (mt3/network.py:303-361) on the encoder
 *                  output of the segment: every position at once, positions 0 .. length-1 on the sinusoidal table the
 *                  cached step uses.
 *   decoder inputs d_decoder_inputs, or (NULL) shift_right(targets) with BOS = 0 -- seqio autoregressive_inputs, what
 *                  mt3_amd.models.convert_features builds.
 *   masks          make_decoder_mask(decoder_target_tokens) (network.py:333-340): a query attends key j <= itself whose
 *                  target is > 0.  Keys with target 0 contribute nothing, wherever they sit in the row.  The query-side
 *                  mask of t5x only touches positions whose target is 0, and those are padding: their token score is 0
 *                  whatever their weight, and (masked as keys) their hidden state never reaches another position.  So
 *                  the scores equal t5x's wherever t5x's own converter sets the weights (target > 0).
 *   token scores   token_scores[b, t] = (logits[b, t, target[b, t]] - logsumexp(logits[b, t, :])) * weights[b, t]
 *                  (0 where target == 0; weights NULL: 1) -- -cross_entropy_with_logits(logits, onehot(targets),
 *                  z_loss = 0)[0] * decoder_loss_weights; t5x returns them with return_intermediates.
 *   sequence score sequence_scores[b] = sum over t of token_scores[b, t], summed in a fixed order (in double), so a
 *                  segment's score has the same bits on every run.
 * Rows: segments 0 .. batch-1 of the preceding mt3_engine_encode (batch <= its batch), as for mt3_engine_decode.
 * d_targets [batch, length] int32 (vocabulary ids, 0 = padding); d_decoder_inputs [batch, length] int32 or NULL;
 * d_weights [batch, length] f32 or NULL; d_sequence_scores [batch] f32; d_token_scores [batch, length] f32 or NULL;
 * d_logits [batch, length, vocab] f32 or NULL.  1 <= length <= max_decode_len, any value (padded internally to 64).
 * Work: the decoder as a PREFILL over chunks of segments x length rows (DESIGN.md "Scoring"): the dense layers on the
 * encoder's large-M tiles (f32: the three-plane tile, whose plane copies of the decoder matrices are built by the first
 * call; bf16: the LDS-DMA tile on the split residual rows), a causal self-attention and a cross-attention against the
 * cached cross-K/V of the encode, a log-softmax / gather reduction.  The chunk comes from a score workspace allocated by
 * the first call (32 segments at L = 1024, at most max_batch; MT3_STATUS_SCORE_CHUNKS reports the chunks of the last
 * call); the tiles do not depend on the batch or the chunk, so a segment gets the same bits in any batch wherever the
 * encoder gives it the same bits (f32: always; bf16: passes of 8 or more segments, see mt3_engine_encode).
 * Everything is enqueued on `stream` (no graph, no row groups); the call does not touch the decode state, so a decode
 * of the same encoded rows after it returns the same ids.
 * MT3_ERR_INVALID: a decode in flight (MT3_DECODE_ASYNC), e4m3 K/V caches (kv_cache_dtype MT3_FP8_E4M3: out of scope),
 * length outside 1 .. max_decode_len, batch outside 1 .. the encoded batch, null targets or sequence scores.  Ids
 * outside [0, vocab) are the caller's error (they are clamped, the scores are then meaningless).  Token masks
 * (mt3_engine_set_token_masks) are ignored: the scores are the unconstrained model's log-probabilities. */
int mt3_engine_score(mt3_engine* e, int32_t batch, int32_t length, const int32_t* d_targets,
                     const int32_t* d_decoder_inputs /* NULL: shift right */, const float* d_weights /* NULL: target > 0 */,
                     float* d_sequence_scores, float* d_token_scores, float* d_logits, void* stream);

/* Scoring of a whole job: mt3_engine_encode + mt3_engine_score over ANY number of segments, with the statistics a note
 * confidence is made of.  It sits behind the same reference call as mt3_engine_score -- t5x score_batch with
 * return_intermediates on the features mt3_amd.models.convert_features builds (mt3/models.py:121-152) -- looped over the
 * batches of a file as the notebook loops predict_batch_with_aux (NB:295-301).
 * d_inputs [n_segments, T, input_depth] f32 (log-mel); d_targets [n_segments, length] int32 (0 = padding).  The decoder
 * inputs are shift_right(targets) and the weights target > 0 (the NULL defaults of mt3_engine_score).
 * d_sequence_scores [n_segments] f32; d_token_scores [n_segments, length] f32 or NULL; d_top1_ids [n_segments, length]
 * int32 or NULL: the arg-max of the position's logits, the LOWEST id on equal logits (lax.top_k's tie rule, as the beam
 * kernels rank); d_top1_scores [n_segments, length] f32 or NULL: its log-probability logits[top1] - logsumexp(logits),
 * so token score - top1 score is the margin of the target to the model's best token (0 when they are the same).  Where
 * the target is 0 all three are 0.
 * Work: chunks of at most max_batch segments; per chunk the encoder pass and cross-K/V of mt3_engine_encode into the
 * caches, then the prefill of mt3_engine_score against them.  Without a top-1 output the reduction is the one of
 * mt3_engine_score; with one, a kernel that finds the arg-max in the pass that finds the maximum (same reduction order,
 * same token scores).  Everything is enqueued on `stream` (no graph, no row groups, no worker threads); the call does not
 * block (the FIRST scoring call of an f32 engine waits once for the plane copies of its decoder matrices).
 * Contract: segment i's sequence score and token scores are BIT-IDENTICAL to mt3_engine_encode of its chunk (segments
 * [c * max_batch, min(n_segments, (c + 1) * max_batch))) + mt3_engine_score, under the encoder-reproducibility condition
 * mt3_engine_encode documents (f32: always; bf16: passes of 8 or more segments).  In bf16 a last chunk of n < 8 segments
 * is encoded in a pass of min(8, max_batch) rows behind the segments in front of it, exactly as mt3_engine_transcribe
 * pads its staging passes, so a segment's scores do not depend on where the job ends.
 * State: the call leaves the engine "encoded" with its last pass, as a sequence of mt3_engine_encode calls would: the
 * last chunk's segments in cache rows 0 .. n-1 (bf16, padded last chunk: the pass's 8 rows, the chunk's segments last).
 * It does not touch the decode state.  MT3_STATUS_SCORE_CHUNKS reports the prefill chunks of the whole call.
 * MT3_ERR_INVALID, before any device work: a NULL engine, inputs, targets or sequence scores; n_segments < 1; length
 * outside 1 .. max_decode_len; an engine that is not finalized; a decode in flight (MT3_DECODE_ASYNC); e4m3 K/V caches
 * (kv_cache_dtype MT3_FP8_E4M3: out of scope, as for mt3_engine_score).  Ids outside [0, vocab) are clamped.  Token
 * masks (mt3_engine_set_token_masks) are ignored, as by mt3_engine_score. */
int mt3_engine_score_segments(mt3_engine* e, const float* d_inputs /* [n_segments, T, input_depth] log-mel */,
                              int32_t n_segments, int32_t length, const int32_t* d_targets /* [n_segments, length] */,
                              float* d_sequence_scores /* [n_segments] */, float* d_token_scores /* [n, length] or NULL */,
                              int32_t* d_top1_ids /* [n, length] or NULL */, float* d_top1_scores /* [n, length] or NULL */,
                              void* stream);

/* Scoring of CANDIDATES: `per` target rows against every segment, the segment encoded ONCE -- the table of an offset
 * search (the same notes under `per` time shifts) without `per` encoder passes per segment.
 * d_inputs [n_segments, T, input_depth] f32 (log-mel); d_targets [n_segments * per, length] int32: row s * per + j is
 * candidate j of segment s.  The outputs are those of mt3_engine_score_segments, one row per target row:
 * d_sequence_scores [n_segments * per]; d_token_scores, d_top1_ids, d_top1_scores [n_segments * per, length] or NULL.
 * Work: the encoder chunks of mt3_engine_score_segments over the n_segments segments (at most max_batch each; in bf16 a
 * short last chunk padded to a pass of min(8, max_batch) rows, exactly as there); per chunk of n segments the prefill
 * of mt3_engine_score over its n * per rows, in pieces that fit the score workspace.  Row i of the chunk reads the
 * cross-K/V cache at row i / per (a divisor in the cross-attention launch; the kernel is the one
 * mt3_op_score_attention runs); embedding, self-attention, dense tiles and reductions are launched as they are there.
 * Contract: the outputs are BIT-IDENTICAL to mt3_engine_score_segments on the job with every segment repeated `per`
 * times (row s * per + j of its inputs = segment s) wherever that function gives a segment the same bits in any batch:
 * f32 always; bf16 when every encoder pass of BOTH calls holds 8 or more segments (see mt3_engine_encode) -- the tiles
 * of the prefill do not depend on the batch or the piece, so only the encoder can tell the two jobs apart.
 * State: as mt3_engine_score_segments -- the engine is left encoded with the last pass of the n_segments segments; the
 * decode state is not touched.  MT3_STATUS_SCORE_CHUNKS reports the prefill pieces of the whole call and
 * MT3_STATUS_SCORE_ENCODER_PASSES its encoder passes (ceil(n_segments / max_batch), whatever `per` is).
 * MT3_ERR_INVALID, before any device work: everything mt3_engine_score_segments refuses; per < 1; n_segments * per
 * above INT32_MAX. */
int mt3_engine_score_candidates(mt3_engine* e, const float* d_inputs /* [n_segments, T, input_depth] log-mel */,
                                int32_t n_segments, int32_t per, int32_t length,
                                const int32_t* d_targets /* [n_segments * per, length] */,
                                float* d_sequence_scores /* [n_segments * per] */, float* d_token_scores /* or NULL */,
                                int32_t* d_top1_ids /* or NULL */, float* d_top1_scores /* or NULL */, void* stream);

/* Engine facts a caller cannot see from results alone (a negative return is an mt3_status).
 * GRAPH_FALLBACKS: decode calls so far whose step graph could not be captured/instantiated and that therefore
 * ran as direct launches (same ids, slower) -- the fallback is counted, never silent;
 * LAST_DECODE_USED_GRAPH: 1/0 for the most recent decode; RESIDUAL_SPLIT: 1 if the bf16 decode loop carries the
 * residual rows as f32 + bf16 copy + partial sums of squares. */
enum { MT3_STATUS_GRAPH_FALLBACKS = 0, MT3_STATUS_LAST_DECODE_USED_GRAPH = 1, MT3_STATUS_RESIDUAL_SPLIT = 2,
       MT3_STATUS_KV_FP8 = 3, MT3_STATUS_Q_FOLD = 4 /* cross q-projection folded into the neighbouring launches */,
       MT3_STATUS_DENSE_FP8 = 5 /* encoder dense layers on the MXFP8 path */,
       MT3_STATUS_QKV_FOLD = 6 /* the decoder layers' q/k/v projections folded into the preceding launches */,
       MT3_STATUS_LAST_DECODE_GROUPS = 7 /* row groups of the most recent decode (2 or 4: the row-group schedule); 1: on the caller's stream */,
       MT3_STATUS_PARTITION_FALLBACKS = 8 /* decodes that wanted the row-group schedule but could not set it up */,
       MT3_STATUS_LAST_DECODE_COMPACTIONS = 9 /* live-row compactions of the most recent decode (all row groups) */,
       MT3_STATUS_LAST_DECODE_FORKS = 10 /* cache-row copies of the most recent mt3_engine_decode_beams / mt3_engine_transcribe_beams */,
       MT3_STATUS_SCORE_CHUNKS = 11 /* chunks of the most recent mt3_engine_score / mt3_engine_score_segments (all its encoder chunks) */,
       MT3_STATUS_TOKEN_MASKS = 12 /* masks set by mt3_engine_set_token_masks (0: none) */,
       MT3_STATUS_PROMPTS = 13 /* prompts set by mt3_engine_set_prompts (0: none) */,
       MT3_STATUS_TOKEN_GRAMMAR = 14 /* 1: a grammar is set by mt3_engine_set_token_grammar (0: none) */,
       MT3_STATUS_SAMPLING = 15 /* 1: sampling is set by mt3_engine_set_sampling (0: none) */,
       MT3_STATUS_NOTE_GRAMMAR = 16 /* 1: a note grammar is set by mt3_engine_set_note_grammar (0: none) */,
       MT3_STATUS_SCORE_ENCODER_PASSES = 17 /* encoder passes of the most recent mt3_engine_score_segments / mt3_engine_score_candidates */ };
int mt3_engine_status(const mt3_engine* e, int32_t what);

/* GenericTokenVocabulary._decode_tf (mt3/vocabularies.py:241-271): -1 from the
 * first EOS(1) to the end of the row, id-3 for 3 <= id < 3+num_regular, else -2. */
int mt3_ids_to_tokens(const int32_t* d_ids, int32_t batch, int32_t length, int32_t num_regular,
                      int32_t* d_tokens, void* stream);

/* ------------------------------------------------ kernel-level entry points
 * The same kernels the engine launches, exposed one at a time so that parity
 * tests can check each against the oracle.  dtype: mt3_dtype of A/W/out. */
enum { MT3_EPI_STORE = 0, MT3_EPI_RESID = 1, MT3_EPI_GEGLU = 2, MT3_EPI_POS = 3, MT3_EPI_F32 = 4, MT3_EPI_HEADS = 5 };
/* out = epilogue( [rms(A)] * A[M,K] @ Wt[N,K]^T );  a_is_f32: A is f32 (converted on load);
 * norm: multiply rows by rsqrt(mean(A^2)+1e-6) (requires a_is_f32).  aux: pos table (EPI_POS, f32 [T,N]);
 * seq_len: T for EPI_POS / EPI_HEADS; heads for EPI_HEADS = N/(2*64).  small: use the decode-sized tile. */
int mt3_op_gemm(int32_t dtype, const void* d_A, int32_t a_is_f32, int32_t norm, const void* d_Wt,
                void* d_out, int32_t M, int32_t N, int32_t K, int32_t epilogue, const float* d_aux,
                int32_t seq_len, int32_t small, void* stream);
/* The same with the split residual stream: norm = 2 takes A as the COMPUTE-TYPE copy of the
 * rows plus d_a_ss [M][K/16], the exact f32 sums of squares of each 16-column group (what the producer of the rows
 * left), instead of accumulating statistics from an f32 A; with EPI_RESID, d_out_ct / d_out_ss (both or neither)
 * receive the compute-type copy [M][N] and the partial sums [M][N/16] of the updated rows.  small = 0 with bf16
 * operands in memory selects the LDS-DMA staged 128x128x64 tile. */
int mt3_op_gemm_ex(int32_t dtype, const void* d_A, int32_t a_is_f32, int32_t norm, const void* d_Wt,
                   void* d_out, int32_t M, int32_t N, int32_t K, int32_t epilogue, const float* d_aux,
                   int32_t seq_len, int32_t small, const float* d_a_ss, void* d_out_ct, float* d_out_ss,
                   void* stream);
/* The two decode-sized launches that carry a SECOND product in extra column tiles (the qkv-fold):
 * columns [0, n_split) behave as mt3_op_gemm_ex with small = 1, columns [n_split, n_split + n_side) are the plain f32
 * product of the same rows with the weight rows that follow -- no row scale, no activation -- in d_side [M][n_side].
 *   MT3_EPI_GEGLU: norm 2 (d_A compute type + d_a_ss), d_out [M][n_split / 2]; d_side is STORED.  d_Wt holds
 *                  n_split + 64 * ceil(n_side / 64) rows (whole tiles; what the padding rows hold is never stored).
 *   MT3_EPI_RESID: no norm, f32 d_out [M][n_split] += product (d_out_ct / d_out_ss as for mt3_op_gemm_ex); d_side is
 *                  ACCUMULATED into: side = side + product.  n_side a multiple of 32.
 * n_split a multiple of 64.  concurrent != 0 with f32 operands and M >= 256 selects the 64 x 32 x 128 tile of large
 * row groups that run side by side (same bits). */
int mt3_op_gemm_side(int32_t dtype, const void* d_A, const void* d_Wt, void* d_out, int32_t M, int32_t n_split,
                     int32_t n_side, int32_t K, int32_t epilogue, const float* d_a_ss, void* d_out_ct, float* d_out_ss,
                     float* d_side, int32_t concurrent, void* stream);
/* The decode-sized tiles in EVERY form the decode loop launches them in (tests/test_gpu_decode_gemm_forms.py): a view of
 * all the launch's fields, optional pointers NULL.  Test driver: it fills the launch description and launches the
 * decode-sized tile (small = 1) on `stream`, nothing else (nothing allocated or waited for).
 *   A [M][lda] (lda 0: K) f32 (a_is_f32) or compute type; Wt [N][K] compute type; norm 0 / 1 / 2 and a_ss as for
 *   mt3_op_gemm_ex; out rows are ldo elements apart (GEGLU: >= N / 2, or n_split / 2 with out2; else >= N, or n_split).
 *   epilogue: one of MT3_EPI_*.  out_ct / out_ss: MT3_EPI_RESID, as for mt3_op_gemm_ex (out_ct [M][ldo], out_ss
 *   [M][width / 16]).
 *   out2 != NULL (MT3_EPI_STORE, MT3_EPI_RESID, MT3_EPI_GEGLU only) makes the weight rows [n_split, N) a SECOND product
 *   of the same rows, as for mt3_op_gemm_side: plain f32, no row scale, no activation, row r at out2 + r * ld2 (ld2 0:
 *   N - n_split).  STORE and GEGLU store it, RESID adds it to what is there; columns at and past the side width of a
 *   wider row (ld2 > N - n_split: a region inside a wider buffer) are neither read nor written.  GEGLU: N - n_split is
 *   padded to whole 64-column tiles and only the first ld2 columns are written.  n_split a multiple of 64.
 *   concurrent != 0 with f32 operands, M >= 256 and MT3_EPI_RESID / MT3_EPI_GEGLU selects the 64 x 32 x 128 tile.
 * MT3_ERR_INVALID before anything touches a device: v NULL, norm outside 0 .. 2, an epilogue outside MT3_EPI_*, out2
 * with an epilogue that has no second product, lda < K, ldo below the primary width, ld2 < 0 or (STORE / RESID) a
 * non-zero ld2 below N - n_split, out_ct / out_ss not as mt3_op_gemm_ex takes them, and whatever the launcher refuses
 * for the engine too (NULL operands, shapes that are no multiple of the tile, n_split, a_ss without norm 2, ...). */
typedef struct mt3_gemm_view {
  const void* A;
  const void* Wt;
  void* out;
  int32_t M, N, K;
  int32_t lda, ldo;
  int32_t a_is_f32, norm, epilogue;
  const float* a_ss;
  void* out_ct;
  float* out_ss;
  float* out2;
  int32_t n_split, ld2;
  int32_t concurrent, reserved;
} mt3_gemm_view;
int mt3_op_gemm_decode(int32_t dtype, const mt3_gemm_view* v, void* stream);
/* x f32 [rows][dim] -> compute-type copy [rows][dim] + per-16-column sums of squares [rows][dim/16] */
int mt3_op_residual_split(int32_t dtype, const float* d_x, void* d_x_ct, float* d_x_ss, int32_t rows, int32_t dim,
                          void* stream);
/* encoder self-attention over qkv [B, T, 3, H, 64] -> out [B, T, H*64]; unscaled logits, softmax f32 */
int mt3_op_encoder_attention(int32_t dtype, const void* d_qkv, void* d_out, int32_t B, int32_t T, int32_t H,
                             void* stream);
/* single-query attention: q [B, H*64] (row stride q_stride elements) against cache K/V [B, H, cap, 64],
 * attending positions 0..n_keys-1; if d_new_kv != NULL its [B, 2, H, 64]-strided K/V rows (row stride
 * kv_stride, K at +0 and V at +H*64) are first appended at position n_keys-1.  With d_step != NULL the key
 * count is read PER ROW from device memory: n_keys = d_step[b] + 1.  The kernel requests its first group of
 * keys before it knows the row's length; what lies past the row's length is discarded BY POSITION (selected away,
 * never multiplied by a zero weight), so cache rows beyond n_keys may hold anything, NaN / Inf patterns included
 * (they only have to be addressable up to `cap`). */
int mt3_op_decode_attention(int32_t dtype, const void* d_q, int32_t q_stride, void* d_kcache, void* d_vcache,
                            int32_t cap, const void* d_new_k, const void* d_new_v, int32_t kv_stride,
                            const int32_t* d_step, int32_t n_keys, void* d_out, int32_t B, int32_t H, void* stream);
/* The same over an fp8 cache (kv_cache_dtype MT3_FP8_E4M3): d_kcache / d_vcache hold OCP e4m3 bytes [B, H, cap, 64],
 * d_kv_scale [B, H, cap] pairs of f32 {k_scale, v_scale} (row value = byte value * scale); q, the new rows and
 * out are bf16.  An appended row is quantised by the kernel (power-of-two scale from the row's amax per head). */
int mt3_op_decode_attention_fp8(const void* d_q, int32_t q_stride, void* d_kcache, void* d_vcache, void* d_kv_scale,
                                int32_t cap, const void* d_new_k, const void* d_new_v, int32_t kv_stride,
                                const int32_t* d_step, int32_t n_keys, void* d_out, int32_t B, int32_t H,
                                void* stream);
/* The same kernels in EVERY form the decode loop launches them in (tests/test_gpu_decode_attention_forms.py): a view
 * of all the launch's fields, pointers those of the first slot, optional ones NULL.  Test driver: it fills the launch
 * description and launches on `stream`, nothing else (nothing allocated or waited for).
 *   plain query:   q [B][q_stride] compute type (bf16 / f32 by `dtype`), as mt3_op_decode_attention.
 *   folded query:  q NULL, q_f32 [B][q_stride] UNNORMALISED f32 products, q_ss [B][q_ss_n] the partial sums of squares of
 *                  the residual row they were projected from (q_ss_n = emb / 16: 4 .. 64, a multiple of 4).  The kernel
 *                  forms rs = rsqrt(sum(q_ss[b]) / (16 q_ss_n) + 1e-6) and uses round_ct(q_f32 * rs); with new_k / new_v
 *                  those are f32 rows [B][kv_stride] too and round_ct(new * rs) is what is appended (e4m3 caches:
 *                  quantised after the bf16 rounding).  q_stride (and kv_stride) % 4 == 0.
 *   kv_scale:      non-NULL = e4m3 caches with their scale pairs [B][H][cap], as mt3_op_decode_attention_fp8 (bf16 only).
 *   row retirement: done [B] per slot -- a slot with done != 0 is left alone: its out row, its cache row and its step
 *                  entry are neither read nor written; cache_row [B] (needs done) maps slot b to the row of kcache /
 *                  vcache / kv_scale it reads and appends in (NULL: row b).
 * MT3_ERR_INVALID before anything touches a device: v NULL, q and q_f32 both NULL or both set, NULL caches / out, B, H
 * or cap <= 0, n_keys outside 1 .. cap without step, new_k without new_v, q_f32 without q_ss or with q_ss_n outside
 * 4 .. 64 / not a multiple of 4 or strides that are no multiple of 4, cache_row without done, kv_scale with f32. */
typedef struct mt3_dec_attn_view {
  const void* q;
  int32_t q_stride, cap;
  void* kcache;
  void* vcache;
  const void* new_k;
  const void* new_v;
  int32_t kv_stride, n_keys;
  const int32_t* step;
  void* out;
  int32_t B, H;
  void* kv_scale;
  const float* q_f32;
  const float* q_ss;
  int32_t q_ss_n, reserved;
  const int32_t* done;
  const int32_t* cache_row;
} mt3_dec_attn_view;
int mt3_op_decode_attention_ex(int32_t dtype, const mt3_dec_attn_view* v, void* stream);
/* d_src bf16 [2][rows][64] (K rows, then V rows) -> d_dst e4m3 [2][rows][64] + d_scales [rows] f32 pairs */
int mt3_op_kv_quantize_fp8(const void* d_src, void* d_dst, void* d_scales, int32_t rows, void* stream);

/* The token-rule kernels of the decode loop on SCRIPTED logits: the launches the engine ends every decode step with
 * (greedy / beam-1 pick, k-beam step, fork copies, finalisation), on logits the caller wrote instead of a model's, with
 * state the call allocates and frees.  Test drivers: they synchronise `stream` and return when the result is complete.
 * Common: d_ss != NULL makes the logits of step t UNNORMALISED rows with d_ss [num_steps][rows][n_ss] partial sums
 * (1 <= n_ss <= 64): the kernels scale row r by rsqrt(sum(d_ss[t][r]) / dim + 1e-6) before anything else, as they do for
 * the engine's folded logits projection.  max_len > 0 closes a row / element once its position counter reaches max_len
 * (0: off), as the in-flight batching jobs do.  NULL pointers (other than the optional ones), k outside 1 .. 8 and, for the
 * beam step, vocab outside [2k, 2048] return MT3_ERR_INVALID before anything touches the device.
 *
 * mt3_op_beam_search_scripted: the search of mt3_engine_decode_beams over `elems` elements of k beams; d_logits
 * [num_steps][elems * k][vocab] f32, row b*k + j of step t = what live beam j of element b sees at step t.  The slot ->
 * cache-row map starts as the identity; the call stops after the step at which every element is retired or closed
 * (*h_steps_run).  d_ids [elems][num_steps], d_all_ids [elems][k][num_steps], d_scores [elems][k] as
 * mt3_engine_decode_beams returns them (an element that max_len closed with nothing finished returns its live beams of
 * max_len tokens).  h_trace (host) [num_steps][4][elems * k] int32: after step t the slot -> row map, the fork source of
 * each slot (-1: none), the done flags and the next input tokens; h_live (host) [num_steps][elems * k]: the live
 * log-probs (rows of steps that did not run are not written).  *h_forks: the fork count
 * (MT3_STATUS_LAST_DECODE_FORKS).  d_table [vocab][dim_e] / d_pos [num_steps + 1][dim_e] / d_y_next [elems * k][dim_e]
 * f32 (all or none, dim_e % 16 == 0): each step also writes the next input row of every slot of an open element,
 * table[token] + pos[t + 1] (the single-stream f32 form). */
int mt3_op_beam_search_scripted(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t elems,
                                int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len, const float* d_table,
                                const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids, float* d_scores,
                                float* d_y_next, int32_t* h_trace, float* h_live, int32_t* h_forks,
                                int32_t* h_steps_run, void* stream);
/* num_steps steps of the token kernel of mt3_engine_decode on d_logits [num_steps][rows][vocab] (vocab >= 2, any size;
 * with d_ss the scaled logits are written back in place): mode 0 = greedy (first arg-max, 0 after EOS), mode 1 =
 * MT3_DECODE_BEAM1 including its finalisation.  No teacher forcing, no EOS schedule.  d_ids [rows][num_steps];
 * h_done (host) [num_steps][rows]: the done flags after each step. */
int mt3_op_token_steps_scripted(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows,
                                int32_t vocab, int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids,
                                int32_t* h_done, void* stream);
/* The two drivers above with token masks (mt3_engine_set_token_masks states the rule): d_masks [n_masks][ceil(vocab / 32)]
 * uint32 and d_row_mask, the mask index (-1: unconstrained) per ROW for the token kernel and per ELEMENT for the beam
 * kernel (NULL: mask 0), both DEVICE arrays.  They are read back and checked first: MT3_ERR_INVALID for n_masks outside
 * 1 .. 4096, an index outside [-1, n_masks), a mask without EOS, with bits past vocab, or with fewer than 2 (token
 * kernel) / 2k (beam kernel) allowed tokens.  The logits in d_logits stay unmasked. */
int mt3_op_beam_search_masked(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t elems,
                              int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len, const float* d_table,
                              const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids, float* d_scores,
                              float* d_y_next, int32_t* h_trace, float* h_live, int32_t* h_forks, int32_t* h_steps_run,
                              void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask);
int mt3_op_token_steps_masked(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows, int32_t vocab,
                              int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids, int32_t* h_done,
                              void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask);
/* The two masked drivers with prompts (mt3_engine_set_prompts states the rule): d_prompts [.][stride] int32, 0-padded, and
 * d_row_prompt, the prompt index (-1: none) per ROW for the token kernel and per ELEMENT for the beam kernel (NULL: prompt
 * 0), both DEVICE arrays; the prompts are rows 0 .. the largest index.  They are read back and checked first:
 * MT3_ERR_INVALID for a stride outside 1 .. 4096, an index outside [-1, 4096) or a prompt mt3_engine_set_prompts would
 * refuse.  d_masks == NULL: no masks (n_masks and d_row_mask are then ignored); d_prompts == NULL: no prompts. */
int mt3_op_beam_search_prompted(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t elems,
                                int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len, const float* d_table,
                                const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids, float* d_scores,
                                float* d_y_next, int32_t* h_trace, float* h_live, int32_t* h_forks, int32_t* h_steps_run,
                                void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                                const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt);
int mt3_op_token_steps_prompted(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows, int32_t vocab,
                                int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids, int32_t* h_done,
                                void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                                const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt);
/* The two prompted drivers with the event grammar (mt3_engine_set_token_grammar states the rule): h_grammar is a HOST
 * descriptor, checked first as mt3_engine_set_token_grammar checks it (MT3_ERR_INVALID; and for a mask whose intersection
 * with the grammar leaves fewer than 2 / 2k ids in the tie-section state or the worst state after it); NULL: no grammar --
 * the call is then the _prompted driver, bit for bit.  h_state (HOST, [num_steps][rows] for the token kernel,
 * [num_steps][elems * k] for the beam kernel, may be NULL) receives the packed grammar state of every slot after each
 * step (rows of steps that did not run stay untouched). */
int mt3_op_beam_search_grammar(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t elems,
                               int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len, const float* d_table,
                               const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids, float* d_scores,
                               float* d_y_next, int32_t* h_trace, float* h_live, int32_t* h_forks, int32_t* h_steps_run,
                               void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                               const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt,
                               const mt3_token_grammar* h_grammar, int32_t* h_state);
int mt3_op_token_steps_grammar(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows, int32_t vocab,
                               int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids, int32_t* h_done,
                               void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                               const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt,
                               const mt3_token_grammar* h_grammar, int32_t* h_state);
/* The grammar token driver with temperature sampling (mt3_engine_set_sampling states the rule): h_sampling is a HOST
 * descriptor, checked first as mt3_engine_set_sampling checks it (MT3_ERR_INVALID; also for vocab > 2048 and for mode 1,
 * beam-1, which does not sample); NULL: no sampling -- the call is then the _grammar driver, bit for bit.  h_row_stream
 * (HOST, [rows], may be NULL: the stream of row i is i) gives the noise stream of each row. */
int mt3_op_token_steps_sampled(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows, int32_t vocab,
                               int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids, int32_t* h_done,
                               void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                               const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt,
                               const mt3_token_grammar* h_grammar, int32_t* h_state, const mt3_sampling* h_sampling,
                               const uint64_t* h_row_stream);
/* The grammar drivers with the note rule (mt3_engine_set_note_grammar states it): h_notes is a HOST descriptor, checked
 * first as mt3_engine_set_note_grammar checks it and, with a mask, for the room the rule leaves (MT3_ERR_INVALID); its `g`
 * member is the grammar.  NULL: the calls are mt3_op_token_steps_sampled / mt3_op_beam_search_grammar with a NULL
 * grammar, bit for bit.  h_state as there; h_note (HOST, [num_steps][slots], may be NULL) receives the `note` int of every
 * slot after each step and h_held (HOST, [num_steps][slots][program_count * ceil(pitch_count / 32)], may be NULL) the whole
 * table of every slot after each step (slots = rows, or elems * k). */
int mt3_op_token_steps_notes(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows, int32_t vocab,
                             int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids, int32_t* h_done,
                             void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                             const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt,
                             const mt3_note_grammar* h_notes, int32_t* h_state, const mt3_sampling* h_sampling,
                             const uint64_t* h_row_stream, int32_t* h_note, uint32_t* h_held);
/* mt3_op_token_steps_notes with per-row Philox keys (mt3_engine_set_sampling_seeds states the rule): h_row_seed (HOST,
 * [rows], may be NULL) gives the key of each row in place of h_sampling->seed; it is read only with h_sampling.  With
 * NULL the call is the _notes driver, bit for bit. */
int mt3_op_token_steps_seeded(float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t rows, int32_t vocab,
                              int32_t num_steps, int32_t mode, int32_t max_len, int32_t* d_ids, int32_t* h_done,
                              void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                              const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt,
                              const mt3_note_grammar* h_notes, int32_t* h_state, const mt3_sampling* h_sampling,
                              const uint64_t* h_row_stream, int32_t* h_note, uint32_t* h_held,
                              const uint64_t* h_row_seed);
int mt3_op_beam_search_notes(const float* d_logits, const float* d_ss, int32_t n_ss, int32_t dim, int32_t elems,
                             int32_t k, int32_t vocab, int32_t num_steps, int32_t max_len, const float* d_table,
                             const float* d_pos, int32_t dim_e, int32_t* d_ids, int32_t* d_all_ids, float* d_scores,
                             float* d_y_next, int32_t* h_trace, float* h_live, int32_t* h_forks, int32_t* h_steps_run,
                             void* stream, const uint32_t* d_masks, int32_t n_masks, const int32_t* d_row_mask,
                             const int32_t* d_prompts, int32_t stride, const int32_t* d_row_prompt,
                             const mt3_note_grammar* h_notes, int32_t* h_state, int32_t* h_note, uint32_t* h_held);
/* The fork copies of one k-beam step on caller-owned caches: for every slot with d_fork_src[slot] >= 0 and
 * d_done[slot] == 0, positions [0, d_step[slot]) of row d_fork_src[slot] are copied into row d_slot_row[slot] of every
 * layer's K and V cache [rows][H][cap][64] of kv_esize-byte elements (1, 2 or 4) and, where given, of its scale pairs
 * [rows][H][cap] (h_scale == NULL or h_scale[l] == NULL: none).  h_k / h_v / h_scale: HOST arrays of n_layers (<= 16)
 * device pointers. */
int mt3_op_beam_reorder(int32_t n_layers, int32_t H, int32_t cap, int32_t kv_esize, int32_t slots, void* const* h_k,
                        void* const* h_v, void* const* h_scale, const int32_t* d_fork_src, const int32_t* d_slot_row,
                        const int32_t* d_step, const int32_t* d_done, void* stream);

/* The slot-moving launches of the decode loop on SCRIPTED slot state: the input-row writer (every decode step, refill),
 * the compaction of row retirement (MT3_DECODE_EARLY_EXIT) and the refills of in-flight batching
 * (mt3_engine_transcribe, mt3_engine_transcribe_beams), each alone on device memory the CALLER owns and has filled
 * (tests/test_gpu_slot_moves.py).  Test drivers: scratch the caller has no business with (the plan / permutation, the
 * compaction's scratch rows) is allocated, 0xFF-filled and freed by the call, which synchronises `stream` before it
 * returns.  Every argument error -- what the launch itself refuses, a missing pointer, a size out of range -- returns
 * MT3_ERR_INVALID before anything touches a device.  The views below mirror the engine's own descriptions; pointers
 * are those of the first slot of the region the call works on, optional ones may be NULL.
 *
 * mt3_input_row_view: a decoder input row table[tok] + pos[min(t, max_pos - 1)] and the forms it is written in: y f32
 * [slots][dim]; y_ct its bf16 copy (round to nearest even); y_ss [slots][dim / 16] the sums of squares of each 16-column
 * group (y_ct needs y_ss, both need dim % 16 == 0; y alone dim % 4 == 0); q_out [slots][q_n] = ew[tok] + pw[min(t,
 * max_pos - 1)] (q_n % 4 == 0; needs ew, pw and y). */
typedef struct mt3_input_row_view {
  const float* table;
  const float* pos;
  int32_t max_pos, dim;
  float* y;
  void* y_ct;
  float* y_ss;
  const float* ew;
  const float* pw;
  float* q_out;
  int32_t q_n, reserved;
} mt3_input_row_view;
/* per-slot int32 state: done flag, slot -> row of the caches and id rows, segment the slot decodes (-1: none), position
 * counter, next input token; n_done: the group's counter of finished slots (one int32) */
typedef struct mt3_slot_state_view {
  int32_t* done;
  int32_t* slot_row;
  int32_t* slot_seg;
  int32_t* step;
  int32_t* cur_tok;
  int32_t* n_done;
} mt3_slot_state_view;
/* staged cross-attention K/V of a run of segments and the caches they go to.  src / dst / src_sc / dst_sc: HOST arrays
 * of n_layers (<= 16) device pointers: per layer, staging chunk [2][src_batch][row_bytes] (the run starts at entry
 * src_entry0) -> cache [2][dst_batch][row_bytes], and scale rows [src_batch][sc_bytes] -> [dst_batch][sc_bytes] where
 * src_sc != NULL and src_sc[l] != NULL.  row_bytes and sc_bytes are multiples of 16. */
typedef struct mt3_staged_cross_view {
  int32_t n_layers, src_batch, src_entry0, dst_batch;
  uint64_t row_bytes, sc_bytes;
  const void* const* src;
  void* const* dst;
  const void* const* src_sc;
  void* const* dst_sc;
} mt3_staged_cross_view;
/* state of the k-beam search over `elems` elements of k slots (slot = element * k + beam): live log-probs, the finished
 * entries best first (score, step of the EOS or -1, beam whose prefix it ends), the history [L][hist_stride] of parent
 * beam and token per step and slot, the pending fork sources */
typedef struct mt3_beam_k_view {
  int32_t k, elems, vocab, hist_stride;
  float* live;
  float* fin_score;
  int32_t* fin_step;
  int32_t* fin_beam;
  int32_t* hist_par;
  int32_t* hist_tok;
  int32_t* fork_src;
} mt3_beam_k_view;
/* in->y[r] (and the other forms `in` holds) = the input row of token d_tok[r] at position d_t[r], r < rows */
int mt3_op_embed_rows(const mt3_input_row_view* in, const int32_t* d_tok, const int32_t* d_t, int32_t rows,
                      void* stream);
/* Row retirement over slots [0, rows): the state of the i-th live slot (done == 0, ascending) moves to slot i -- in->y,
 * y_ct, y_ss, q_out (tables unused; dim % 16 == 0; y_ct needs y_ss, as everywhere), slot_row, step, cur_tok, slot_seg (optional) and, with d_beam_f, the
 * beam-1 state d_beam_f[slot], d_beam_f[beam_rows + slot] (beam_rows >= rows) and d_beam_len[slot]; done becomes 0 for
 * the n live slots and 1 for slots [n, rows), whose slot_seg becomes -1 and whose other state keeps its bytes.
 * h_perm (host, optional) [rows + 1]: the permutation, h_perm[i < n] = source of slot i, h_perm[rows] = n (entries
 * [n, rows) are not written: 0xFF bytes). */
int mt3_op_slot_compact(const mt3_slot_state_view* st, const mt3_input_row_view* in, float* d_beam_f, int32_t beam_rows,
                        int32_t* d_beam_len, int32_t rows, int32_t* h_perm, void* stream);
/* The refill of mt3_engine_transcribe over slots [0, rows): every finished slot with slot_seg >= 0 hands id row
 * d_ids[slot_row] ([..][ids_stride]) to d_out_ids[slot_seg] (with d_beam_f and n = d_beam_len_row[row] >= 0: ids[:n], 1,
 * zeros); the first n_new finished slots restart on segments first_seg, first_seg + 1, ... (zeroed id row, counters,
 * beam-1 state, the BOS row in every form of `in`, the staged cross K/V of entry src_entry0 + i of `x` into cache row
 * slot_row[slot]); the others get slot_seg = -1; *n_done drops by the number restarted.  d_beam_f needs d_beam_len
 * and d_beam_len_row (indexed by row).  x may be NULL when n_new == 0.  h_plan (host, optional) [rows + 1]: the finished
 * slots ascending, h_plan[rows] = how many. */
int mt3_op_slot_refill(const mt3_slot_state_view* st, const mt3_input_row_view* in, float* d_beam_f, int32_t beam_rows,
                       int32_t* d_beam_len, int32_t* d_beam_len_row, int32_t* d_ids, int32_t ids_stride,
                       int32_t* d_out_ids, int32_t rows, int32_t n_new, int32_t first_seg,
                       const mt3_staged_cross_view* x, int32_t* h_plan, void* stream);
/* mt3_op_slot_refill as mt3_engine_transcribe_draws issues it: `per` consecutive DRAWS share one staged entry.  first_seg
 * and x->src_entry0 count draws; x keeps its layout, its src_batch is the number of staged ENTRIES (the encoder pass's
 * real batch, the plane stride of the chunk), and src_entry0 + n_new <= src_batch * per.  The i-th restarted slot takes
 * the staged cross K/V (and e4m3 scale rows, where x has them) of entry (src_entry0 + i) / per -- a run may start in the
 * middle of an entry's draws -- and restarts on draw first_seg + i.  per = 1 is mt3_op_slot_refill, byte for byte;
 * per < 1 is MT3_ERR_INVALID. */
int mt3_op_slot_refill_draws(const mt3_slot_state_view* st, const mt3_input_row_view* in, float* d_beam_f,
                             int32_t beam_rows, int32_t* d_beam_len, int32_t* d_beam_len_row, int32_t* d_ids,
                             int32_t ids_stride, int32_t* d_out_ids, int32_t rows, int32_t n_new, int32_t first_seg,
                             const mt3_staged_cross_view* x, int32_t per, int32_t* h_plan, void* stream);
/* The refill of mt3_engine_transcribe_beams over b->elems elements: every finished element (first slot done) with
 * slot_seg >= 0 has its k decodes walked back from the history into d_out_all[seg] [k][L] / d_out_scores[seg] [k]
 * (increasing score; optional) and the best into d_out_ids[seg] [L]; the first n_new restart (live = [0, -1e7, ...],
 * nothing finished, no fork pending, BOS rows, the staged cross K/V into each of the element's k cache rows); *n_done
 * drops by k per restarted element.  vocab <= 2048, k <= 8, num_steps <= L, (num_steps + L) * k * 2 <= 65536. */
int mt3_op_beam_refill(const mt3_beam_k_view* b, const mt3_slot_state_view* st, const mt3_input_row_view* in, int32_t L,
                       int32_t num_steps, int32_t* d_out_ids, int32_t* d_out_all, float* d_out_scores, int32_t n_new,
                       int32_t first_seg, const mt3_staged_cross_view* x, int32_t* h_plan, void* stream);
/* start of an mt3_engine_transcribe_beams job: done = 1, slot_seg = fork_src = -1, slot_row = slot for slots [0, slots);
 * d_n_done[g] = h_group_slots[g] for g < groups (1 .. 4; host array) */
int mt3_op_beam_stream_init(int32_t* d_done, int32_t* d_slot_seg, int32_t* d_fork_src, int32_t* d_slot_row,
                            int32_t* d_n_done, int32_t slots, int32_t groups, const int32_t* h_group_slots,
                            void* stream);

/* The statistics kernel of mt3_engine_score_segments on SCRIPTED logits (t5x score_batch's log-softmax / gather with
 * the row's arg-max next to it): per row, token score = (logits[target] - logsumexp(logits)) * weight with the bits
 * mt3_engine_score gives for the same logits, top-1 id = the arg-max (lowest id on equal logits), top-1 score =
 * logits[top1] - logsumexp(logits); a row whose target is 0 gets 0, 0 and 0 and is not read.
 * d_logits [rows][vocab] f32, d_targets [rows] int32 (0 = padding; ids outside [0, vocab) are clamped as mt3_engine_score
 * clamps them), d_weights [rows] f32 or NULL.  d_token_scores / d_top1_ids / d_top1_scores [rows] (each may be NULL).
 * One launch on `stream`, nothing allocated or waited for.  MT3_ERR_INVALID: NULL logits/targets, rows < 1, vocab < 2. */
int mt3_op_score_token_stats(const float* d_logits, const int32_t* d_targets, const float* d_weights, int32_t rows,
                             int32_t vocab, float* d_token_scores, int32_t* d_top1_ids, float* d_top1_scores, void* stream);

/* The other kernels of the scoring path (mt3_engine_score, mt3_engine_score_segments), each alone on memory the CALLER
 * owns and has filled (tests/test_gpu_score_attention.py, test_gpu_score_embed_reduce.py, test_gpu_three_plane_ops.py).
 * Test drivers: each fills the launch description and launches on `stream`, nothing allocated or waited for.  Every
 * argument error returns MT3_ERR_INVALID, with the entry point's name in mt3_last_error(), before anything touches a
 * device.  A chunk holds rows = segments * Lp rows, row = seg * Lp + t, Lp a multiple of 64; caller arrays are
 * [batch][length] with the chunk's first segment at index seg0.
 *
 * mt3_op_score_attention: the prefill attention, 64 queries by 64 keys per step, out = softmax(q . K^T) V with UNSCALED
 * logits over the visible keys; q / k / v / out are bf16 or f32 by `dtype`.
 *   query (b, i, h)   q + (b * Lq + i) * q_stride + h * 64            out likewise with out_stride
 *   key   (b, j, h)   k + b * kv_bstride + h * kv_hstride + j * kv_stride   (v likewise; all strides in elements)
 *   causal != 0       n_keys == Lq; query i sees key j iff j <= i and (key_tgt == NULL or key_tgt[b * Lq + j] != 0).  The K
 *                     and V rows of a key whose target is 0 are never loaded (they may hold anything, NaN and Inf
 *                     included); a causal-hidden key with a non-zero target IS loaded and gets probability exactly 0,
 *                     so it has to be finite.  A query with no visible key gets a row of zeros.
 *   causal == 0       every query sees keys 0 .. n_keys - 1 (n_keys a multiple of 64); key_tgt must be NULL.
 *   self-attention on qkv rows [B * Lq][3][H][64]: q_stride = kv_stride = 3 * H * 64, kv_bstride = Lq * 3 * H * 64, kv_hstride
 *   = 64; cross-attention on a cache [2][Bc][H][T][64]: kv_stride = 64, kv_hstride = T * 64, kv_bstride = H * T * 64.
 * MT3_ERR_INVALID: NULL view; unknown dtype; key_tgt with causal == 0; q, k or v not on 16 bytes, or q_stride, kv_stride,
 * kv_bstride or kv_hstride no multiple of 16 bytes (8 bf16 / 4 f32 elements: the kernel loads rows in 16-byte pieces);
 * q_stride or out_stride below H * 64, kv_stride below 64; NULL q / k / v / out; B, H or Lq <= 0; Lq no multiple of 64;
 * causal with n_keys != Lq; otherwise n_keys <= 0 or no multiple of 64. */
typedef struct mt3_score_attn_view {
  const void* q;
  int32_t q_stride, reserved0;
  const void* k;
  const void* v;
  int32_t kv_stride, reserved1;
  int64_t kv_bstride, kv_hstride;
  const int32_t* key_tgt;
  void* out;
  int32_t out_stride, B, H, Lq, n_keys, causal;
} mt3_score_attn_view;
int mt3_op_score_attention(int32_t dtype, const mt3_score_attn_view* v, void* stream);
/* Decoder input rows of a chunk.  Row r = seg * Lp + t, src = (seg0 + seg) * length + t:
 *   d_tgt_pad[r] = t < length ? clamp(d_targets[src]) : 0
 *   tok          = t >= length ? 0 : d_dec_in ? clamp(d_dec_in[src]) : t == 0 ? 0 (BOS) : clamp(d_targets[src - 1])
 *   d_y[r][:]    = d_table[tok][:] + d_pos[t][:]      (f32, one addition per element)
 * clamp: ids below 0 become 0, ids at or above vocab become vocab - 1.  d_table [vocab][dim], d_pos [>= Lp][dim], d_y
 * [rows][dim] f32; d_targets / d_dec_in the caller's [batch][length] int32 (d_dec_in may be NULL: shift right); nothing
 * outside d_y[0 .. rows) and d_tgt_pad[0 .. rows) is written.
 * MT3_ERR_INVALID: rows < 1, Lp < 64 or no multiple of 64, rows no multiple of Lp, length outside 1 .. Lp, seg0 < 0, dim
 * < 4 or no multiple of 4, vocab < 1, table / pos / y not on 16 bytes, NULL table / pos / targets / tgt_pad / y. */
int mt3_op_score_embed(const float* d_table, const float* d_pos, const int32_t* d_targets, const int32_t* d_dec_in,
                       int32_t* d_tgt_pad, float* d_y, int32_t rows, int32_t Lp, int32_t length, int32_t seg0, int32_t dim,
                       int32_t vocab, void* stream);
/* The reduction of a chunk: per row r = seg * Lp + t with t < length, o = (seg0 + seg) * length + t,
 *   score = d_tgt_pad[r] == 0 ? 0 : (logits[r][tgt] - logsumexp(logits[r])) * (d_weights ? d_weights[o] : 1)
 * goes to d_tok_pad[r] and, if given, d_token_scores[o]; then d_seq_scores[seg0 + seg] = float(sum over t < length of
 * d_tok_pad[seg * Lp + t]), summed in double in a fixed order.  Rows with t >= length are neither read nor written.
 * With d_top1_ids or d_top1_scores (caller [batch][length], either may be NULL) the launch is the statistics kernel of
 * mt3_engine_score_segments (mt3_op_score_token_stats states its outputs); the token and sequence scores have the
 * same bits either way.  d_logits [rows][vocab] f32, d_tgt_pad [rows] int32 (as mt3_op_score_embed leaves them).
 * MT3_ERR_INVALID: rows / Lp / length / seg0 as for mt3_op_score_embed, vocab < 1 (< 2 with a top-1 output), NULL logits /
 * tgt_pad / tok_pad / seq_scores. */
int mt3_op_score_reduce(const float* d_logits, const int32_t* d_tgt_pad, const float* d_weights, float* d_tok_pad,
                        float* d_token_scores, float* d_seq_scores, int32_t rows, int32_t Lp, int32_t length, int32_t seg0,
                        int32_t vocab, int32_t* d_top1_ids, float* d_top1_scores, void* stream);
/* d_w f32 [n] -> the three bf16 planes of mt3_op_gemm_x6's weight operand, [n] each: hi = rne_bf16(w), mid = rne_bf16(w -
 * hi), lo = rne_bf16(w - hi - mid), both differences exact in f32 (the rule the engine applies to its weights on the
 * host).  Nothing at or past index n is written.  MT3_ERR_INVALID: a NULL pointer, n < 1 or n > 2^39. */
int mt3_op_planes(const float* d_w, void* d_hi, void* d_mid, void* d_lo, int64_t n, void* stream);
/* The f32 engine's encoder-sized GEMM tile (128 x 128, six bf16 products per f32 product; MT3_OPT_ENCODER_F32_MFMA states
 * the arithmetic): d_out = epilogue( [rms(A)] * A[M][K] @ W[N][K]^T ), A f32 (row stride K), W as the planes mt3_op_planes
 * made of the f32 [N][K] matrix, outputs f32.  (norm, epilogue): (1, MT3_EPI_STORE), (1, MT3_EPI_GEGLU) -- d_out [M][N / 2],
 * W rows interleaved gate / linear in 16s as for mt3_op_gemm -- (0, MT3_EPI_RESID), (0, MT3_EPI_POS) with d_aux f32
 * [seq_len][N], (0, MT3_EPI_HEADS) with d_out [2][M / seq_len][N / 128][seq_len][64].  Any M >= 1: rows at and past M are
 * neither stored nor, for MT3_EPI_RESID, read back.
 * MT3_ERR_INVALID: M < 1, N < 128 or no multiple of 128, K < 64 or no multiple of 64, a NULL A / plane / out, A or W of
 * 4 GB or more, POS without d_aux or seq_len, HEADS with seq_len < 1 or M no multiple of it, any other (norm, epilogue). */
int mt3_op_gemm_x6(const float* d_A, const void* d_W_hi, const void* d_W_mid, const void* d_W_lo, int32_t norm,
                   int32_t epilogue, float* d_out, int32_t M, int32_t N, int32_t K, const float* d_aux, int32_t seq_len,
                   void* stream);
/* mt3_op_encoder_attention in the f32 engine's default arithmetic: Q, K, V and P as three bf16 planes each.  d_qkv f32
 * [B, T, 3, H, 64] -> d_out f32 [B, T, H*64].  MT3_ERR_INVALID: a NULL pointer, B or H < 1, T other than 256 or 512. */
int mt3_op_encoder_attention_x6(const float* d_qkv, float* d_out, int32_t B, int32_t T, int32_t H, void* stream);
/* The standalone T5 LayerNorm the engine applies once per encode (encoder_norm): per row of d_x f32 [rows][dim],
 * y = x * rsqrt(mean(x^2) + 1e-6) * d_scale[dim] -- the 1e-6 sits INSIDE the root, so a row of zeros gives exactly 0 --,
 * evaluated in f32.  d_out_ct [rows][dim] takes y in the compute type (bf16, rounded to nearest even, or f32 by `dtype`),
 * d_out_f32 [rows][dim] takes y in f32; either may be NULL and is then not written.  Nothing at or past row `rows` is
 * written.  MT3_ERR_INVALID: dtype other than MT3_BF16 / MT3_F32, a NULL d_x or d_scale, rows < 1, dim < 4 or
 * dim % 4 != 0 (rows are read and written as float4). */
int mt3_op_rmsnorm(int32_t dtype, const float* d_x, const float* d_scale, void* d_out_ct, float* d_out_f32,
                   int32_t rows, int32_t dim, void* stream);

/* MXFP8 dense path (dense_dtype MT3_FP8_E4M3; no counterpart in the reference, whose DenseGeneral is f32,
 * mt3/layers.py:311-360): operands are OCP e4m3fn bytes [rows][K] with one E8M0 power-of-two scale per 32 consecutive
 * K elements [rows][K/32]: scale = 2^(floor(log2 amax) - 7), so amax / scale lies in [128, 256) and nothing
 * saturates; elements are rounded to nearest even.  mt3_host_mx8_quantize is the host (weight) side of that rule,
 * mt3_op_mx8_quantize the device (activation) side: in_is_f32 ? f32 : bf16 rows [M][K], K a multiple of 64;
 * d_ss (f32 input only, may be NULL) receives the per-16-column sums of squares [M][K/16]. */
int mt3_host_mx8_quantize(const float* h_w, int64_t rows, int64_t K, uint8_t* h_q, uint8_t* h_sc);
int mt3_op_mx8_quantize(const void* d_in, int32_t in_is_f32, int32_t M, int32_t K, uint8_t* d_q, uint8_t* d_sc,
                        float* d_ss, void* stream);
/* out = epilogue( [rms] * A[M,K] @ W[N,K]^T ) on v_mfma_scale_f32_16x16x128_f8f6f4, f32 accumulation; K and N
 * multiples of 128.  d_a_ss != NULL: fused RMSNorm from the [M][K/16] sums of squares of the rows A was quantised
 * from (K <= 1024).  epilogue: MT3_EPI_STORE (bf16 d_out [M][N]), MT3_EPI_HEADS (bf16 [2][B][H][seq_len][64]),
 * MT3_EPI_RESID (f32 d_out [M][N] += product; the updated rows also leave as MXFP8 d_out_q / d_out_sc and their
 * per-16-column sums of squares d_out_ss), MT3_EPI_GEGLU (W rows interleaved gate/linear in 16s as for mt3_op_gemm;
 * the result gelu(gate) * linear leaves ONLY as MXFP8 d_out_q [M][N/2] / d_out_sc [M][N/64]). */
int mt3_op_gemm_mx8(const uint8_t* d_A, const uint8_t* d_a_sc, const uint8_t* d_W, const uint8_t* d_w_sc, void* d_out,
                    int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t seq_len, const float* d_a_ss,
                    uint8_t* d_out_q, uint8_t* d_out_sc, float* d_out_ss, void* stream);

/* --------------------------------------------------- symbolic stage (host CPU)
 * Replaces metrics_utils.event_predictions_to_ns (mt3/metrics_utils.py:59-146) =
 * decode_and_combine_predictions + run_length_encoding.decode_events
 * (mt3/run_length_encoding.py:371-423) + the note state machine
 * (mt3/note_sequences.py:262-446) + event_codec.Codec.decode_event_index
 * (mt3/event_codec.py:103-112).  Integer results are bit-exact with the reference;
 * times are computed in double with the reference's own expressions.
 */
enum { MT3_EV_SHIFT = 0, MT3_EV_PITCH = 1, MT3_EV_VELOCITY = 2, MT3_EV_TIE = 3, MT3_EV_PROGRAM = 4, MT3_EV_DRUM = 5 };
enum { MT3_SPEC_ONSETS = 0, MT3_SPEC_NOTES = 1, MT3_SPEC_TIES = 2 };  /* note_sequences.py:416-446 */

typedef struct mt3_event_range { int32_t type, min_value, max_value; } mt3_event_range;
typedef struct mt3_codec {
  double steps_per_second;
  int32_t num_ranges;               /* ranges[0] must be MT3_EV_SHIFT with min 0 */
  mt3_event_range ranges[8];
} mt3_codec;
typedef struct mt3_note {
  double start_time, end_time;
  int32_t pitch, velocity, program, is_drum, instrument, reserved;
} mt3_note;

/* vocabularies.build_codec (mt3/vocabularies.py:119-140) */
int mt3_build_codec(int32_t steps_per_second, int32_t max_shift_seconds, int32_t num_velocity_bins,
                    mt3_codec* out);
int mt3_codec_num_classes(const mt3_codec* c);
int mt3_codec_decode_event(const mt3_codec* c, int32_t index, int32_t* type, int32_t* value);  /* MT3_ERR_INVALID = ValueError */
int mt3_codec_encode_event(const mt3_codec* c, int32_t type, int32_t value, int32_t* index);
/* The token mask of a set of instruments (mt3_engine_set_token_masks): h_mask [ceil(vocab / 32)] uint32 with every id
 * below vocab allowed except the MT3_EV_PROGRAM events whose value is not in programs [n_programs] (n_programs < 0: all
 * programs) and, with allow_drums == 0, the MT3_EV_DRUM events.  Token id = 3 + event index (mt3_ids_to_tokens); ids at
 * or past vocab are never set.  MT3_ERR_INVALID: a program outside the codec's range, programs given for a codec without
 * a program range, vocab < 3 or null pointers. */
int mt3_codec_token_mask(const mt3_codec* c, int32_t vocab, const int32_t* programs, int32_t n_programs,
                         int32_t allow_drums, uint32_t* h_mask);
/* The event grammar of a codec (mt3_engine_set_token_grammar): the id ranges of the codec's shift, pitch and program
 * events and of its tie event (token id = 3 + event index), with_ties = (spec == MT3_SPEC_TIES), and max_steps, the largest
 * shift a free pick may take -- the segment's length in steps: floor(input_length * hop_width / sample_rate *
 * steps_per_second), 204 for `mt3` and 409 for `ismir2021`.  MT3_ERR_INVALID: null pointers, a malformed codec or one
 * without a pitch, tie or program range, max_steps < 1, max_steps above the codec's largest shift (a canonical stream
 * then needs two shifts in a row, which the rule forbids), or ranges that do not fit below vocab. */
int mt3_codec_token_grammar(const mt3_codec* c, int32_t spec, int32_t vocab, int32_t max_steps, mt3_token_grammar* out);
/* The note grammar of a codec (mt3_engine_set_note_grammar): mt3_codec_token_grammar's descriptor plus the id ranges of
 * the codec's velocity and drum events.  MT3_ERR_INVALID as there, and for a codec without a velocity or drum range, a spec
 * without a tie section, or more than 128 programs or pitches. */
int mt3_codec_note_grammar(const mt3_codec* c, int32_t spec, int32_t vocab, int32_t max_steps, mt3_note_grammar* out);
/* tokens: concatenated per-segment token rows (already trimmed at EOS); seg_offsets [n_segments+1];
 * h_has_max_time==NULL -> the combiner rule (max_time = next segment's start, none for the last);
 * otherwise explicit per-segment max_time (decode_events' own argument). */
int mt3_notes_decode(const mt3_codec* c, int32_t spec, int32_t n_segments, const int32_t* h_tokens,
                     const int64_t* h_seg_offsets, const double* h_start_times,
                     const int32_t* h_has_max_time, const double* h_max_times,
                     mt3_note* h_notes, int64_t notes_capacity, int64_t* n_notes,
                     int64_t* invalid_events, int64_t* dropped_events, double* total_time);
/* mt3_notes_decode with each note's tokens: the same notes in the same order, the same counts and total_time (one state
 * machine serves both), plus h_note_tokens [notes_capacity][2] int64 (written for the notes returned; may be NULL).  The
 * reference's state machine (note_sequences.decode_note_event, mt3/note_sequences.py:284-387) keeps no such link.
 *   [j][0]  index INTO h_tokens of the PITCH or DRUM token whose event created note j: the onset that entered the
 *           active notes (for a note carried over segments it lies in an earlier segment), or, for drums and the
 *           onsets-only spec, the token that emitted the note.
 *   [j][1]  index of the token that ended it: a PITCH token at velocity 0, the PITCH token of a re-onset, or the TIE
 *           token that closed a tie section in which the note was not declared; -1 where no token ended it (notes
 *           flushed at the end, the default durations of drums and onsets-only notes). */
int mt3_notes_decode_traced(const mt3_codec* c, int32_t spec, int32_t n_segments, const int32_t* h_tokens,
                            const int64_t* h_seg_offsets, const double* h_start_times,
                            const int32_t* h_has_max_time, const double* h_max_times,
                            mt3_note* h_notes, int64_t notes_capacity, int64_t* n_notes,
                            int64_t* invalid_events, int64_t* dropped_events, double* total_time,
                            int64_t* h_note_tokens /* [notes_capacity][2] */);

/* --------------------------------------------------- piano rolls and frame counts
 * Replaces metrics_utils.get_prettymidi_pianoroll and metrics_utils.frame_metrics (mt3/metrics_utils.py:149-196, called
 * at mt3/metrics.py:321-332 for 'Frame Precision' / 'Frame Recall' / 'Frame F1').  The reference delegates to
 * pretty_midi.PrettyMIDI.get_piano_roll and sklearn.metrics.precision_recall_fscore_support; the rule below restates the
 * reference's own lines plus the documented behaviour of those two calls [from memory, parity unpinned against the
 * libraries themselves: neither is installable here].
 *
 * The roll of one set of notes at `fps` frames per second, with the flag `is_drum`:
 *   length   a note with  is_drum != 0  or  end_time - start_time < 0.05  gets  end = start_time + 0.05  (float64; the
 *            reference writes that into its argument's notes, here the caller's notes are read only);
 *   width    F = int(fps * max end) over ALL the notes after that adjustment, drum notes included; no notes: F = 0.
 *            The caller computes F (h_widths); the device never writes at or past a row's F whatever the notes say;
 *   cells    roll[pitch, f0 : f1] += velocity  with  f0 = int(start_time * fps),  f1 = int(end * fps):  one float64
 *            product each, truncated (Python's int(x * fs)), f1 cut to F; f1 <= f0 adds nothing.  Notes on one pitch, of
 *            one program or several, sum;
 *   drums    with is_drum == 0 a note whose own drum flag is set adds nothing (pretty_midi renders a drum instrument as
 *            zeros) though it counted for F; with is_drum != 0 every note is rendered (the reference clears the
 *            instruments' flags);
 *   nothing else sounds: the two control changes the reference appends at the end time change no cell, and there is no
 *   sustain pedal and no pitch bend.
 * A note whose pitch is outside 0 .. 127 is skipped; a start or end that is negative or NaN counts as frame 0 (callers
 * reject such notes before upload: Python's slice would count a negative index from the row's end).  Every cell is a sum
 * of int32 velocities; it must stay below 2^24 in magnitude for its float32 to be exact (1,000 full-velocity notes on
 * one cell are 127,000).
 *
 * mt3_op_pianoroll: the notes of a job -> all its rolls.  Roll i takes notes [h_note_offsets[i], h_note_offsets[i + 1])
 *   of the five device arrays and is written as float32, row-major [128, h_widths[i]], at d_out + 128 *
 *   h_col_offsets[i].  The rolls must not overlap and lie in order: h_col_offsets[i + 1] >= h_col_offsets[i] +
 *   h_widths[i]; the whole span from roll 0's first cell to the last roll's end, gaps included, is written (zeros in
 *   the gaps), nothing outside it.  The cost does not depend on the notes' durations: every note makes two int32 atomic
 *   adds (+velocity at f0, -velocity at f1) into the zeroed span, and one workgroup per (roll, pitch) turns its row into
 *   running sums in place -- integer sums, so the result does not depend on the order of the atomics.
 *   The three host tables go to the kernels BY VALUE (128 rolls per launch; longer jobs are issued in pieces), so
 *   they are free when the call returns; everything is enqueued on `stream`, nothing is allocated, copied to the host or
 *   waited for.  MT3_ERR_INVALID, before any HIP call: n_rolls < 0, n_notes < 0, fps not finite or <= 0, a NULL table
 *   with n_rolls > 0, a NULL note array with n_notes > 0, h_note_offsets not non-decreasing inside [0, n_notes], more
 *   than 2^31 - 1 notes in one roll, a negative width or column offset, rolls out of order or overlapping, a span past
 *   out_capacity (in floats) or NULL d_out with a non-empty span.  n_rolls == 0, or rolls that are all of width 0, is a
 *   valid call that does nothing.
 *
 * The frame counts of a (reference roll, estimated roll) pair with `velocity_threshold`: the narrower roll counts as
 * zero from its own width on (the reference pads it), ref_on = ref > velocity_threshold (strict), est_on = est > 0, and
 * over all 128 * max(F_ref, F_est) cells  TP = #(ref_on & est_on),  FP = #(!ref_on & est_on),  FN = #(ref_on & !est_on).
 * precision = TP / (TP + FP), recall = TP / (TP + FN), F1 = 2 P R / (P + R), each 0 where its denominator is 0
 * (sklearn's value for the positive class; it warns, this library does not) -- left to the caller.
 *
 * mt3_op_frame_counts: d_counts [n_pairs][3] uint64 = (TP, FP, FN) of n_pairs pairs; pair i's rolls are float32
 *   [128, width] at d_rolls + 128 * column offset, as mt3_op_pianoroll wrote them (a roll may serve several pairs).
 *   d_counts is zeroed by the call; each workgroup counts with wave ballots and adds its three totals once.  Same
 *   contract: tables by value (128 pairs per launch), nothing allocated, copied to the host or waited for.
 *   MT3_ERR_INVALID, before any HIP call: n_pairs < 0, a NULL table or NULL d_counts with n_pairs > 0, a negative width
 *   or column offset, a roll that ends past rolls_capacity (in floats), NULL d_rolls with a pair of non-zero width, or
 *   |velocity_threshold| > 2^24 (the comparison is made in float32).  n_pairs == 0 is a valid call that does nothing.
 */
#define MT3_PIANOROLL_PITCHES 128
#define MT3_PIANOROLL_MIN_NOTE_SECONDS 0.05

int mt3_op_pianoroll(const double* d_start, const double* d_end, const int32_t* d_pitch, const int32_t* d_velocity,
                     const int32_t* d_is_drum, int64_t n_notes, int32_t n_rolls, const int64_t* h_note_offsets /* [n_rolls + 1] */,
                     const int64_t* h_col_offsets /* [n_rolls] */, const int32_t* h_widths /* [n_rolls] */, double fps,
                     int32_t is_drum, float* d_out, int64_t out_capacity, void* stream);
int mt3_op_frame_counts(const float* d_rolls, int64_t rolls_capacity, int32_t n_pairs,
                        const int64_t* h_ref_col_offsets, const int32_t* h_ref_widths,
                        const int64_t* h_est_col_offsets, const int32_t* h_est_widths /* each [n_pairs] */,
                        int32_t velocity_threshold, uint64_t* d_counts /* [n_pairs][3] */, void* stream);

/* --------------------------------------------------- rendering notes to audio
 * The audible output: what the reference's Colab does with fluidsynth and mt3/summaries.py:111-161
 * (_synthesize_example_notes, audio_summaries) with note_seq's synthesiser.  Neither a SoundFont nor any library
 * synthesiser is available to this project, so the voice is its own -- the timbre of mt3_amd.synthetic.render_notes
 * (which the trained fixture under tests/golden/ recognises) made deterministic: zero phases, a fixed summation order,
 * no added noise.  PARITY WITH ANY LIBRARY IS NOT CLAIMED.  Programs are ignored: every tonal note has the one timbre.
 *
 * job      n_seq sequences; sequence i owns n_samples[i] float32 samples at the integer sample_rate (1 .. 384000 Hz),
 *          which start at sample_offsets[i] of one output buffer.
 * note     start, end (float64 seconds), pitch 0 .. 127, velocity 0 .. 127, is_drum.  g = velocity / 127 (float32
 *          division); a note of velocity 0 adds nothing.  A note whose pitch is outside 0 .. 127 is skipped.
 * time     of sample n relative to a note:  t = (double)n / sample_rate - start:  one float64 division, then one
 *          float64 subtraction.
 * tonal    (is_drum clear)  d = end - start >= 0 (float64).  The note sounds for  0 <= t < d + 0.04  (float64 sum).
 *          env(t)  = min(t / 0.004, 1) * exp(-t / 0.7) * clamp(1 - (t - d) / 0.04, 0, 1)    (t - d in float64)
 *          f0      = 440 * 2^((pitch - 69) / 12)  in float64  (the library takes 2^(r / 12), r = 0 .. 11, from a table of
 *                    correctly rounded float64 values and scales by the octave: within 2 ulp of the expression)
 *          tone(t) = sum over k = 1 .. 6 with  k * f0 < 0.475 * sample_rate  of  sin(2 pi frac((k * f0) * t)) / k,
 *                    k ascending.  The product (k * f0) * t and its fractional part are float64 -- at t = 600 s the
 *                    sixth partial of pitch 96 has turned 7.5 million times, and float32 holds no fraction of that --
 *                    everything after is float32.
 *          Zero phase, no randomness.
 * drum     (is_drum set)  sounds for  0 <= t < 0.15  whatever its end.   x = u * exp(-t / 0.03),
 *          u = (h(pitch * 2^20 + m) >> 8) * 2^-23 - 1  (exact in float32, in [-1, 1)),  m = the sample's index counted
 *          from the note's first sounding sample (the least n with t >= 0),  h the 32-bit integer mix
 *          x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32 arithmetic).
 * sample   the float32 sum of  g * env * tone  (tonal) or  g * x  (drum) over its sequence's notes, the notes taken in
 *          ascending (start, end, pitch, velocity, is_drum) order whatever order the caller holds them in.  The order is
 *          part of the rule: float32 sums do not commute, and the same notes must give the same bits.
 * normalise (on by default in the Python layer)  peak = max |sample| over the sequence; if peak > 0 every sample is
 *          multiplied by the float32  0.9f / peak  (the inf-norm of mt3/mixing.py:71-75); a silent sequence stays zeros.
 * length   when the caller gives none:  n_samples = ceil(sample_rate * latest sounding instant), the sounding instant of
 *          a tonal note being end + 0.04 and of a drum note start + 0.15, in float64 on the host
 *          (mt3_amd.render.render_length, the only place lengths come from); no notes: 0 samples.
 *
 * mt3_op_render_notes: the notes of a job -> all its audio, in one call.  Sequence i takes notes [h_note_offsets[i],
 *   h_note_offsets[i + 1]) of the six device arrays and writes d_out[h_sample_offsets[i] .. + h_n_samples[i]); the
 *   spans must lie in order and must not overlap; NOTHING outside them is written, gaps between them included.
 *   PRECONDITION the host cannot check (the arrays are on the device): within a sequence the notes are sorted ascending
 *   by (start, end, pitch, velocity, is_drum), and d_reach[j] is the running maximum, from the sequence's first note to
 *   note j, of the notes' sounding instants (end + 0.04, or start + 0.15 for a drum note).  Unsorted notes or a wrong
 *   d_reach may give wrong audio; the kernels still read only the sequence's own notes and write only its own span.
 *   A workgroup owns a tile of MT3_RENDER_TILE consecutive samples of one sequence and walks, in order, the notes from
 *   the first whose d_reach comes up to the tile's first instant (less a guard of 2^-40, relative and absolute, that
 *   covers the roundings of the rule) to the last whose start is not past the tile's last instant -- two binary
 *   searches; a note in that range that ended before the tile is skipped.  No atomics in the accumulation.  With
 *   normalize != 0 a second kernel takes max |sample| per sequence into d_peaks (an atomic max on the bit patterns of
 *   non-negative floats: order-independent) and a third scales; d_peaks [n_seq] is zeroed by the call and holds the
 *   peaks BEFORE scaling afterwards.  With normalize == 0 d_peaks is not touched and may be NULL.
 *   Tables go to the kernels by value (128 sequences per launch); everything is enqueued on `stream`, nothing is
 *   allocated, copied to the host or waited for.  MT3_ERR_INVALID, before any HIP call: n_seq < 0, n_notes < 0,
 *   sample_rate outside 1 .. 384000, a NULL table with n_seq > 0, a NULL note array with n_notes > 0, h_note_offsets not
 *   non-decreasing inside [0, n_notes], more than 2^31 - 1 notes in one sequence, a negative length or sample offset, a
 *   sequence longer than MT3_RENDER_MAX_SAMPLES, spans out of order or overlapping, a span past out_capacity (in
 *   floats), NULL d_out with a non-empty span, NULL d_peaks with normalize != 0 and a non-empty span.  n_seq == 0, or
 *   sequences that are all of length 0, is a valid call that does nothing.
 */
#define MT3_RENDER_TILE 1024
#define MT3_RENDER_MAX_SAMPLE_RATE 384000
#define MT3_RENDER_MAX_SAMPLES (INT64_C(1) << 40)
#define MT3_RENDER_RELEASE_SECONDS 0.04
#define MT3_RENDER_DRUM_SECONDS 0.15

int mt3_op_render_notes(const double* d_start, const double* d_end, const double* d_reach, const int32_t* d_pitch,
                        const int32_t* d_velocity, const int32_t* d_is_drum, int64_t n_notes, int32_t n_seq,
                        const int64_t* h_note_offsets /* [n_seq + 1] */, const int64_t* h_sample_offsets /* [n_seq] */,
                        const int64_t* h_n_samples /* [n_seq] */, int32_t sample_rate, int32_t normalize, float* d_out,
                        int64_t out_capacity, float* d_peaks /* [n_seq] */, void* stream);

/* --------------------------------------------------- note matching
 * Replaces the matching inside mir_eval.transcription.precision_recall_f1_overlap as mt3/metrics.py calls it (lines 97-99,
 * 163-166, 267-290): for each problem of a job, the size of a MAXIMUM bipartite matching between reference and estimated
 * notes, and the matching.  The size of a maximum matching is unique, so the 'Onset', 'Onset + offset', program-aware and
 * tolerance-sweep scores that are quotients of it are pinned; which maximum matching is returned is not.  NOT BUILT: the
 * '+ velocity' scores (mir_eval.transcription_velocity fits a regression to the velocities of the particular matching
 * its Hopcroft-Karp returned, so their value depends on WHICH maximum matching one holds and cannot be pinned without
 * mir_eval itself).
 *
 * job      packed float64 device arrays over all notes of the job: onset, offset (seconds) and log2(pitch) -- the
 *          logarithm is taken on the host (numpy's log2), so the cents comparison never depends on a device log2.
 * problem  reference notes [ref0, ref0 + n_ref), estimated notes [est0, est0 + n_est) SORTED ASCENDING BY ONSET (the caller
 *          sorts them, stably), its state at d_workspace + state0 (in int32 words), and an index into the rule table.
 *          Note ranges may be shared between problems (the onset-only, onset + offset and sweep problems of one track
 *          read the same notes); state ranges may not.
 * rule     onset_tolerance, pitch_tolerance, offset_ratio (MT3_NOTE_MATCH_NO_OFFSET: no offset test),
 *          offset_min_tolerance, strict.
 * edge     reference note i and estimate j can be paired when all of the following hold, every operation float64 and
 *          rounded on its own (no fused multiply-add):
 *            D(a, b) = rint(|a - b| * 1e6) / 1e6            (numpy's around(., 6): one product, rint, one quotient)
 *            onset    D(ref_on, est_on) <= onset_tolerance
 *            cents    |1200 * (l2_ref - l2_est)| <= pitch_tolerance, a NaN difference counting as 0
 *            offset   D(ref_off, est_off) <= max(offset_ratio * (ref_off - ref_on), offset_min_tolerance)
 *          with every <= a < under `strict`; and j lies in i's window, the estimates whose onset is in
 *          [ref_on - m, ref_on + m], m = onset_tolerance + 1e-6 (found by binary search; it contains every j that passes
 *          the onset test).  Adjacency is never stored: the predicate is evaluated again wherever it is needed, so no
 *          size depends on a count the host would have to wait for.
 * state    per problem, int32 words: mate_ref [n_ref] first -- the output: the estimate (index within the problem, in
 *          its sorted order) matched to reference i, or -1 -- then five more arrays of n_ref (window bounds, level,
 *          cursor, parent) and two of n_est (mate_est, claim).  Problems with unsorted estimates or NaN times may give a
 *          matching that is not maximum; the kernel still touches only its own notes and its own state.
 * warm start  with warm_start != 0 mate_ref is read as an initial partial matching.  An entry is kept only if it lies in
 *          the window, passes the edge rule and claims an estimate no other entry has claimed; anything else counts as
 *          -1.  A bad warm start therefore costs matches, never memory safety.  warm_start == 0: start empty.
 * algorithm  one workgroup of 256 lanes per problem, 64 problems per launch, launches in stream order (so at most 64
 *          workgroups are in flight at a time): a greedy pass (compare-and-swap on the estimate's mate), then
 *          Hopcroft-Karp phases -- a level-synchronous breadth-first search from the free references, then one lane per
 *          free reference walking the levels depth-first with its path in the state (no per-lane stack), estimates
 *          claimed atomically so that paths are vertex-disjoint.  A phase whose search found a free estimate and whose
 *          walks augmented nothing repeats the walk with one lane, so every phase adds a match; there are at most
 *          min(n_ref, n_est) + 1 phases.  Should that bound ever be passed, the problem's count is written as -1.
 *
 * The state-words query: the int32 words of one problem's state, 6 n_ref + 2 n_est; -1 for a negative count.
 *
 * The matching op: d_matched [n_problems] int32 = the size of each problem's maximum matching (0 for a problem with an
 *   empty side, whose mate_ref is all -1).  The two host tables go to the kernel BY VALUE (64 problems per launch, at most
 *   MT3_NOTE_MATCH_MAX_RULES rules), so they are free when the call returns; everything is enqueued on `stream`, nothing
 *   is allocated, copied to the host or waited for.  MT3_ERR_INVALID, before any HIP call: a negative n_problems, n_notes,
 *   workspace_words or note count, n_rules outside 0 .. MT3_NOTE_MATCH_MAX_RULES, a NULL rule table with n_rules > 0, a
 *   tolerance that is negative or not finite (offset_ratio: or not MT3_NOTE_MATCH_NO_OFFSET), a NULL problem table or NULL
 *   d_matched with n_problems > 0, a NULL note array with n_notes > 0, a note range outside [0, n_notes], a rule index
 *   out of range, state ranges that overlap or are out of order (state0 must not decrease below the previous problem's
 *   end) or end past workspace_words, NULL d_workspace with a non-empty state.  n_problems == 0 is a valid call that
 *   does nothing.
 */
#define MT3_NOTE_MATCH_MAX_RULES 16
#define MT3_NOTE_MATCH_NO_OFFSET (-1.0)

typedef struct mt3_match_rule {
  double onset_tolerance, pitch_tolerance;
  double offset_ratio;                /* MT3_NOTE_MATCH_NO_OFFSET: onsets and pitches only */
  double offset_min_tolerance;
  int32_t strict;
  int32_t reserved;
} mt3_match_rule;

typedef struct mt3_match_problem {
  int64_t ref0, est0;                 /* first reference / estimated note, in notes */
  int64_t state0;                     /* first word of the state in d_workspace */
  int32_t n_ref, n_est;
  int32_t rule;
  int32_t reserved;
} mt3_match_problem;

int64_t mt3_note_match_state_words(int32_t n_ref, int32_t n_est);
int mt3_op_match_notes(const double* d_onset, const double* d_offset, const double* d_log2_pitch, int64_t n_notes,
                       int32_t n_problems, const mt3_match_problem* h_problems /* [n_problems] */, int32_t n_rules,
                       const mt3_match_rule* h_rules /* [n_rules] */, int32_t* d_workspace, int64_t workspace_words,
                       int32_t warm_start, int32_t* d_matched /* [n_problems] */, void* stream);

/* --------------------------------------------------- target tokenizer: notes -> the id rows the model is trained on
 * The target side of the reference's data pipeline: mt3/preprocessors.py:93-226 (tokenize_transcription_example) and
 * mt3/tasks.py:160-180 (extract_target_sequence_with_indices with the tie token, map_midi_programs,
 * run_length_encode_shifts, remove_redundant_state_changes(['velocity', 'program']), trim, EOS), for the segments the
 * inference path cuts.  The rule is stated once, below (mt3t_*); mt3_notes_tokenize is that rule on host arrays and
 * mt3_op_tokenize_notes is the kernel that compiles the same functions.  Integers only: no floating point on the device.
 *
 * events   of one file, prepared by the host ALREADY IN THE REFERENCE'S ORDER (mt3_amd.tokenize.pack), six int32 arrays:
 *          step     round(time * steps_per_second), Python's round (half to even on the float64 product), not negative and
 *                   below INT32_MAX; ascending within a file (the host's stable sort by float64 time);
 *          pitch, program   0 .. 127 (both are taken & 127: a bad value costs tokens, never memory safety);
 *          velbin   0 = an offset, otherwise vocabularies.velocity_to_bin (taken clamped to 0 .. velocity_count - 1);
 *          is_drum  (read by MT3_SPEC_TIES only);   note   the index of the event's note in the caller's list.
 * segment  step_lo, step_hi: its events are those with step_lo <= step < step_hi (two binary searches); the last segment
 *          of a file has step_hi = INT32_MAX.
 * row      1. tie section (MT3_SPEC_TIES only).  b = the first event with step >= step_lo; if there is none, the FIRST
 *             event whose step equals the file's last step (the reference's frozen_state_idx: its trailing shifts do not
 *             refresh the state index, so trailing silence keeps the state from BEFORE the last step's first event --
 *             reproduced, not repaired); 0 for an empty file (mt3t_tie_begin).  Events 0 .. b - 1 are replayed into a
 *             table keyed by (program, pitch): drums skipped, velbin != 0 sets, velbin == 0 clears, the last writer
 *             wins.  The held pairs go out in ascending (program, pitch) order as program id, pitch id; then tie_id.
 *          2. the segment's events: [shift] program velocity pitch, or [shift] velocity drum for a drum, or [shift]
 *             velocity pitch under MT3_SPEC_NOTES.  With d = step - step_lo, shift ids come before an event exactly when d
 *             exceeds the d of the segment's previous event (0 before the first); a d above max_shift_steps is split into
 *             d / max_shift_steps ids of max_shift_steps and, if not zero, one of the rest (mt3t_shift_count, _value).
 *          3. program granularity: program_map[p], keyed by the ORIGINAL program, is the program to write, or -1 to write
 *             no program id for it (full: p; midi_class: 8 * (p / 8); flat: -1).
 *          4. redundant state changes, over the whole row: a program id equal to the last program id before it in the
 *             row is dropped, a velocity id likewise against the last velocity id; "none yet" matches nothing.
 *          5. EOS (1), then the cut to `stride` ids: a row that does not fit ends without EOS and has truncated = 1.
 * outputs  per row: ids [stride] int32, 0-padded; length (EOS included); truncated; note_of [stride] int32: at every pitch
 *          or drum id of the EVENT part the event's `note`, -1 elsewhere (tie section included); is_onset [stride] uint8:
 *          1 at those positions where the event's velbin is not 0, else 0.
 * mt3_codec_tokenize_rule fills the descriptor from a codec: the id bases (token id = 3 + event index), max_shift_steps
 *   and the map of `granularity` (MT3_GRANULARITY_*).  MT3_ERR_INVALID: null pointers, a malformed codec, a spec other
 *   than MT3_SPEC_NOTES / MT3_SPEC_TIES, an unknown granularity, a codec without pitch, velocity (from 0), tie, program and
 *   drum ranges or whose pitch, program or drum range is not 0 .. 127, ranges that do not fit below vocab.
 * mt3_notes_tokenize: one row of one file on HOST arrays (n_events >= 0; the arrays may be NULL when it is 0).
 * mt3_op_tokenize_notes: a JOB in one launch.  d_files [n_files]: each file's event range in the six device arrays and
 *   its rows [row0, row0 + n_rows); d_rows [rows]: file, step_lo, step_hi, in ascending step_lo within a file.  One
 *   workgroup of 256 lanes per file walks its rows in order; the held table stays in LDS and is advanced by the events
 *   between consecutive tie-section starts (last writer by an LDS table of positions, as mt3_op_tie_prompts).  Indices read
 *   from the two device tables are range-checked in the kernel: a file whose event range leaves [0, n_events] counts as
 *   empty, rows outside [0, rows) or owned by another file are not written, a tie-section start that runs backwards
 *   leaves the table as it is.  Enqueued on `stream`; nothing is allocated, copied or waited for.
 * MT3_ERR_INVALID, before any HIP call (both entry points, where the argument exists): a null rule, table or output
 *   pointer; a null event array with n_events > 0; n_events < 0; n_files < 1; rows < 1; stride < 2 or above 2^20; a spec
 *   other than the two; max_shift_steps < 1; velocity_count < 1; a program_map entry outside -1 .. 127; vocab < 4 or an id
 *   base whose range does not lie in [3, vocab). */
enum { MT3_GRANULARITY_FULL = 0, MT3_GRANULARITY_MIDI_CLASS = 1, MT3_GRANULARITY_FLAT = 2 };
#define MT3_TOKENIZE_PROGRAMS 128
#define MT3_TOKENIZE_PITCHES 128
#define MT3_TOKENIZE_MAX_STRIDE (1 << 20)

typedef struct mt3_tokenize_rule {
  int32_t spec, vocab, max_shift_steps;
  int32_t shift_first, pitch_first, velocity_first, velocity_count, tie_id, program_first, drum_first;
  int32_t reserved[2];
  int32_t program_map[MT3_TOKENIZE_PROGRAMS];
} mt3_tokenize_rule;

typedef struct mt3_tokenize_file {
  int64_t event0;                     /* first event of the file in the job's event arrays */
  int32_t n_events;
  int32_t row0, n_rows;               /* its rows, one per segment, in order */
  int32_t reserved;
} mt3_tokenize_file;

typedef struct mt3_tokenize_row {
  int32_t file, step_lo, step_hi, reserved;
} mt3_tokenize_row;

/* the first i in [0, n) with step[i] >= key, n if there is none */
MT3_RULE_FN int32_t mt3t_lower_bound(const int32_t* step, int32_t n, int32_t key) {
  int32_t lo = 0, hi = n < 0 ? 0 : n;
  while (lo < hi) {                                          /* at most 32 rounds */
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (step[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
/* b of the tie section: the events before it are the ones replayed */
MT3_RULE_FN int32_t mt3t_tie_begin(const int32_t* step, int32_t n, int32_t step_lo) {
  if (n <= 0) return 0;
  const int32_t b = mt3t_lower_bound(step, n, step_lo);
  return b < n ? b : mt3t_lower_bound(step, n, step[n - 1]);
}
MT3_RULE_FN int32_t mt3t_index(int32_t v) { return (int32_t)((uint32_t)v & 127u); }
MT3_RULE_FN int32_t mt3t_velbin(const mt3_tokenize_rule* r, int32_t v) {
  return v < 0 ? 0 : (v >= r->velocity_count ? r->velocity_count - 1 : v);
}
/* the shift ids in front of an event at d steps from the segment's start, the event before it at `prev` */
MT3_RULE_FN int64_t mt3t_shift_count(const mt3_tokenize_rule* r, int64_t d, int64_t prev) {
  return d > prev ? (d + r->max_shift_steps - 1) / r->max_shift_steps : 0;
}
/* the value of the k-th of them */
MT3_RULE_FN int32_t mt3t_shift_value(const mt3_tokenize_rule* r, int64_t d, int64_t k) {
  return k < d / r->max_shift_steps ? r->max_shift_steps : (int32_t)(d % r->max_shift_steps);
}
/* what the op's argument checks say about a rule and a stride: NULL if fine */
MT3_RULE_FN const char* mt3t_bad_rule(const mt3_tokenize_rule* r, int32_t stride) {
  if (!r) return "null rule";
  if (stride < 2 || stride > MT3_TOKENIZE_MAX_STRIDE) return "stride must be in [2, 2^20]";
  if (r->spec != 1 /* MT3_SPEC_NOTES */ && r->spec != 2 /* MT3_SPEC_TIES */) return "spec must be MT3_SPEC_NOTES or MT3_SPEC_TIES";
  if (r->max_shift_steps < 1) return "max_shift_steps must be at least 1";
  if (r->velocity_count < 1) return "velocity_count must be at least 1";
  for (int32_t p = 0; p < MT3_TOKENIZE_PROGRAMS; ++p)
    if (r->program_map[p] < -1 || r->program_map[p] > 127) return "program_map entries must be in -1 .. 127";
  if (r->vocab < 4) return "vocab must be at least 4";
  {
    const int64_t v = r->vocab;
    if (r->shift_first < 3 || (int64_t)r->shift_first + r->max_shift_steps >= v) return "id base: the shift ids do not fit vocab";
    if (r->pitch_first < 3 || (int64_t)r->pitch_first + MT3_TOKENIZE_PITCHES > v) return "id base: the pitch ids do not fit vocab";
    if (r->velocity_first < 3 || (int64_t)r->velocity_first + r->velocity_count > v)
      return "id base: the velocity ids do not fit vocab";
    if (r->spec == 2) {
      if (r->tie_id < 3 || r->tie_id >= v) return "id base: tie_id does not fit vocab";
      if (r->program_first < 3 || (int64_t)r->program_first + MT3_TOKENIZE_PROGRAMS > v)
        return "id base: the program ids do not fit vocab";
      if (r->drum_first < 3 || (int64_t)r->drum_first + MT3_TOKENIZE_PITCHES > v) return "id base: the drum ids do not fit vocab";
    }
  }
  return 0;
}
/* one id at position *at of a row, if it still fits; the position advances either way */
MT3_RULE_FN void mt3t_put(int32_t stride, int64_t* at, int32_t id, int32_t note, int32_t onset, int32_t* ids,
                          int32_t* note_of, uint8_t* is_onset) {
  if (*at < stride) {
    ids[*at] = id;
    note_of[*at] = note;
    is_onset[*at] = (uint8_t)onset;
  }
  ++*at;
}
/* EOS or the cut, the padding, length and truncated of a row whose ids end at `at` */
MT3_RULE_FN void mt3t_finish(int32_t stride, int64_t at, int32_t* ids, int32_t* note_of, uint8_t* is_onset, int32_t* length,
                             int32_t* truncated) {
  if (at < stride) mt3t_put(stride, &at, 1, -1, 0, ids, note_of, is_onset);
  else { *length = stride; *truncated = 1; return; }
  *length = (int32_t)at;
  *truncated = 0;
  while (at < stride) mt3t_put(stride, &at, 0, -1, 0, ids, note_of, is_onset);
}
/* THE RULE: one row, serially.  The arrays are the file's own (event 0 first). */
MT3_RULE_FN void mt3t_row(const mt3_tokenize_rule* r, const int32_t* step, const int32_t* pitch, const int32_t* program,
                          const int32_t* velbin, const int32_t* is_drum, const int32_t* note, int32_t n_events,
                          int32_t step_lo, int32_t step_hi, int32_t stride, int32_t* ids, int32_t* note_of,
                          uint8_t* is_onset, int32_t* length, int32_t* truncated) {
  const int ties = r->spec == 2 /* MT3_SPEC_TIES */;
  int64_t at = 0, prev = 0;
  int32_t last_program = -1, last_velocity = -1;
  if (n_events < 0) n_events = 0;
  if (ties) {
    uint32_t held[MT3_TOKENIZE_PROGRAMS * MT3_TOKENIZE_PITCHES / 32];
    const int32_t b = mt3t_tie_begin(step, n_events, step_lo);
    for (int32_t w = 0; w < MT3_TOKENIZE_PROGRAMS * MT3_TOKENIZE_PITCHES / 32; ++w) held[w] = 0;
    for (int32_t e = 0; e < b; ++e) {
      if (is_drum[e]) continue;
      const int32_t bit = mt3t_index(program[e]) * MT3_TOKENIZE_PITCHES + mt3t_index(pitch[e]);
      if (mt3t_velbin(r, velbin[e])) held[bit >> 5] |= 1u << (bit & 31);
      else held[bit >> 5] &= ~(1u << (bit & 31));
    }
    for (int32_t bit = 0; bit < MT3_TOKENIZE_PROGRAMS * MT3_TOKENIZE_PITCHES; ++bit) {
      if (!((held[bit >> 5] >> (bit & 31)) & 1u)) continue;
      const int32_t m = r->program_map[bit / MT3_TOKENIZE_PITCHES];
      if (m >= 0 && m != last_program) mt3t_put(stride, &at, r->program_first + m, -1, 0, ids, note_of, is_onset);
      if (m >= 0) last_program = m;
      mt3t_put(stride, &at, r->pitch_first + bit % MT3_TOKENIZE_PITCHES, -1, 0, ids, note_of, is_onset);
    }
    mt3t_put(stride, &at, r->tie_id, -1, 0, ids, note_of, is_onset);
  }
  {
    const int32_t e_lo = mt3t_lower_bound(step, n_events, step_lo);
    const int32_t e_hi = step_hi > step_lo ? mt3t_lower_bound(step, n_events, step_hi) : e_lo;
    for (int32_t e = e_lo; e < e_hi; ++e) {
      const int64_t d = (int64_t)step[e] - step_lo, n_shift = mt3t_shift_count(r, d, prev);
      const int32_t v = mt3t_velbin(r, velbin[e]), drum = ties && is_drum[e];
      for (int64_t k = 0; k < n_shift && at < stride; ++k)
        mt3t_put(stride, &at, r->shift_first + mt3t_shift_value(r, d, k), -1, 0, ids, note_of, is_onset);
      if (n_shift && at >= stride) at = (int64_t)stride + 1;       /* the rest of them are past the cut */
      prev = d;
      if (ties && !drum) {
        const int32_t m = r->program_map[mt3t_index(program[e])];
        if (m >= 0 && m != last_program) mt3t_put(stride, &at, r->program_first + m, -1, 0, ids, note_of, is_onset);
        if (m >= 0) last_program = m;
      }
      if (v != last_velocity) mt3t_put(stride, &at, r->velocity_first + v, -1, 0, ids, note_of, is_onset);
      last_velocity = v;
      mt3t_put(stride, &at, (drum ? r->drum_first : r->pitch_first) + mt3t_index(pitch[e]), note[e], v != 0, ids, note_of,
               is_onset);
    }
  }
  mt3t_finish(stride, at, ids, note_of, is_onset, length, truncated);
}

int mt3_codec_tokenize_rule(const mt3_codec* c, int32_t spec, int32_t vocab, int32_t granularity, mt3_tokenize_rule* out);
int mt3_notes_tokenize(const mt3_tokenize_rule* r, const int32_t* h_step, const int32_t* h_pitch, const int32_t* h_program,
                       const int32_t* h_velbin, const int32_t* h_is_drum, const int32_t* h_note, int32_t n_events,
                       int32_t step_lo, int32_t step_hi, int32_t stride, int32_t* h_ids /* [stride] */,
                       int32_t* h_note_of /* [stride] */, uint8_t* h_is_onset /* [stride] */, int32_t* h_length,
                       int32_t* h_truncated);
int mt3_op_tokenize_notes(const mt3_tokenize_rule* r, const int32_t* d_step, const int32_t* d_pitch, const int32_t* d_program,
                          const int32_t* d_velbin, const int32_t* d_is_drum, const int32_t* d_note, int64_t n_events,
                          const mt3_tokenize_file* d_files, int32_t n_files, const mt3_tokenize_row* d_rows, int32_t rows,
                          int32_t stride, int32_t* d_ids /* [rows][stride] */, int32_t* d_lengths /* [rows] */,
                          int32_t* d_truncated /* [rows] */, int32_t* d_note_of /* [rows][stride] */,
                          uint8_t* d_is_onset /* [rows][stride] */, void* stream);

/* ---- shift paths: the best time shift per segment of every file of a job (alignment of known notes to audio).
 * d_scores [total_segments][K] f32: the log-probability of segment s under shift j of the grid, as
 * mt3_engine_score_candidates writes its sequence scores with per = K.  h_files [n_files][2] int32: (first segment,
 * segments S) of each file, in increasing order and without overlap.  h_grid [K] float64: the shifts in seconds,
 * finite and strictly increasing, 1 <= K <= MT3_ALIGN_MAX_SHIFTS.  smoothness: lambda >= 0 (finite), in log-probability
 * per second of jump between neighbouring segments.  max_jump >= 0: the largest jump allowed, INFINITY: any.
 * THE RULE, per file, all in float64 (numpy statement: mt3_amd/alignment.py, best_paths_reference):
 *   c[s][j] = -(double)score[s][j];   D[0][j] = c[0][j];
 *   D[s][j] = c[s][j] + min over k with |g_j - g_k| <= max_jump of (D[s-1][k] + lambda * |g_j - g_k|),
 * the LOWEST k on equal values; the path ends at the lowest j of minimal D[S-1][j] and is read back through the stored k.
 * Every difference, product and sum is rounded once, in the order written (no fused multiply-add), so the device
 * result is numpy's bit for bit.  The scores must be finite (with NaN or infinite scores the path is still a row of
 * indices in [0, K), but which one is not stated).
 * d_path [total_segments] int32: the shift index of every segment that belongs to a file (the others are not written);
 * d_total [n_files] float64: D[S-1] at the path's end = minus the path's log-probability plus its jump penalties.
 * d_backptr: total_segments * K bytes of scratch (the stored k of every (segment, shift)), so the number of segments of
 * a file is not bounded by LDS.  Work: one workgroup of 64 lanes per file, lane j owns shift j, the row D[s-1][.] in
 * LDS; 64 files per launch (their table and the grid ride in the kernel arguments), the launches one after the other on
 * `stream`.  Microseconds for a job: the kernel exists so that the table never leaves the device, not for speed.
 * MT3_ERR_INVALID, before any device work: a NULL pointer; K outside 1 .. 64; a grid that is not finite and strictly
 * increasing; lambda or max_jump negative or NaN, lambda infinite; total_segments or n_files < 0; S < 1; a segment range
 * outside [0, total_segments], overlapping the one before it or out of order.  n_files == 0 is MT3_OK and does
 * nothing. */
#define MT3_ALIGN_MAX_SHIFTS 64
int mt3_op_align_paths(const float* d_scores /* [total_segments][K] */, int32_t total_segments, int32_t K,
                       const int32_t* h_files /* [n_files][2] */, int32_t n_files, const double* h_grid /* [K] */,
                       double smoothness, double max_jump, uint8_t* d_backptr /* [total_segments * K] */,
                       int32_t* d_path /* [total_segments] */, double* d_total /* [n_files] */, void* stream);

/* ---- note consensus: n transcriptions of a file -> one transcription, and for every note the voters that have it.
 * VOTERS  a file has V voters, 1 <= V <= MT3_CONSENSUS_MAX_VOTERS; a voter is one transcription, numbered 0 .. V - 1, and
 *   may have no notes.
 * KEY     key = is_drum << 14 | program << 7 | pitch (int32; the host packs it, and zeroes the program field when
 *   instruments are not to split a vote).  The kernel compares keys and copies them; it never takes one apart.
 * ORDER   the notes of a file, from all its voters together, lie SORTED by (key, onset, offset, velocity, voter): a total
 *   order up to exact duplicates, so the result does not depend on the order the caller held the notes in.  The host
 *   sorts (numpy's lexsort); the op takes sorted columns.
 * CLUSTERS  single linkage on onsets within a key.  Note i of the sorted file starts a cluster when it is the file's
 *   first note, or key[i] != key[i-1], or onset[i] - onset[i-1] > tolerance: ONE float64 difference, rounded once, and
 *   one comparison.  A cluster is therefore a contiguous run [a, b) of m = b - a members.  Rounding is monotone, so these
 *   runs are the connected components of "same key and |onset difference| <= tolerance" over ALL pairs.  Limit: repeated
 *   notes of one key closer than the tolerance chain into one cluster; `members` > `votes` shows such a chain.
 * PER CLUSTER  votes = the number of distinct voters among the members (the population count of a 64-bit mask; a voter
 *   number is taken modulo 64), members = m; the cluster is KEPT when votes >= the file's min_votes (1 .. V).
 * THE EMITTED NOTE of a kept cluster is made of member values alone -- no arithmetic, so nothing rounds:
 *   key       the cluster's;
 *   onset     of the member at position a + (m - 1) / 2: the run is sorted by onset, so this is the lower median;
 *   offset    the member offset of rank (m - 1) / 2 under the order (offset, position);
 *   velocity  the member velocity of rank (m - 1) / 2 under the order (velocity, position).
 *   Every member has offset >= onset, so the k-th smallest offset is >= the k-th smallest onset: an emitted note never
 *   ends before it starts.
 * OUTPUTS (device)  the kept notes of each file compacted in the sorted order, (key, onset), from the position where the
 *   file's input starts (so each output column has n_notes entries; those past a file's count are not written), with
 *   their votes and members; d_counts [n_files]: the kept notes of each file (0 for a file without notes);
 *   d_note_votes [n_notes]: for every input note of a file, in the sorted order, the votes of its cluster, kept or not.
 * WORK  one workgroup of MT3_CONSENSUS_TILE lanes per file, 64 files per launch (their table rides in the kernel
 *   arguments), the launches one after the other on `stream`.  The workgroup walks its file in tiles of
 *   MT3_CONSENSUS_TILE notes, the scan state carried from tile to tile, so a file's length is not bounded by LDS:
 *     1. head flags, and their running sum: each note's cluster number and each cluster's start;
 *     2. per cluster head: the voter mask over its members, votes, kept; a running sum of the kept flags places it;
 *     3. per note: the ranks of its offset and velocity among its cluster's members; the member of the wanted rank (for
 *        the onset: position) writes that field of the emitted note.  Every output word has exactly one writer.
 *   The loops over members are O(m) per note, and m is about V in real input; a degenerate file whose notes all fall
 *   into one cluster costs O(n^2): slow, but finite.  No atomics, no floating-point arithmetic but the one difference:
 *   the same input gives the same bits on every run, and they are numpy's (mt3_amd/consensus.py, consensus_reference).
 * d_scratch: int32 words, at least MT3_CONSENSUS_SCRATCH_WORDS(n_notes) = 4 * n_notes (cluster number of every note;
 *   start, votes and output place of every cluster).
 * SAFETY  every index is derived from the file table, which is checked below before any device work.  Columns that are
 *   not sorted as required (or hold NaN) give unspecified notes, but cluster runs are built from positions alone, so no
 *   read or write leaves the file's own ranges.
 * MT3_ERR_INVALID, before any device work: NULL note columns with n_notes > 0, NULL outputs, NULL scratch, a NULL file
 *   table with n_files > 0; n_notes or n_files negative; a file's note range outside [0, n_notes], overlapping the one
 *   before it or out of order; n_voters outside 1 .. 64; min_votes outside 1 .. n_voters; a tolerance that is negative
 *   or not finite; scratch_words below the formula.  n_files == 0 is MT3_OK and launches nothing. */
#define MT3_CONSENSUS_MAX_VOTERS 64
#define MT3_CONSENSUS_TILE 256
#define MT3_CONSENSUS_SCRATCH_WORDS(n_notes) (4 * (int64_t)(n_notes))

typedef struct mt3_consensus_file {
  int64_t first;                      /* the file's first note in the columns; its output starts there too */
  int32_t n_notes;
  int32_t n_voters;                   /* 1 .. MT3_CONSENSUS_MAX_VOTERS */
  int32_t min_votes;                  /* 1 .. n_voters */
  int32_t reserved;
} mt3_consensus_file;

int mt3_op_note_consensus(const double* d_onset, const double* d_offset, const int32_t* d_key, const int32_t* d_velocity,
                          const int32_t* d_voter, int64_t n_notes, const mt3_consensus_file* h_files /* [n_files] */,
                          int32_t n_files, double tolerance, double* d_out_onset, double* d_out_offset,
                          int32_t* d_out_key, int32_t* d_out_velocity, int32_t* d_out_votes, int32_t* d_out_members,
                          int32_t* d_note_votes /* [n_notes] */, int32_t* d_counts /* [n_files] */, int32_t* d_scratch,
                          int64_t scratch_words, void* stream);

/* ---- note preparation: known notes as the reference prepares them before tokenizing.  Two modes over the same skeleton;
 * a job that wants both calls twice.  The host statement, event by event: mt3_amd/note_sequences.py.
 * MT3_NOTE_PREP_SUSTAIN  note_seq.apply_sustain_control_changes [from memory: parity unpinned against note_seq]: a note
 *   whose key goes up while its instrument's sustain pedal (controller 64, down from value 64 on) is down lasts until the
 *   pedal goes up, or until the same pitch of that instrument is struck again under the pedal.
 *   KEY    key = instrument << 7 | pitch (int32; the kernel reads the instrument as key >> 7).
 *   PEDAL  the controller-64 events of a file lie SORTED by (instrument, time, ON before OFF) as
 *     inst_state = instrument << 1 | (1 for OFF: value < 64).  ped(g, t): the state after g's last event with time <= t,
 *     up when there is none; rel(g, t): the time of g's first OFF with time > t, or none.
 *   t_last  the largest time among the file's note starts, note ends and controller-64 events, 0 for an empty file.
 *   RULE   for note i (start s, end e, instrument g) let j be the FIRST later note of its key, in the order
 *     (start, pos), with ped(g, s_j) down.
 *       cut   if ped(g, e) is down and s_j < rel(g, e) (or there is no rel), or ped(g, e) is up and s_j <= e:
 *             the new end is s_j, and the note is DELETED when s_j == s;
 *       hold  else, if ped(g, e) is down: the new end is rel(g, e), or t_last when there is none;
 *       else  the end stays.
 *     total_time: t_last if any note was held to t_last; else the largest of the old value and every rel a note was held to.
 * MT3_NOTE_PREP_TRIM  mt3 trim_overlapping_notes (mt3/note_sequences.py:52-69).  key = is_drum << 14 | program << 7 |
 *   pitch; j is the NEXT note of the key in the order (start, pos); the new end is s_j if e > s_j, else e; the note is
 *   deleted unless s < the new end.  total_time stays.  The pedal arguments are not read.
 * ORDER   a file's notes lie SORTED by (key, start, pos), pos = the note's position in the caller's own order, 0 .. n - 1,
 *   each once.  The host sorts; the op takes sorted columns.
 * OUTPUTS (device)  the surviving notes of each file in the CALLER'S order, compacted from the position where the file's
 *   input starts: d_out_end the new end, d_out_src the note's pos (entries past a file's count are not written);
 *   d_counts [n_files] the survivors, d_total_time [n_files] the new total_time.  No end is computed: each is a note
 *   start, a pedal time, t_last or the old end, so the result equals the host statement bit for bit.
 * WORK  one workgroup of MT3_NOTE_PREP_TILE lanes per file, 64 files per launch (their table rides in the kernel
 *   arguments), the launches one after the other on `stream`; tiles of MT3_NOTE_PREP_TILE items, scan state carried from
 *   tile to tile: (0, sustain) a reversed max-scan over the pedal events -> the next OFF at or after each, so that rel is a
 *   binary search and one read however long a held pedal's run of ON values is; (1) a reversed max-scan over the notes
 *   flagged ped(g, start) (trim: all) -> j, the case analysis, new end and keep flag into scratch at pos; (2) a sum-scan of
 *   the keep flags over the caller's order compacts.  No atomics.
 * d_scratch: int32 words, 8-byte aligned, at least MT3_NOTE_PREP_SCRATCH_WORDS(n_notes, n_pedal) = 3 * n_notes + n_pedal
 *   (n_pedal counts 0 in trim mode).
 * SAFETY  every index comes from the file table, checked below, from the scans or from a binary search over the file's own
 *   range; a pos outside 0 .. n - 1 is not written.  Columns that are not as required give unspecified notes, but no read or
 *   write leaves the file's own ranges.
 * MT3_ERR_INVALID, before any device work: an unknown mode; n_notes, n_pedal or n_files negative; NULL note columns with
 *   n_notes > 0, NULL pedal columns with n_pedal > 0 (sustain), NULL outputs, NULL or misaligned scratch, a NULL file table
 *   with n_files > 0; a file's note or pedal range outside its column, overlapping the one before it or out of order; a
 *   t_last or total_time that is not finite; scratch_words below the formula.  n_files == 0 is MT3_OK and launches
 *   nothing. */
#define MT3_NOTE_PREP_SUSTAIN 0
#define MT3_NOTE_PREP_TRIM 1
#define MT3_NOTE_PREP_TILE 256
#define MT3_NOTE_PREP_SCRATCH_WORDS(n_notes, n_pedal) (3 * (int64_t)(n_notes) + (int64_t)(n_pedal))

typedef struct mt3_note_prep_file {
  int64_t first;                      /* the file's first note in the columns; its output starts there too */
  int64_t pedal_first;                /* the file's first pedal event in the pedal columns */
  int32_t n_notes;
  int32_t n_pedal;
  double t_last;
  double total_time;
} mt3_note_prep_file;

int mt3_op_prepare_notes(int32_t mode, const double* d_start, const double* d_end, const int32_t* d_key,
                         const int32_t* d_pos, int64_t n_notes, const double* d_pedal_time,
                         const int32_t* d_pedal_inst_state, int64_t n_pedal,
                         const mt3_note_prep_file* h_files /* [n_files] */, int32_t n_files, double* d_out_end,
                         int32_t* d_out_src, int32_t* d_counts /* [n_files] */, double* d_total_time /* [n_files] */,
                         int32_t* d_scratch, int64_t scratch_words, void* stream);

/* ---- note velocities: from the float32 log-mel [n_rows, n_mel] the frontend has written on the device.  Nothing is
 * measured from the samples and no transcendental function runs on the device: every step is a gather, a float64 add in
 * a stated order, one float64 division, a max, a rank selection or a comparison with a host-built table, so the result
 * equals the numpy statement bit for bit (mt3_amd/velocity.py, levels_reference / velocities_reference).  Two ops over
 * one file table; a job calls the first, then the second on its levels.
 * FILES   file f owns the log-mel rows row0 .. row0 + n_frames - 1 (n_frames: its valid frames; the zero rows of a short
 *   last segment and the neighbouring files' rows are never read) and the notes first .. first + n_notes - 1, the
 *   n_pitched pitched ones first, then the drums: the file's two GROUPS.  The host sorts; the ops take sorted columns.
 * NOTES   frame = floor(onset * frames per second), computed on the host in float64, int32; key = the pitch, or
 *   MT3_VELOCITY_KEYS - 1 = 128 for a drum.
 * TABLE   CSR over the 129 keys: bin_first int32 [130], bins int32 [n_bins]; row k lists the mel bins whose values make
 *   key k's level, duplicates allowed (mt3_amd/velocity.py, harmonic_bins: per pitch the strongest mel bin of each of its
 *   first harmonics; the drum row: every 8th bin).  The host copy is what is checked; the device copy holds the same
 *   values and is what the kernel reads -- it still treats an offset outside [0, n_bins] as an empty row and a bin outside
 *   [0, n_mel) as NaN, so a device copy that differs gives other levels, never a read outside the buffers.
 * mt3_op_note_levels  THE LEVEL of a note (frame t, key k) of file f: over the frames g = t .. t + window - 1 cut to
 *   [0, n_frames), s(g) = (the float64 sum of logmel[row0 + g][b] over the bins b of row k, added left to right in table
 *   order) / their count; the level is the largest s(g), frames whose s is NaN skipped (fmax).  d_level is NaN -- the note
 *   is UNMEASURED -- when t is outside [0, n_frames), row k is empty, k is outside 0 .. 128, or every s was NaN.
 *   WORK  a note's window frames are spread over 8 neighbouring lanes of a wave (lane j: frames t + j, t + j + 8, ...),
 *   each lane gathers its frame's bins from one row, and the 8 lanes reduce the max with three cross-lane moves; 32 notes
 *   per workgroup, the grid follows the notes, 64 files per launch (their table rides in the kernel arguments).
 * mt3_op_level_velocities  per (file, group), n = its measured notes: THE ANCHOR is the member level of ascending rank
 *   floor(quantile * (n - 1)) (float64), NaN for n = 0.  d = level - anchor (float64);
 *   velocity = 1 + #{i in 0 .. 125 : d >= d_th[i]}, d_th ASCENDING (th[v] = gamma * ln((v - 0.5) / anchor_velocity) for
 *   v = 2 .. 127, built on the host).  An unmeasured note keeps d_velocity_in.  d_anchor, d_measured: [n_files][2].
 *   WORK  one workgroup of 256 lanes per (file, group); the rank by a radix select on the order-preserving 64-bit image
 *   of the level, 8 passes of 8 bits: a 256-bin histogram in LDS by integer atomics over a strided loop (a group of any
 *   size), a sum-scan over the bins; then a binary search in d_th per note.  Integer counts: the same input gives the same
 *   bits on every run.  No atomics on global memory.
 * SAFETY  every index comes from the file table and the host table, checked below, or is guarded in the kernel; note
 *   columns of any content give unspecified levels, but no read or write leaves the file's own rows and notes.
 * MT3_ERR_INVALID, before any device work: window outside 1 .. 64; n_mel outside 1 .. 4096; n_rows, n_notes, n_files or
 *   n_bins negative; a NULL file table with n_files > 0; a file's note range outside [0, n_notes], overlapping the one
 *   before it or out of order; n_pitched outside 0 .. n_notes; a file's rows outside [0, n_rows]; a NULL table; a
 *   bin_first that does not rise from 0 to n_bins; a bin outside [0, n_mel); NULL columns with n_notes > 0, a NULL
 *   log-mel with n_rows > 0, NULL thresholds or outputs; quantile outside [0, 1] (NaN included).  n_files == 0 is MT3_OK
 *   and launches nothing. */
#define MT3_VELOCITY_KEYS 129
#define MT3_VELOCITY_THRESHOLDS 126
#define MT3_VELOCITY_MAX_WINDOW 64
#define MT3_VELOCITY_MAX_MEL 4096

typedef struct mt3_velocity_file {
  int64_t first;                      /* the file's first note in the columns */
  int64_t row0;                       /* the file's first row in the log-mel */
  int32_t n_notes;
  int32_t n_pitched;                  /* group 0: notes first .. first + n_pitched - 1; group 1 (drums): the rest */
  int32_t n_frames;                   /* the file's valid rows */
  int32_t reserved;
} mt3_velocity_file;

int mt3_op_note_levels(const float* d_logmel, int64_t n_rows, int32_t n_mel,
                       const mt3_velocity_file* h_files /* [n_files] */, int32_t n_files, const int32_t* d_frame,
                       const int32_t* d_key, int64_t n_notes, const int32_t* h_bin_first /* [130] */,
                       const int32_t* h_bins /* [n_bins] */, const int32_t* d_bin_first, const int32_t* d_bins,
                       int32_t n_bins, int32_t window, double* d_level /* [n_notes] */, void* stream);

int mt3_op_level_velocities(const double* d_level, int64_t n_notes, const mt3_velocity_file* h_files /* [n_files] */,
                            int32_t n_files, double quantile, const double* d_th /* [126] */,
                            const int32_t* d_velocity_in, int32_t* d_velocity, double* d_anchor /* [n_files][2] */,
                            int32_t* d_measured /* [n_files][2] */, void* stream);

/* ---- beats: the beats of every file of a job from its own onsets, and the notes of a job on the beats' grid.  The
 * dynamic-programming beat tracker of Ellis (2007) restated in integers: after the host has packed the onset frames no
 * float is left, so any summation order and integer atomics give the same bits as the numpy statement
 * (mt3_amd/beats.py, track_reference).
 * THE RULE, per file of F = n_frames frames at MT3_BEATS_FPS frames per second:
 *   FRAMES    d_frames holds one int32 per note, f = floor(start_time * fps + 0.5), in any order; F = max f + 1.  A frame
 *     outside [0, F) is skipped.  F == 0: no beats, period 0.
 *   ENVELOPE  n[t] = the onsets in frame t, at most 255;  E[t] = n[t-1] + 2 n[t] + n[t+1] for t in 0 .. F-1, zeros outside;
 *     peak = max E;  S[t] = (E[t] << 16) / peak.  peak == 0: no beats, period 0.
 *   PERIOD    A[l] = sum over t of E[t] * E[t + l] (int64) for l in MT3_BEATS_LAG_MIN .. MT3_BEATS_LAG_MAX; p = the LOWEST l
 *     of maximal A[l] * W[l], W = d_prior [176] int64 (a tempo prior, <= 2^16; F < 2^20 keeps the product below 2^63).
 *     Every product 0: no beats, period 0.
 *   PATH      lo = (p + 1) / 2, hi = 2 p, pen[l] = d_penalties[(p - LAG_MIN) * MT3_BEATS_PEN_STRIDE + l - lo] for l in lo .. hi:
 *       best(t) = max over l in lo .. hi with t - l >= 0 of (C[t - l] - pen[l]), the LOWEST l on equal values;
 *       C[t] = S[t] + max(best(t), 0);  back[t] = that l, or 0 when best(t) <= 0 or no l is admissible.
 *   BEATS     the path ends at the LOWEST t of maximal C[t] among the last p frames (all of them when F <= p) and is read
 *     back through `back` until back[t] == 0; the beats are those frames in ascending order, score = C[end].
 * Both tables are built by the host in float64 and rounded there (mt3_amd/beats.py: prior_table, penalty_table); penalties
 * must be >= 0 and below 2^40.
 * h_files [n_files]: per file its notes in d_frames (first, n_notes), its n_frames, frame0 = where its rows start in the
 * per-frame scratch and beat0 = where its beats start in d_beats, which gives it MT3_BEATS_CAPACITY(n_frames) slots (steps
 * of a path are >= 13 frames).  The three kinds of range each lie in increasing order and without overlap.
 * d_rows: 2 * total_frames int32 of scratch (the op zeroes what it needs), d_back: total_frames uint16 of scratch.
 * d_period, d_n_beats [n_files] int32, d_score [n_files] int64, d_beats [total_beats] int32: a file's n_beats beat frames
 * from its beat0 on, the rest of its slots is not written.
 * Work: one workgroup of 256 lanes per file, 32 files per launch (their table rides in the kernel arguments), the launches
 * one after the other on `stream`; the layout is described in mt3_amd/csrc/beats.hip.
 * MT3_ERR_INVALID, before any device work: a NULL pointer that the job needs; a negative count; tables that do not hold
 * 176 and 176 * 301 entries; n_frames outside 0 .. 2^20 - 1; a note, frame or beat range outside its array, overlapping
 * the one before it or out of order.  n_files == 0 is MT3_OK and does nothing.
 *
 * mt3_op_snap_notes: every note time of a job on the grid of `subdivisions` steps per beat, in float64, every operation
 * rounded once (no fused multiply-add), so the result is numpy's bit for bit (mt3_amd/beats.py, snap_reference).  Per
 * file: its beat frames (strictly ascending int32, n_beats of them from beat0 on in d_beat_frames), b = frame / fps.  With
 * fewer than 2 beats the times are copied.  For a time t: i = the last beat at or before t, kept within 0 .. n_beats - 2
 * (the grid of the first / last interval continues outside the beats); d = b[i+1] - b[i];
 * k = ceil(((t - b[i]) / d) * subdivisions - 0.5): the nearest step, the lower one on a tie;
 * point(i, k) = b[i+1] when k == subdivisions, else b[i] + (k / subdivisions) * d.  out_start = point of the start,
 * out_end = point of the end, or, when that would not exceed out_start, point(i, k + 1) of the START: one grid step.
 * MT3_ERR_INVALID, before any device work: a NULL pointer that the job needs; a negative count; subdivisions outside
 * 1 .. MT3_BEATS_MAX_SUBDIVISIONS; a note or beat range outside its array, overlapping the one before it or out of
 * order.  n_files == 0 is MT3_OK and does nothing. */
#define MT3_BEATS_FPS 100
#define MT3_BEATS_LAG_MIN 25
#define MT3_BEATS_LAG_MAX 200
#define MT3_BEATS_PEN_STRIDE 301
#define MT3_BEATS_MAX_FRAMES (1 << 20)
#define MT3_BEATS_TILE 1024
#define MT3_BEATS_MAX_SUBDIVISIONS 48
#define MT3_BEATS_CAPACITY(n_frames) ((int64_t)(n_frames) / 13 + 2)

typedef struct mt3_beats_file {
  int64_t first;                      /* the file's first note in d_frames */
  int64_t frame0;                     /* the file's first word in each per-frame scratch row */
  int64_t beat0;                      /* the file's first slot in d_beats */
  int32_t n_notes;
  int32_t n_frames;
} mt3_beats_file;

typedef struct mt3_snap_file {
  int64_t first;                      /* the file's first note in the columns */
  int64_t beat0;                      /* the file's first beat in d_beat_frames */
  int32_t n_notes;
  int32_t n_beats;
} mt3_snap_file;

int mt3_op_track_beats(const int32_t* d_frames /* [n_notes] */, int64_t n_notes,
                       const mt3_beats_file* h_files /* [n_files] */, int32_t n_files, const int64_t* d_prior /* [176] */,
                       int32_t n_prior, const int64_t* d_penalties /* [176][301] */, int32_t n_penalties,
                       int32_t* d_rows /* [2][total_frames] */, uint16_t* d_back /* [total_frames] */, int64_t total_frames,
                       int32_t* d_period /* [n_files] */, int32_t* d_n_beats /* [n_files] */,
                       int32_t* d_beats /* [total_beats] */, int64_t total_beats, int64_t* d_score /* [n_files] */,
                       void* stream);

int mt3_op_snap_notes(const double* d_start /* [n_notes] */, const double* d_end /* [n_notes] */, int64_t n_notes,
                      const int32_t* d_beat_frames /* [n_beat_frames] */, int64_t n_beat_frames,
                      const mt3_snap_file* h_files /* [n_files] */, int32_t n_files, int32_t subdivisions,
                      double* d_out_start /* [n_notes] */, double* d_out_end /* [n_notes] */, void* stream);

/* ---- score-to-audio synchronisation: chroma features of a recording (from the log-mel the frontend has written) and of
 * a score (from its notes), and the dynamic-time-warping path between the two.  Integer or fixed-order arithmetic
 * throughout, so each op equals its numpy statement bit for bit (mt3_amd/sync.py: logmel_chroma_reference,
 * note_chroma_reference, paths_reference).  Three ops over ONE file table; a job calls the two chroma ops, then the path op
 * on their outputs.  Max-log chroma is this project's own feature; it claims parity with no library.
 * FILES   h_files [n_files] is what is checked; d_files is the same records on the device and what the kernels read (the
 *   one upload of a job carries it), so each op is ONE launch (the path op), or one launch per kernel, whatever n_files is.
 *   A device copy that differs from the checked one is the caller's error, as a wrong pointer is.  File f owns the log-mel
 *   rows row0 .. row0 + n_frames - 1, the notes first .. first + n_notes - 1, the audio features a0 .. a0 + n - 1 of d_a, the
 *   score features s0 .. s0 + m - 1 of d_s, the path slots path0 .. path0 + MT3_SYNC_PATH_CAPACITY(n, m) - 1 and the
 *   workspace words work0 .. work0 + mt3s_workspace_words(n, m) - 1.  Each kind of range lies in increasing order and
 *   without overlap.  An op checks and reads only the fields it names.
 * mt3_op_logmel_chroma  (row0, n_frames, a0, n; n == ceil(n_frames / pool))  d_a [total_a][12] uint8.  d_bins int8
 *   [n_mel]: each mel bin's pitch class 0 .. 11, anything else: unused (the host builds it: mt3_amd/sync.py, chroma_bins).
 *   Feature frame i of a file covers its rows i * pool .. min((i + 1) * pool, n_frames) - 1:
 *     v[c] = the largest log-mel value at the bins of class c over those rows, NaN values skipped; a class with no bin or
 *            nothing but NaN is UNMEASURED;  mx = the largest measured v[c];
 *     q[c] = clamp(floor(((v[c] - mx) + range) * scale)) in float32, each of the three operations rounded on its own
 *            (no fused multiply-add), scale = (float)(255.0 / (double)range) from the host; clamp(t) = 255 for t >= 255,
 *            (int)t for 0 <= t < 255, else 0 (NaN among them); an unmeasured class gives 0.
 *     The frame is SILENT, twelve zeros, unless mx >= floor (nothing measured: silent).  No transcendental function runs.
 *   WORK  a wave per feature frame, four to a workgroup, the grid over the job's feature frames (a frame finds its file
 *   by binary search in d_files).  A lane reads 16 bytes of each row (four bins; 64 lanes: 1 KiB, contiguous) when n_mel
 *   is a multiple of 4 and the log-mel is 16-byte aligned, else single floats 256 bytes per wave; it folds the rows per
 *   bin, then its bins into twelve registers, and six xor moves per class reduce across the wave.  Lanes 0 .. 11 store.
 * mt3_op_note_chroma  (first, n_notes, s0, m)  d_s [total_s][12] uint8.  Note columns (int32): d_j0, d_j1, d_pitch; the
 *   host computes j0 = floor(start * fps), j1 = max(j0 + 1, floor(end * fps)) in float64 and m = the largest j1 of the file
 *   (0 without notes).  For h < n_harmonics the note adds h_weights[h] (0 .. 255) to class (pitch + MT3_SYNC_OFFSETS[h])
 *   mod 12 over the frames j0 .. j1 - 1;  s[j][c] = min(255, sum).  A note with pitch outside 0 .. 127, j0 outside [0, m)
 *   or j1 outside (j0, m] adds nothing.
 *   WORK  the piano roll's idiom: the op zeroes 12 * total_s int32 words of d_scratch (file f's twelve rows of m words
 *   from 12 * s0 on), a lane per note makes two return-less integer atomic adds per harmonic (+w at j0, -w at j1 < m),
 *   one workgroup per (file, class) add-scans its row and stores the clipped bytes.  Integer sums: any order, same bits.
 * mt3_op_sync_paths  (a0, n, s0, m, path0)  cost(i, j) = sum over c of |a[i][c] - s[j][c]| (<= 3060), all int32:
 *     D[0][0] = cost(0, 0);  D[i][j] = cost(i, j) + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) over the predecessors that
 *     exist, the FIRST of equal values in that order;  the path runs from (n-1, m-1) back to (0, 0) along those choices.
 *   d_path_i, d_path_j: the path in FORWARD order from path0 on, d_path_len [n_files] its length (<= n + m - 1),
 *   d_total [n_files] = D[n-1][m-1].  n == 0 or m == 0: length 0, total 0.  n, m <= MT3_SYNC_MAX_FRAMES keeps every D below
 *   2^31; n * m <= MT3_SYNC_MAX_CELLS bounds the workspace -- there is no band constraint.
 *   WORK  ONE workgroup of MT3_SYNC_LANES lanes per file, the files side by side in one launch; no workgroup ever waits for
 *   another.  The skewed column-strip form: lane l owns the MT3_SYNC_STRIP columns of strip l and keeps their row of D and
 *   their twelve-byte score features in registers; at step t it computes row t - l of its strip (twelve absolute
 *   differences are three sad_u8), takes the strip's left boundary from lane l - 1 (a cross-lane move inside a wave, one
 *   LDS word between waves, one barrier per step) and stores the strip's 16 two-bit choices as ONE dword, in step order so
 *   that a wave's stores are contiguous.  More than MT3_SYNC_LANES strips: panels of that many, the boundary column
 *   between two panels (n int32) in the workspace.  The read-back is one lane following dependent loads, as in
 *   mt3_op_align_paths (a move to the left inside a strip reuses the dword it holds); it fills the file's slots from the
 *   back, and the workgroup then moves the path to the front.
 *   d_workspace: int32 words, 4-byte aligned; a file's words are never read before they are written, so nothing needs
 *   clearing.  mt3_sync_workspace_bytes(h_files, n_files): the bytes the files need back to back (work0 = the running
 *   sum of mt3s_workspace_words); -1 (and mt3_last_error) for a NULL table or an n or m the path op would refuse.
 * MT3_ERR_INVALID, before any device work: n_files negative; a NULL table (host or device) with n_files > 0; a count of a
 *   file negative; pool outside 1 .. MT3_SYNC_MAX_POOL; n_mel outside 1 .. 4096; range not finite and > 0; floor NaN;
 *   n != ceil(n_frames / pool); n_harmonics outside 1 .. MT3_SYNC_HARMONICS, a weight outside 0 .. 255; n or m above
 *   MT3_SYNC_MAX_FRAMES; n * m above MT3_SYNC_MAX_CELLS; a range outside its array, overlapping the one before it or out
 *   of order; a NULL or misaligned (4 bytes) array the job needs; a NULL or short workspace.  n_files == 0 is MT3_OK and
 *   launches nothing. */
#define MT3_SYNC_CLASSES 12
#define MT3_SYNC_MAX_POOL 16
#define MT3_SYNC_HARMONICS 6
#define MT3_SYNC_MAX_FRAMES (1 << 18)
#define MT3_SYNC_MAX_CELLS ((int64_t)1 << 31)
#define MT3_SYNC_LANES 1024
#define MT3_SYNC_STRIP 16
#define MT3_SYNC_PATH_CAPACITY(n, m) ((n) > 0 && (m) > 0 ? (int64_t)(n) + (int64_t)(m) - 1 : (int64_t)0)

typedef struct mt3_sync_file {
  int64_t row0;                       /* the file's first row in the log-mel */
  int64_t first;                      /* the file's first note in the note columns */
  int64_t a0;                         /* the file's first audio feature frame in d_a */
  int64_t s0;                         /* the file's first score feature frame in d_s */
  int64_t path0;                      /* the file's first slot in d_path_i / d_path_j */
  int64_t work0;                      /* the file's first int32 word in d_workspace */
  int32_t n_frames;                   /* the file's valid log-mel rows */
  int32_t n_notes;
  int32_t n;                          /* audio feature frames */
  int32_t m;                          /* score feature frames */
} mt3_sync_file;

/* the semitone offsets of the harmonics 1 .. 6 of a note: 0, 12, 19, 24, 28, 31 */
MT3_RULE_FN int32_t mt3s_offset(int32_t h) {
  return h == 0 ? 0 : h == 1 ? 12 : h == 2 ? 19 : h == 3 ? 24 : h == 4 ? 28 : 31;
}

/* int32 words of workspace of one file: the choices of every panel in step order, then the boundary column */
MT3_RULE_FN int64_t mt3s_workspace_words(int32_t n, int32_t m) {
  if (n <= 0 || m <= 0) return 0;
  const int64_t strips = ((int64_t)m + MT3_SYNC_STRIP - 1) / MT3_SYNC_STRIP;
  const int64_t full = strips / MT3_SYNC_LANES, rest = strips % MT3_SYNC_LANES;
  return full * ((int64_t)n + MT3_SYNC_LANES - 1) * MT3_SYNC_LANES + (rest ? ((int64_t)n + rest - 1) * rest : 0) + n;
}

int64_t mt3_sync_workspace_bytes(const mt3_sync_file* h_files /* [n_files] */, int32_t n_files);

int mt3_op_logmel_chroma(const float* d_logmel, int64_t n_rows, int32_t n_mel, const mt3_sync_file* h_files /* [n_files] */,
                         const mt3_sync_file* d_files, int32_t n_files, const int8_t* d_bins /* [n_mel] */, int32_t pool,
                         float range, float floor, uint8_t* d_a /* [total_a][12] */, int64_t total_a, void* stream);

int mt3_op_note_chroma(const int32_t* d_j0, const int32_t* d_j1, const int32_t* d_pitch, int64_t n_notes,
                       const mt3_sync_file* h_files /* [n_files] */, const mt3_sync_file* d_files, int32_t n_files,
                       const int32_t* h_weights /* [n_harmonics] */, int32_t n_harmonics,
                       int32_t* d_scratch /* [12 * total_s] */, uint8_t* d_s /* [total_s][12] */, int64_t total_s,
                       void* stream);

int mt3_op_sync_paths(const uint8_t* d_a /* [total_a][12] */, int64_t total_a, const uint8_t* d_s /* [total_s][12] */,
                      int64_t total_s, const mt3_sync_file* h_files /* [n_files] */, const mt3_sync_file* d_files,
                      int32_t n_files, void* d_workspace, int64_t workspace_bytes, int32_t* d_path_i, int32_t* d_path_j,
                      int64_t total_path, int32_t* d_path_len /* [n_files] */, int32_t* d_total /* [n_files] */,
                      void* stream);

/* ---- harmony: the key, the chord of every beat, the bar length and the downbeat phase of every file of a job, from its
 * notes and its beat frames.  Integer arithmetic throughout, so any order of the sums and integer atomics give the bits of
 * the numpy statement (mt3_amd/harmony.py, analyze_reference).  `/` below floors, also for a negative dividend; argmax takes
 * the LOWEST index unless said otherwise.  The feature claims parity with no library.
 * NOTES   three int32 columns: d_start = s, d_end = e (frames at MT3_BEATS_FPS; the host rounds, e >= s + 1) and d_key =
 *   pitch + 256 * is_drum.  A note with s < 0 or e <= s adds nothing anywhere.  h_key is the host's copy of d_key: what is
 *   checked.  h_beats / d_beats likewise: per file n_beats strictly ascending frames b[0 .. B-1] in 0 .. 2^20 - 1.
 * THE RULE, per file:
 *   INTERVALS  B < 2: no chords, beats_per_bar 0, downbeat -1, chord_score 0; the key is still found.  Else interval i is
 *     [b[i], b[i+1]) for i < B - 1, the last [b[B-1], 2 b[B-1] - b[B-2]); len[i] its length.  A note is clipped to them.
 *   ROLL     R[i][p] = the frames the non-drum notes of pitch p share with interval i, summed over the notes (int32: n_notes
 *     times the longest interval stays below 2^31).  H[i][c] = sum of R[i][p] over p % 12 == c, tot[i] = sum of H[i].
 *     low[i] = the lowest p with 4 R[i][p] >= len[i], else -1;  bass[i] = low[i] % 12, else -1.
 *   KEY      D[c] = the sum of e - s over the non-drum notes of class c (int64);  key_score[k] = sum over c of
 *     K[k][c] * D[c], K = d_profiles int32 [24][12] (the host builds it: harmony.py, key_profiles);  key = the lowest k of
 *     maximal score, -1 when every D is 0.
 *   CHORDS   MT3_HARMONY_STATES = 25 states: 0 = N, 1 + 2 r + q = the major (q = 0: r, r + 4, r + 7) or minor (q = 1: r,
 *     r + 3, r + 7) triad on r.  E[i][k] = sum over c of w_k(c) H[i][c] + (H[i][r] if bass[i] == r), w = +2 on a chord tone,
 *     -1 elsewhere, E[i][0] = 0;  Q[i][k] = (E[i][k] * 256) / max(tot[i], 1), -256 .. 768.
 *       V[0][k] = Q[0][k];  V[i][k] = Q[i][k] + max(V[i-1][k], M - change_penalty), M = the largest V[i-1][.] at its lowest
 *       index j, staying on equal values;  back[i][k] = k or j.
 *     The path ends at the lowest k of maximal V[B-1] and is read back: chords int8 [B];  chord_score = V[B-1][end]
 *     (|V| <= 768 B + 2^20 < 2^30: int32).
 *   METER    change[i] = (i > 0 and chords[i] != chords[i-1]);  on[i] = min(the notes, drums too, with |s - b[i]| <=
 *     MT3_HARMONY_ONSET_WINDOW, 255);  struck[i] = some non-drum note with |s - b[i]| <= the window has pitch low[i];
 *     a[i] = onset_weight on[i] + change_weight change[i] + bass_weight struck[i].  For m in 2, 3, 4 with B >= 2 m and f in
 *     0 .. m - 1: num = the sum of a[i] over i % m == f, cnt = the number of such i,
 *       score(m, f) = (num << 16) / cnt - ((sum of a - num) << 16) / (B - cnt)   (int64)
 *     (beats_per_bar, downbeat) = the (m, f) of maximal score, the lowest m and then f on ties; (0, -1) when no m is
 *     admissible or no score is > 0.
 * FILES   h_files [n_files] is what is checked, d_files the same records on the device and what the kernel reads: the
 *   notes first .. first + n_notes - 1 and the beats beat0 .. beat0 + n_beats - 1, each kind in increasing order and
 *   without overlap.  A file's chords lie at d_chords + beat0 (not written when n_beats < 2).
 * OUT     d_key_scores int64 [n_files][24];  d_info int32 [n_files][4] = key, chord_score, beats_per_bar, downbeat;
 *   d_chords int8 [n_beats].  d_workspace: MT3_HARMONY_WORKSPACE_BYTES_PER_BEAT * n_beats bytes, 2-byte aligned; nothing
 *   in it is read before it is written, so nothing needs clearing.
 * WORK    ONE launch: a workgroup of MT3_HARMONY_NOTE_TILE lanes per file, no workgroup waits for another; the beats go
 *   through LDS in tiles of MT3_HARMONY_BEAT_TILE intervals (mt3_amd/csrc/harmony.hip).
 * MT3_ERR_INVALID, before any device work: n_files, n_notes or n_beats negative; a NULL pointer that the job needs; a
 *   table that does not hold 24 * 12 entries; change_penalty outside 0 .. MT3_HARMONY_MAX_CHANGE_PENALTY, a weight outside
 *   0 .. MT3_HARMONY_MAX_WEIGHT; a note or beat range outside its array, overlapping the one before it or out of order; a
 *   key whose pitch is outside 0 .. 127 or that has bits above the drum flag; beat frames that do not ascend strictly
 *   inside 0 .. 2^20 - 1; n_notes times the longest interval at or above 2^31; a short or misaligned workspace.
 *   n_files == 0 is MT3_OK and launches nothing. */
#define MT3_HARMONY_STATES 25
#define MT3_HARMONY_KEYS 24
#define MT3_HARMONY_BEAT_TILE 32
#define MT3_HARMONY_NOTE_TILE 256
#define MT3_HARMONY_ONSET_WINDOW 3
#define MT3_HARMONY_MAX_CHANGE_PENALTY (1 << 20)
#define MT3_HARMONY_MAX_WEIGHT 255
#define MT3_HARMONY_WORKSPACE_BYTES_PER_BEAT 27

typedef struct mt3_harmony_file {
  int64_t first;                      /* the file's first note in the note columns */
  int64_t beat0;                      /* the file's first beat in d_beats, and its first chord in d_chords */
  int32_t n_notes;
  int32_t n_beats;
} mt3_harmony_file;

int mt3_op_analyze_harmony(const int32_t* d_start, const int32_t* d_end, const int32_t* d_key,
                           const int32_t* h_key /* [n_notes] */, int64_t n_notes, const int32_t* d_beats,
                           const int32_t* h_beats /* [n_beats] */, int64_t n_beats,
                           const mt3_harmony_file* h_files /* [n_files] */, const mt3_harmony_file* d_files,
                           int32_t n_files, const int32_t* d_profiles /* [24][12] */, int32_t n_profiles,
                           int32_t change_penalty, int32_t onset_weight, int32_t change_weight, int32_t bass_weight,
                           void* d_workspace, int64_t workspace_bytes, int64_t* d_key_scores /* [n_files][24] */,
                           int32_t* d_info /* [n_files][4] */, int8_t* d_chords /* [n_beats] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MT3_HIP_H_ */
