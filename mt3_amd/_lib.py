"""ctypes binding of libmt3hip.so (the C ABI in include/mt3_hip.h).

The library is the product; there is NO Python/CPU fallback: if it is missing or a
call fails, the caller gets an exception (`Mt3Error`).  `import torch` happens
first on purpose so that the library binds to the same HIP runtime
(libamdhip64.so.7) that owns torch's device allocations.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmt3hip.so")

MT3_OK, MT3_ERR_INVALID, MT3_ERR_HIP, MT3_ERR_CAPACITY, MT3_ERR_MISSING = 0, -1, -2, -3, -4
MT3_BF16, MT3_F32, MT3_FP8_E4M3 = 0, 1, 2
EPI_STORE, EPI_RESID, EPI_GEGLU, EPI_POS, EPI_F32, EPI_HEADS = range(6)
DECODE_NO_GRAPH, DECODE_EARLY_EXIT, DECODE_BEAM1, DECODE_SINGLE_STREAM, DECODE_ASYNC = 1, 2, 4, 8, 16
(OPT_SINGLE_RESIDUAL_STREAM, OPT_SEPARATE_PROJECTIONS, OPT_ENCODER_SINGLE_RESIDUAL_STREAM,
 OPT_SEPARATE_QKV_PROJECTION, OPT_NO_ROW_GROUPS) = 1, 2, 4, 8, 16              # mt3_engine_config.options
OPT_ENCODER_F32_MFMA = 32
OPT_SPIN_WAITS = 64
# include/mt3_hip_debug.h (measurement / fault injection; not the product ABI)
DEBUG_SKIP_SELF_ATTN, DEBUG_SKIP_CROSS_ATTN = 1, 2
(STATUS_GRAPH_FALLBACKS, STATUS_LAST_DECODE_USED_GRAPH, STATUS_RESIDUAL_SPLIT, STATUS_KV_FP8, STATUS_Q_FOLD,
 STATUS_DENSE_FP8, STATUS_QKV_FOLD, STATUS_LAST_DECODE_GROUPS, STATUS_PARTITION_FALLBACKS,
 STATUS_LAST_DECODE_COMPACTIONS, STATUS_LAST_DECODE_FORKS, STATUS_SCORE_CHUNKS, STATUS_TOKEN_MASKS,
 STATUS_PROMPTS, STATUS_TOKEN_GRAMMAR, STATUS_SAMPLING, STATUS_NOTE_GRAMMAR, STATUS_SCORE_ENCODER_PASSES) = range(18)
SAMPLING_MAX_TOP_K, SAMPLING_MAX_VOCAB = 256, 2048      # mt3_engine_set_sampling
(MT3_PCM_U8, MT3_PCM_S16, MT3_PCM_S24, MT3_PCM_S32, MT3_PCM_F32, MT3_PCM_F64) = range(6)     # mt3_pcm_decode formats
PCM_MAX_CHANNELS = 7
MAX_BEAMS = 8                                  # mt3_engine_decode_beams: 1 <= num_beams <= 8
EV_SHIFT, EV_PITCH, EV_VELOCITY, EV_TIE, EV_PROGRAM, EV_DRUM = range(6)
EVENT_TYPE_NAMES = ("shift", "pitch", "velocity", "tie", "program", "drum")
SPEC_ONSETS, SPEC_NOTES, SPEC_TIES = range(3)
TIE_DROP_REDUNDANT_PROGRAMS = 1                # mt3_op_tie_prompts flags
PIANOROLL_PITCHES, PIANOROLL_MIN_NOTE_SECONDS = 128, 0.05      # mt3_op_pianoroll
RENDER_TILE, RENDER_MAX_SAMPLE_RATE, RENDER_MAX_SAMPLES = 1024, 384000, 1 << 40      # mt3_op_render_notes
RENDER_RELEASE_SECONDS, RENDER_DRUM_SECONDS = 0.04, 0.15
NOTE_MATCH_MAX_RULES, NOTE_MATCH_NO_OFFSET = 16, -1.0          # mt3_op_match_notes
GRANULARITY_FULL, GRANULARITY_MIDI_CLASS, GRANULARITY_FLAT = range(3)      # mt3_codec_tokenize_rule
GRANULARITIES = {"full": GRANULARITY_FULL, "midi_class": GRANULARITY_MIDI_CLASS, "flat": GRANULARITY_FLAT}
TOKENIZE_MAX_STRIDE = 1 << 20                  # mt3_op_tokenize_notes
ALIGN_MAX_SHIFTS = 64                          # mt3_op_align_paths
CONSENSUS_MAX_VOTERS, CONSENSUS_TILE, CONSENSUS_SCRATCH_WORDS_PER_NOTE = 64, 256, 4      # mt3_op_note_consensus
NOTE_PREP_SUSTAIN, NOTE_PREP_TRIM, NOTE_PREP_TILE = 0, 1, 256                              # mt3_op_prepare_notes
VELOCITY_KEYS, VELOCITY_THRESHOLDS, VELOCITY_MAX_WINDOW, VELOCITY_MAX_MEL = 129, 126, 64, 4096   # mt3_op_note_levels
BEATS_FPS, BEATS_LAG_MIN, BEATS_LAG_MAX, BEATS_PEN_STRIDE = 100, 25, 200, 301                    # mt3_op_track_beats
BEATS_MAX_FRAMES, BEATS_TILE, BEATS_MAX_SUBDIVISIONS = 1 << 20, 1024, 48
SYNC_CLASSES, SYNC_MAX_POOL, SYNC_HARMONICS, SYNC_LANES, SYNC_STRIP = 12, 16, 6, 1024, 16        # mt3_op_sync_paths
SYNC_MAX_FRAMES, SYNC_MAX_CELLS = 1 << 18, 1 << 31
HARMONY_STATES, HARMONY_KEYS, HARMONY_BEAT_TILE, HARMONY_NOTE_TILE = 25, 24, 32, 256                # mt3_op_analyze_harmony
HARMONY_ONSET_WINDOW = 3
HARMONY_MAX_CHANGE_PENALTY, HARMONY_MAX_WEIGHT, HARMONY_WORKSPACE_BYTES_PER_BEAT = 1 << 20, 255, 27


class Mt3Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmt3hip error %d: %s" % (code, msg))
        self.code = code


class FrontendConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("hop_width", C.c_int32), ("num_mel_bins", C.c_int32),
                ("fft_size", C.c_int32), ("lo_hz", C.c_float), ("hi_hz", C.c_float), ("table_dtype", C.c_int32)]


class EngineConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "vocab_size", "emb_dim", "num_heads", "head_dim", "mlp_dim", "num_encoder_layers",
        "num_decoder_layers", "input_depth", "input_length", "max_decode_len", "max_batch", "compute_dtype",
        "decode_chains", "kv_cache_dtype", "dense_dtype", "options")]


class TranscribeStats(C.Structure):            # mt3_transcribe_stats
    _fields_ = [(n, C.c_int32) for n in ("slots", "groups", "steps_run", "polls", "refills", "starved_polls",
                                         "encoder_chunks", "compactions", "used_graph")] + [("reserved", C.c_int32 * 7)]


class EventRange(C.Structure):
    _fields_ = [("type", C.c_int32), ("min_value", C.c_int32), ("max_value", C.c_int32)]


class CodecDesc(C.Structure):
    _fields_ = [("steps_per_second", C.c_double), ("num_ranges", C.c_int32), ("ranges", EventRange * 8)]


class TokenGrammar(C.Structure):               # mt3_token_grammar
    _fields_ = [(n, C.c_int32) for n in ("shift_first", "shift_count", "max_steps", "tie_id", "program_first",
                                         "program_count", "pitch_first", "pitch_count", "with_ties")]


class NoteGrammar(C.Structure):                # mt3_note_grammar
    _fields_ = [("g", TokenGrammar)] + [(n, C.c_int32) for n in ("velocity_first", "velocity_count", "drum_first",
                                                                  "drum_count")]


class Sampling(C.Structure):                   # mt3_sampling (sizeof 24: seed is 8-byte aligned)
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("seed", C.c_uint64)]


class NoteStruct(C.Structure):
    _fields_ = [("start_time", C.c_double), ("end_time", C.c_double), ("pitch", C.c_int32),
                ("velocity", C.c_int32), ("program", C.c_int32), ("is_drum", C.c_int32),
                ("instrument", C.c_int32), ("reserved", C.c_int32)]


class MatchRule(C.Structure):                  # mt3_match_rule
    _fields_ = [(n, C.c_double) for n in ("onset_tolerance", "pitch_tolerance", "offset_ratio", "offset_min_tolerance")] + \
               [("strict", C.c_int32), ("reserved", C.c_int32)]


class MatchProblem(C.Structure):               # mt3_match_problem
    _fields_ = [("ref0", C.c_int64), ("est0", C.c_int64), ("state0", C.c_int64)] + \
               [(n, C.c_int32) for n in ("n_ref", "n_est", "rule", "reserved")]


class TokenizeRule(C.Structure):               # mt3_tokenize_rule
    _fields_ = [(n, C.c_int32) for n in ("spec", "vocab", "max_shift_steps", "shift_first", "pitch_first",
                                         "velocity_first", "velocity_count", "tie_id", "program_first", "drum_first")] + \
               [("reserved", C.c_int32 * 2), ("program_map", C.c_int32 * 128)]


class TokenizeFile(C.Structure):               # mt3_tokenize_file
    _fields_ = [("event0", C.c_int64)] + [(n, C.c_int32) for n in ("n_events", "row0", "n_rows", "reserved")]


class TokenizeRow(C.Structure):                # mt3_tokenize_row
    _fields_ = [(n, C.c_int32) for n in ("file", "step_lo", "step_hi", "reserved")]


class ConsensusFile(C.Structure):              # mt3_consensus_file
    _fields_ = [("first", C.c_int64)] + [(n, C.c_int32) for n in ("n_notes", "n_voters", "min_votes", "reserved")]


class NotePrepFile(C.Structure):               # mt3_note_prep_file
    _fields_ = [("first", C.c_int64), ("pedal_first", C.c_int64), ("n_notes", C.c_int32), ("n_pedal", C.c_int32),
                ("t_last", C.c_double), ("total_time", C.c_double)]


class VelocityFile(C.Structure):               # mt3_velocity_file
    _fields_ = [("first", C.c_int64), ("row0", C.c_int64)] + \
               [(n, C.c_int32) for n in ("n_notes", "n_pitched", "n_frames", "reserved")]


class BeatsFile(C.Structure):                  # mt3_beats_file
    _fields_ = [("first", C.c_int64), ("frame0", C.c_int64), ("beat0", C.c_int64), ("n_notes", C.c_int32),
                ("n_frames", C.c_int32)]


class SnapFile(C.Structure):                   # mt3_snap_file
    _fields_ = [("first", C.c_int64), ("beat0", C.c_int64), ("n_notes", C.c_int32), ("n_beats", C.c_int32)]


class SyncFile(C.Structure):                   # mt3_sync_file
    _fields_ = [(n, C.c_int64) for n in ("row0", "first", "a0", "s0", "path0", "work0")] + \
               [(n, C.c_int32) for n in ("n_frames", "n_notes", "n", "m")]


class HarmonyFile(C.Structure):                # mt3_harmony_file
    _fields_ = [("first", C.c_int64), ("beat0", C.c_int64), ("n_notes", C.c_int32), ("n_beats", C.c_int32)]


_P = C.c_void_p


# the views of the slot-move test drivers (mt3_op_embed_rows ... mt3_op_beam_stream_init)
class InputRowView(C.Structure):               # mt3_input_row_view
    _fields_ = [("table", _P), ("pos", _P), ("max_pos", C.c_int32), ("dim", C.c_int32), ("y", _P), ("y_ct", _P),
                ("y_ss", _P), ("ew", _P), ("pw", _P), ("q_out", _P), ("q_n", C.c_int32), ("reserved", C.c_int32)]


class SlotStateView(C.Structure):              # mt3_slot_state_view
    _fields_ = [(n, _P) for n in ("done", "slot_row", "slot_seg", "step", "cur_tok", "n_done")]


class StagedCrossView(C.Structure):            # mt3_staged_cross_view
    _fields_ = [(n, C.c_int32) for n in ("n_layers", "src_batch", "src_entry0", "dst_batch")] + \
               [("row_bytes", C.c_uint64), ("sc_bytes", C.c_uint64)] + \
               [(n, C.POINTER(_P)) for n in ("src", "dst", "src_sc", "dst_sc")]


class BeamKView(C.Structure):                  # mt3_beam_k_view
    _fields_ = [(n, C.c_int32) for n in ("k", "elems", "vocab", "hist_stride")] + \
               [(n, _P) for n in ("live", "fin_score", "fin_step", "fin_beam", "hist_par", "hist_tok", "fork_src")]


class DecAttnView(C.Structure):                # mt3_dec_attn_view (mt3_op_decode_attention_ex)
    _fields_ = [("q", _P), ("q_stride", C.c_int32), ("cap", C.c_int32), ("kcache", _P), ("vcache", _P), ("new_k", _P),
                ("new_v", _P), ("kv_stride", C.c_int32), ("n_keys", C.c_int32), ("step", _P), ("out", _P),
                ("B", C.c_int32), ("H", C.c_int32), ("kv_scale", _P), ("q_f32", _P), ("q_ss", _P),
                ("q_ss_n", C.c_int32), ("reserved", C.c_int32), ("done", _P), ("cache_row", _P)]


class GemmView(C.Structure):                   # mt3_gemm_view (mt3_op_gemm_decode)
    _fields_ = [("A", _P), ("Wt", _P), ("out", _P)] + \
               [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldo", "a_is_f32", "norm", "epilogue")] + \
               [("a_ss", _P), ("out_ct", _P), ("out_ss", _P), ("out2", _P)] + \
               [(n, C.c_int32) for n in ("n_split", "ld2", "concurrent", "reserved")]


class ScoreAttnView(C.Structure):              # mt3_score_attn_view (mt3_op_score_attention)
    _fields_ = [("q", _P), ("q_stride", C.c_int32), ("reserved0", C.c_int32), ("k", _P), ("v", _P),
                ("kv_stride", C.c_int32), ("reserved1", C.c_int32), ("kv_bstride", C.c_int64), ("kv_hstride", C.c_int64),
                ("key_tgt", _P), ("out", _P)] + \
               [(n, C.c_int32) for n in ("out_stride", "B", "H", "Lq", "n_keys", "causal")]


# every symbol include/mt3_hip.h and include/mt3_hip_debug.h declare: (name, restype, argtypes)
SIGNATURES = {
    "mt3_last_error": (C.c_char_p, []),
    "mt3_abi_version": (C.c_int, []),
    "mt3_frontend_create": (C.c_int, [C.POINTER(FrontendConfig), C.POINTER(_P)]),
    "mt3_frontend_destroy": (None, [_P]),
    "mt3_frontend_mel_matrix": (C.c_int, [_P, _P, C.POINTER(C.c_int64)]),
    "mt3_frontend_logmel": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "mt3_frontend_logmel_dev": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "mt3_resample_output_length": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "mt3_resampler_create": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "mt3_resampler_destroy": (None, [_P]),
    "mt3_resampler_run": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P]),
    "mt3_pcm_decode": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "mt3_resampler_run_pcm": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "mt3_engine_create": (C.c_int, [C.POINTER(EngineConfig), C.POINTER(_P)]),
    "mt3_engine_destroy": (None, [_P]),
    "mt3_engine_load_weight": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    "mt3_engine_finalize": (C.c_int, [_P]),
    "mt3_engine_device_bytes": (C.c_int64, [_P]),
    "mt3_engine_encode": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "mt3_engine_decode": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_int32), _P]),
    "mt3_engine_decode_wait": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "mt3_engine_decode_beams": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                          C.POINTER(C.c_int32), _P]),
    "mt3_engine_transcribe": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(TranscribeStats), _P]),
    "mt3_engine_transcribe_beams": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                              C.POINTER(TranscribeStats), _P]),
    "mt3_engine_transcribe_draws": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                              C.POINTER(TranscribeStats), _P]),
    "mt3_engine_decode_forced": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "mt3_engine_score": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "mt3_engine_score_segments": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mt3_engine_score_candidates": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mt3_engine_set_token_masks": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32]),
    "mt3_engine_set_prompts": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "mt3_engine_set_token_grammar": (C.c_int, [_P, C.POINTER(TokenGrammar)]),
    "mt3_engine_set_note_grammar": (C.c_int, [_P, C.POINTER(NoteGrammar)]),
    "mt3_note_grammar_table_words": (C.c_int32, [C.POINTER(NoteGrammar)]),
    "mt3_note_grammar_advance": (C.c_int32, [C.POINTER(NoteGrammar), C.c_int32, C.c_int32, _P, C.c_int32]),
    "mt3_note_grammar_allowed": (C.c_int32, [C.POINTER(NoteGrammar), C.c_int32, C.c_int32, _P, C.c_int32]),
    "mt3_note_grammar_check": (C.c_int, [C.POINTER(NoteGrammar), C.c_int32]),
    "mt3_note_grammar_tie_prompt": (C.c_int32, [C.POINTER(NoteGrammar), _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "mt3_op_tie_prompts": (C.c_int, [C.POINTER(NoteGrammar), _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                     _P]),
    "mt3_token_grammar_initial": (C.c_int32, [C.POINTER(TokenGrammar)]),
    "mt3_token_grammar_advance": (C.c_int32, [C.POINTER(TokenGrammar), C.c_int32, C.c_int32]),
    "mt3_token_grammar_allowed": (C.c_int32, [C.POINTER(TokenGrammar), C.c_int32, C.c_int32]),
    "mt3_engine_set_sampling": (C.c_int, [_P, C.POINTER(Sampling), _P, C.c_int32]),
    "mt3_engine_set_sampling_seeds": (C.c_int, [_P, _P, C.c_int32]),
    "mt3_sampling_bits": (C.c_uint32, [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32]),
    "mt3_sampling_gumbel": (C.c_float, [C.c_uint32]),
    "mt3_engine_status": (C.c_int, [_P, C.c_int32]),
    "mt3_debug_engine_decode": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "mt3_debug_engine_transcribe": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                              C.POINTER(TranscribeStats), _P]),
    "mt3_debug_engine_set_score_chunk": (C.c_int, [_P, C.c_int32]),
    "mt3_debug_engine_poison_caches": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "mt3_debug_engine_set_eos_schedule": (C.c_int, [_P, _P, C.c_int32]),
    "mt3_ids_to_tokens": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "mt3_op_score_token_stats": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "mt3_op_score_attention": (C.c_int, [C.c_int32, C.POINTER(ScoreAttnView), _P]),
    "mt3_op_score_embed": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, _P]),
    "mt3_op_score_reduce": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P,
                                      _P]),
    "mt3_op_planes": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P]),
    "mt3_op_gemm_x6": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32,
                                 _P]),
    "mt3_op_encoder_attention_x6": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "mt3_op_rmsnorm": (C.c_int, [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "mt3_op_gemm": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                              C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    "mt3_op_gemm_ex": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "mt3_op_gemm_side": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                   _P, C.c_int32, _P]),
    "mt3_op_gemm_decode": (C.c_int, [C.c_int32, C.POINTER(GemmView), _P]),
    "mt3_op_residual_split": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "mt3_op_encoder_attention": (C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "mt3_op_decode_attention": (C.c_int, [C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32, _P,
                                          C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    "mt3_op_decode_attention_fp8": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32,
                                              _P, C.c_int32, C.c_int32, _P]),
    "mt3_op_decode_attention_ex": (C.c_int, [C.c_int32, C.POINTER(DecAttnView), _P]),
    "mt3_op_kv_quantize_fp8": (C.c_int, [_P, _P, _P, C.c_int32, _P]),
    "mt3_op_beam_search_scripted": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P]),
    "mt3_op_token_steps_scripted": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, _P, _P, _P]),
    "mt3_op_beam_search_masked": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, C.c_int32, _P]),
    "mt3_op_token_steps_masked": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, _P, _P, _P, _P, C.c_int32, _P]),
    "mt3_op_beam_search_prompted": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, C.c_int32, _P,
                                              _P, C.c_int32, _P]),
    "mt3_op_token_steps_prompted": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P]),
    "mt3_op_beam_search_grammar": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, C.c_int32, _P,
                                             _P, C.c_int32, _P, C.POINTER(TokenGrammar), _P]),
    "mt3_op_token_steps_grammar": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P,
                                             C.POINTER(TokenGrammar), _P]),
    "mt3_op_token_steps_sampled": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P,
                                             C.POINTER(TokenGrammar), _P, C.POINTER(Sampling), _P]),
    "mt3_op_token_steps_notes": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P,
                                           C.POINTER(NoteGrammar), _P, C.POINTER(Sampling), _P, _P, _P]),
    "mt3_op_token_steps_seeded": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P,
                                            C.POINTER(NoteGrammar), _P, C.POINTER(Sampling), _P, _P, _P, _P]),
    "mt3_op_beam_search_notes": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, C.c_int32, _P,
                                           _P, C.c_int32, _P, C.POINTER(NoteGrammar), _P, _P, _P]),
    "mt3_op_beam_reorder": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(_P),
                                      C.POINTER(_P), _P, _P, _P, _P, _P]),
    "mt3_op_embed_rows": (C.c_int, [C.POINTER(InputRowView), _P, _P, C.c_int32, _P]),
    "mt3_op_slot_compact": (C.c_int, [C.POINTER(SlotStateView), C.POINTER(InputRowView), _P, C.c_int32, _P, C.c_int32, _P,
                                      _P]),
    "mt3_op_slot_refill": (C.c_int, [C.POINTER(SlotStateView), C.POINTER(InputRowView), _P, C.c_int32, _P, _P, _P,
                                     C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(StagedCrossView), _P, _P]),
    "mt3_op_slot_refill_draws": (C.c_int, [C.POINTER(SlotStateView), C.POINTER(InputRowView), _P, C.c_int32, _P, _P, _P,
                                           C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(StagedCrossView),
                                           C.c_int32, _P, _P]),
    "mt3_op_beam_refill": (C.c_int, [C.POINTER(BeamKView), C.POINTER(SlotStateView), C.POINTER(InputRowView), C.c_int32,
                                     C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(StagedCrossView), _P, _P]),
    "mt3_op_beam_stream_init": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "mt3_host_mx8_quantize": (C.c_int, [_P, C.c_int64, C.c_int64, _P, _P]),
    "mt3_op_mx8_quantize": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "mt3_op_gemm_mx8": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                  _P, _P]),
    "mt3_build_codec": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(CodecDesc)]),
    "mt3_codec_num_classes": (C.c_int, [C.POINTER(CodecDesc)]),
    "mt3_codec_decode_event": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mt3_codec_encode_event": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "mt3_codec_token_mask": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    "mt3_codec_note_grammar": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(NoteGrammar)]),
    "mt3_codec_token_grammar": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(TokenGrammar)]),
    "mt3_notes_decode": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64,
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_double)]),
    "mt3_notes_decode_traced": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_int64,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_double), _P]),
    "mt3_op_pianoroll": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_double, C.c_int32, _P,
                                   C.c_int64, _P]),
    "mt3_op_frame_counts": (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P]),
    "mt3_op_render_notes": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, _P,
                                      C.c_int64, _P, _P]),
    "mt3_note_match_state_words": (C.c_int64, [C.c_int32, C.c_int32]),
    "mt3_op_match_notes": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P,
                                     _P]),
    "mt3_codec_tokenize_rule": (C.c_int, [C.POINTER(CodecDesc), C.c_int32, C.c_int32, C.c_int32, C.POINTER(TokenizeRule)]),
    "mt3_notes_tokenize": (C.c_int, [C.POINTER(TokenizeRule), _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, _P, _P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mt3_op_tokenize_notes": (C.c_int, [C.POINTER(TokenizeRule), _P, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int32, _P,
                                        C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mt3_op_align_paths": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_double, C.c_double, _P, _P, _P, _P]),
    "mt3_op_note_consensus": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, _P, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P,
                                        _P, _P, _P, C.c_int64, _P]),
    "mt3_op_prepare_notes": (C.c_int, [C.c_int32, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int32, _P, _P, _P,
                                       _P, _P, C.c_int64, _P]),
    "mt3_op_note_levels": (C.c_int, [_P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int32,
                                     C.c_int32, _P, _P]),
    "mt3_op_level_velocities": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P]),
    "mt3_op_track_beats": (C.c_int, [_P, C.c_int64, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, _P, _P,
                                     _P, C.c_int64, _P, _P]),
    "mt3_op_snap_notes": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "mt3_sync_workspace_bytes": (C.c_int64, [_P, C.c_int32]),
    "mt3_op_logmel_chroma": (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_float, C.c_float, _P,
                                       C.c_int64, _P]),
    "mt3_op_note_chroma": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int64, _P]),
    "mt3_op_sync_paths": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int32, _P, C.c_int64, _P, _P, C.c_int64, _P,
                                    _P, _P]),
    "mt3_op_analyze_harmony": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, C.c_int32, _P, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, _P, _P, _P, _P]),
}

_lib = None


def load():
    """Load (once) and type the library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Mt3Error(MT3_ERR_MISSING,
                       "%s not found: build it with `python -m mt3_amd.build` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    try:
        import torch  # noqa: F401  -- load torch's HIP runtime first so both share one libamdhip64
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError here == a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int):
    if rc != MT3_OK:
        raise Mt3Error(rc, (load().mt3_last_error() or b"").decode("utf-8", "replace"))
    return rc
