"""Encoder-decoder engine wrapper (mirror of mt3/network.py's public surface).

`T5Config` keeps the reference's field names (network.py:25-41; values of
mt3/gin/model.gin:47-59 as defaults).  `Transformer` owns one `mt3_engine` of
libmt3hip.so: `encode()` = network.Transformer.encode (network.py:275-301) plus the
hoisted cross-attention K/V; `decode()` = the cached greedy loop that t5x runs
around network.Transformer.decode (network.py:303-361).  Device memory for inputs
and outputs is plain torch CUDA tensors; all compute is in the library.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib


@dataclasses.dataclass(frozen=True)
class T5Config:
    vocab_size: int = 1536
    dtype: str = "bfloat16"          # MFMA operand type: 'bfloat16' (product) or 'float32' (parity path)
    emb_dim: int = 512
    num_heads: int = 6
    num_encoder_layers: int = 8
    num_decoder_layers: int = 8
    head_dim: int = 64
    mlp_dim: int = 1024
    mlp_activations: Sequence[str] = ("gelu", "linear")
    dropout_rate: float = 0.1        # unused at inference
    logits_via_embedding: bool = False
    input_depth: int = 512           # spectrograms.input_depth
    kv_dtype: str = ""               # "" = K/V caches in `dtype`; "fp8_e4m3" (with bfloat16): e4m3 rows + per-row scales
    dense_dtype: str = ""            # "" = dense layers in `dtype`; "fp8_e4m3" (with bfloat16): the encoder's dense layers and
                                     # the cross-K/V projections as MXFP8 (e4m3 + one E8M0 scale per 32 K) on the scaled MFMA


MT3_SMALL = T5Config()                                           # model.gin / ismir2022/small.gin
MT3_BASE = T5Config(emb_dim=768, num_heads=12, num_encoder_layers=12, num_decoder_layers=12,
                    mlp_dim=2048)                                # ismir2022/base.gin:4-10


def param_shapes(cfg: T5Config) -> Dict[str, tuple]:
    """Flax parameter tree of network.Transformer flattened with '/' (SURVEY.md A.3)."""
    e, hd, f, v = cfg.emb_dim, cfg.num_heads * cfg.head_dim, cfg.mlp_dim, cfg.vocab_size
    s = {"encoder/continuous_inputs_projection/kernel": (cfg.input_depth, e),
         "encoder/encoder_norm/scale": (e,),
         "decoder/token_embedder/embedding": (v, e),
         "decoder/decoder_norm/scale": (e,),
         "decoder/logits_dense/kernel": (e, v)}

    def attn(p):
        for n in ("query", "key", "value"):
            s[f"{p}/{n}/kernel"] = (e, hd)
        s[f"{p}/out/kernel"] = (hd, e)

    def mlp(p):
        s[f"{p}/wi_0/kernel"] = (e, f)
        s[f"{p}/wi_1/kernel"] = (e, f)
        s[f"{p}/wo/kernel"] = (f, e)

    for i in range(cfg.num_encoder_layers):
        p = f"encoder/layers_{i}"
        s[f"{p}/pre_attention_layer_norm/scale"] = (e,)
        attn(f"{p}/attention")
        s[f"{p}/pre_mlp_layer_norm/scale"] = (e,)
        mlp(f"{p}/mlp")
    for i in range(cfg.num_decoder_layers):
        p = f"decoder/layers_{i}"
        s[f"{p}/pre_self_attention_layer_norm/scale"] = (e,)
        attn(f"{p}/self_attention")
        s[f"{p}/pre_cross_attention_layer_norm/scale"] = (e,)
        attn(f"{p}/encoder_decoder_attention")
        s[f"{p}/pre_mlp_layer_norm/scale"] = (e,)
        mlp(f"{p}/mlp")
    return s


def init_random_params(cfg: T5Config, seed: int = 0, norm_scale_jitter: float = 0.0) -> Dict[str, np.ndarray]:
    """Random-init weights with the reference's initialisers:
    embedding N(0,1) (network.py:221); attention kernels N(0, 1/fan_in), query / sqrt(head_dim)
    (layers.py:177-178,230-234); MLP / logits / input projection truncated-normal fan-in
    (layers.py:384-385, flax lecun_normal); norm scales 1 (optionally jittered for tests so that
    the scale-folding is exercised)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in param_shapes(cfg).items():
        if name.endswith("/scale"):
            w = torch.ones(shape)
            if norm_scale_jitter:
                w = w + norm_scale_jitter * torch.randn(shape, generator=g)
        elif name.endswith("/embedding"):
            w = torch.randn(shape, generator=g)
        else:
            fan_in = shape[0]
            std = math.sqrt(1.0 / fan_in)
            if "/attention/" in name or "_attention/" in name:
                w = torch.randn(shape, generator=g) * std
                if name.endswith("query/kernel"):
                    w = w / math.sqrt(cfg.head_dim)
            else:
                w = torch.empty(shape)
                torch.nn.init.trunc_normal_(w, mean=0.0, std=1.0, a=-2.0, b=2.0, generator=g)
                w = w * (std / 0.87962566103423978)
        out[name] = w.numpy().astype(np.float32)
    return out


class Transformer:
    """One engine per (device, stream)."""

    def __init__(self, config: T5Config, input_length: int = 256, max_decode_length: int = 1024,
                 max_batch: int = 8, decode_chains: int = 1, options: int = 0):
        """options: bit set of _lib.OPT_* (mt3_engine_config.options): how the same function is evaluated --
        OPT_SINGLE_RESIDUAL_STREAM / OPT_ENCODER_SINGLE_RESIDUAL_STREAM (no bf16 copy / partial sums of the decoder's /
        encoder's residual rows), OPT_SEPARATE_PROJECTIONS
        (no folding of projections into neighbouring launches).  0 = the defaults."""
        self.config = config
        self.input_length, self.max_decode_length, self.max_batch = input_length, max_decode_length, max_batch
        if config.dtype not in ("bfloat16", "float32"):
            raise ValueError("T5Config.dtype must be 'bfloat16' or 'float32'")
        if config.kv_dtype not in ("", "fp8_e4m3") or (config.kv_dtype and config.dtype != "bfloat16"):
            raise ValueError("T5Config.kv_dtype must be '' or 'fp8_e4m3' (the latter with dtype 'bfloat16')")
        if config.dense_dtype not in ("", "fp8_e4m3") or (config.dense_dtype and config.dtype != "bfloat16"):
            raise ValueError("T5Config.dense_dtype must be '' or 'fp8_e4m3' (the latter with dtype 'bfloat16')")
        self._lib = _lib.load()
        ec = _lib.EngineConfig(config.vocab_size, config.emb_dim, config.num_heads, config.head_dim, config.mlp_dim,
                               config.num_encoder_layers, config.num_decoder_layers, config.input_depth,
                               input_length, max_decode_length, max_batch,
                               _lib.MT3_BF16 if config.dtype == "bfloat16" else _lib.MT3_F32, decode_chains,
                               _lib.MT3_FP8_E4M3 if config.kv_dtype == "fp8_e4m3" else 0,
                               _lib.MT3_FP8_E4M3 if config.dense_dtype == "fp8_e4m3" else 0, options)
        self._ec = ec
        self._h = None
        self._create()

    def _create(self):
        h = C.c_void_p()
        _lib.check(self._lib.mt3_engine_create(C.byref(self._ec), C.byref(h)))
        old, self._h = self._h, h
        if old:
            self._lib.mt3_engine_destroy(old)
        self._loaded = False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.mt3_engine_destroy(h)

    def load_params(self, params: Dict[str, np.ndarray]):
        """`params`: flat dict in the reference's names/orientation (f32).  Names outside the network's
        parameter tree (optimizer state, other heads of a larger checkpoint) are ignored; kernels stored with
        split head axes (exactly [in, heads, head_dim] or [heads, head_dim, out]) are flattened to the 2-D DenseGeneral
        form, any other shape is an error; names outside the tree are listed in `self.ignored_params`; a second call
        re-restores (the engine is rebuilt and the encoded batch of the old one is gone), as the reference's
        restore_from_checkpoint allows."""
        if self._loaded:
            self._create()
        want = param_shapes(self.config)
        missing = [n for n in want if n not in params]
        if missing:
            raise _lib.Mt3Error(_lib.MT3_ERR_MISSING, "weights missing from the checkpoint: %s%s"
                                % (", ".join(missing[:4]), " ..." if len(missing) > 4 else ""))
        self.ignored_params = sorted(n for n in params if n not in want)     # reported, not silently dropped
        H, D = self.config.num_heads, self.config.head_dim
        for name, shape in want.items():
            arr = np.asarray(params[name])
            if arr.shape != shape:
                # DenseGeneral kernels with split head axes (layers.py:373-418): ONLY the two layouts flax produces
                # -- q/k/v [in, heads, head_dim], out [heads, head_dim, out] -- whose C-order flattening is the 2-D form
                if arr.ndim == 3 and len(shape) == 2 and (arr.shape == (shape[0], H, D) or arr.shape == (H, D, shape[1])):
                    arr = arr.reshape(shape)
                else:
                    raise _lib.Mt3Error(_lib.MT3_ERR_INVALID, "weight %s has shape %s, expected %s"
                                        % (name, tuple(arr.shape), shape))
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            _lib.check(self._lib.mt3_engine_load_weight(self._h, name.encode(), a.ctypes.data, shape, a.ndim))
        _lib.check(self._lib.mt3_engine_finalize(self._h))
        self._loaded = True

    @property
    def device_bytes(self) -> int:
        return int(self._lib.mt3_engine_device_bytes(self._h))

    def encode(self, encoder_input_tokens, return_encoded: bool = False, num_beams: int = 1):
        """encoder_input_tokens: CUDA f32 tensor [B, T, input_depth].  num_beams = k > 1: each segment is encoded k times
        in a row (B * k engine rows, the input `decode_beams(k)` expects; `decode()` would then decode every copy)."""
        import torch
        x = encoder_input_tokens
        if x.dim() != 3 or x.shape[1] != self.input_length or x.shape[2] != self.config.input_depth:
            raise ValueError(f"expected [B, {self.input_length}, {self.config.input_depth}], got {tuple(x.shape)}")
        x = x.to(device="cuda", dtype=torch.float32).contiguous()
        if num_beams < 1:
            raise ValueError(f"num_beams must be >= 1, got {num_beams}")
        if num_beams > 1:
            x = x.repeat_interleave(num_beams, 0).contiguous()
        enc = torch.empty((x.shape[0], x.shape[1], self.config.emb_dim), device="cuda", dtype=torch.float32) \
            if return_encoded else None
        _lib.check(self._lib.mt3_engine_encode(self._h, x.data_ptr(), x.shape[0], enc.data_ptr() if enc is not None
                                               else None, torch.cuda.current_stream().cuda_stream))
        self._batch = x.shape[0]
        self._encoded_beams = num_beams
        return enc

    def decode(self, num_steps: Optional[int] = None, use_graph: bool = True, early_exit: bool = False,
               return_first_logits: bool = False, chains: int = 0, beam1: bool = False, single_stream: bool = False,
               wait: bool = True):
        """Decode for the batch of the last `encode`: greedy until EOS, or with `beam1` the selection
        rule of t5x beam_search(num_decodes=1, alpha=0.6) that the reference's predict_tokens runs.
        Returns int32 CUDA [B, L] ids (and the step-0 logits [B, V] if asked).  Batches of >= 128 rows are
        decoded as 2 or 4 row groups on streams with hardware queues of their own (include/mt3_hip.h) unless `single_stream`.
        early_exit: stop when every row has finished, and RETIRE finished rows meanwhile (no K/V is streamed for them, the
        live rows are compacted; ids up to each row's EOS are unchanged).  wait=False: MT3_DECODE_ASYNC -- the call returns
        once the engine's worker threads have the decode; `decode_wait()` joins it and returns the ids."""
        import torch
        B, L = self._batch, self.max_decode_length
        ids = torch.empty((B, L), device="cuda", dtype=torch.int32)
        logits = torch.empty((B, self.config.vocab_size), device="cuda", dtype=torch.float32) \
            if return_first_logits else None
        flags = (0 if use_graph else _lib.DECODE_NO_GRAPH) | (_lib.DECODE_EARLY_EXIT if early_exit else 0) | \
            ((chains & 0xF) << 8) | (_lib.DECODE_BEAM1 if beam1 else 0) | \
            (_lib.DECODE_SINGLE_STREAM if single_stream else 0) | (0 if wait else _lib.DECODE_ASYNC)
        ran = C.c_int32()
        _lib.check(self._lib.mt3_engine_decode(self._h, B, num_steps or L, flags, ids.data_ptr(),
                                               logits.data_ptr() if logits is not None else None, C.byref(ran),
                                               torch.cuda.current_stream().cuda_stream))
        if not wait:
            self._async = (ids, logits)              # kept alive until decode_wait
            return None
        self.steps_run = ran.value
        return (ids, logits) if return_first_logits else ids

    def decode_beams(self, num_beams: int, num_steps: Optional[int] = None, use_graph: bool = True,
                     early_exit: bool = False, single_stream: bool = False, return_all: bool = False):
        """mt3_engine_decode_beams: t5x beam_search(alpha=0.6) with num_decodes = num_beams (1 .. 8) for the segments of
        the last `encode(x, num_beams=num_beams)` (include/mt3_hip.h states the rule).  Returns int32 CUDA ids [B, L] of
        the best decode and f32 scores [B]; with `return_all` all k decodes [B, k, L] and their scores [B, k] in
        increasing order of score (the best last, as t5x returns them).  early_exit: stop once every segment's search is
        closed (a closed segment's beams cost no attention meanwhile); `self.steps_run` says how many steps ran."""
        import torch
        k = int(num_beams)
        if k < 1 or k > _lib.MAX_BEAMS:
            raise ValueError(f"num_beams must be 1 .. {_lib.MAX_BEAMS}, got {num_beams}")
        if getattr(self, "_encoded_beams", 1) != k or self._batch % k:
            raise ValueError(f"decode_beams({k}) needs the segments encoded with encode(x, num_beams={k}) first")
        B, L = self._batch // k, self.max_decode_length
        ids = torch.empty((B, L), device="cuda", dtype=torch.int32)
        all_ids = torch.empty((B, k, L), device="cuda", dtype=torch.int32) if return_all else None
        scores = torch.empty((B, k), device="cuda", dtype=torch.float32)
        flags = (0 if use_graph else _lib.DECODE_NO_GRAPH) | (_lib.DECODE_EARLY_EXIT if early_exit else 0) | \
            (_lib.DECODE_SINGLE_STREAM if single_stream else 0)
        ran = C.c_int32()
        _lib.check(self._lib.mt3_engine_decode_beams(self._h, B, k, num_steps or L, flags, ids.data_ptr(),
                                                     all_ids.data_ptr() if all_ids is not None else None,
                                                     scores.data_ptr(), C.byref(ran),
                                                     torch.cuda.current_stream().cuda_stream))
        self.steps_run = ran.value
        if return_all:
            return all_ids, scores
        return ids, scores[:, -1].contiguous()

    def transcribe(self, encoder_input_tokens, num_steps: Optional[int] = None, beam1: bool = False,
                   use_graph: bool = True, single_stream: bool = False, debug_poll_steps: int = 0,
                   debug_row_groups: int = 0, debug_skip_encoder_passes: bool = False,
                   num_beams: Optional[int] = None, return_all: bool = False, draws: Optional[int] = None):
        """mt3_engine_transcribe: encode + decode of ANY number of segments through the engine's `max_batch` decode slots
        with in-flight batching -- a slot whose segment has finished restarts on the next one (the reference's loop over
        `.batch(8)` calls of predict_batch_with_aux, NB:295-301, without its batch-synchronous wait for the longest row).
        encoder_input_tokens: CUDA f32 [N, T, input_depth].  Returns int32 CUDA [N, L] ids, row i = segment i, bit-identical
        to encode() + decode(early_exit=True) of that segment; `self.transcribe_stats` says what ran.
        num_beams = k (1 .. 8): mt3_engine_transcribe_beams -- the k-beam search of `decode_beams` with in-flight batching
        of max_batch // k elements of k slots each (each segment is passed once).  Returns the ids [N, L] of the best
        decode, or with `return_all` all k decodes [N, k, L] and their scores [N, k] in increasing order of score:
        bit-identical to encode(x, num_beams=k) + decode_beams(k, early_exit=True) of each segment.
        draws = per (>= 1): mt3_engine_transcribe_draws -- `per` decodes of every segment in ONE job, each segment encoded
        once.  Returns ids [N * per, L], row s * per + j = draw j of segment s; "segment i" of every per-segment table
        (masks, prompts, sampling streams and seeds, the EOS schedule) means draw i.  Bit-identical to
        transcribe(x.repeat_interleave(per, 0)) under the same tables.  Not with num_beams, beam1 or the debug_* schedule."""
        import torch
        x = encoder_input_tokens
        if x.dim() != 3 or x.shape[1] != self.input_length or x.shape[2] != self.config.input_depth:
            raise ValueError(f"expected [N, {self.input_length}, {self.config.input_depth}], got {tuple(x.shape)}")
        x = x.to(device="cuda", dtype=torch.float32).contiguous()
        N, L = x.shape[0], self.max_decode_length
        if num_beams is not None:
            k = int(num_beams)
            if k < 1 or k > min(_lib.MAX_BEAMS, self.max_batch):
                raise ValueError(f"num_beams must be 1 .. {min(_lib.MAX_BEAMS, self.max_batch)}, got {num_beams}")
            if beam1 or debug_poll_steps or debug_row_groups or debug_skip_encoder_passes or draws is not None:
                raise ValueError("num_beams goes with neither beam1, draws nor the debug_* schedule parameters")
            ids = torch.empty((N, L), device="cuda", dtype=torch.int32)
            all_ids = torch.empty((N, k, L), device="cuda", dtype=torch.int32) if return_all else None
            scores = torch.empty((N, k), device="cuda", dtype=torch.float32) if return_all else None
            flags = (0 if use_graph else _lib.DECODE_NO_GRAPH) | (_lib.DECODE_SINGLE_STREAM if single_stream else 0)
            st = _lib.TranscribeStats()
            _lib.check(self._lib.mt3_engine_transcribe_beams(
                self._h, x.data_ptr(), N, k, num_steps or L, flags, ids.data_ptr(),
                all_ids.data_ptr() if return_all else None, scores.data_ptr() if return_all else None, C.byref(st),
                torch.cuda.current_stream().cuda_stream))
            self._batch = int(st.slots)
            self._encoded_beams = k
            self.transcribe_stats = {n: int(getattr(st, n)) for n, _ in st._fields_ if n != "reserved"}
            self.last_transcribe_stats = self.transcribe_stats
            self.steps_run = st.steps_run
            return (all_ids, scores) if return_all else ids
        if return_all:
            raise ValueError("return_all needs num_beams")
        if draws is not None:
            per = int(draws)
            if per < 1:
                raise ValueError(f"draws must be at least 1, got {draws}")
            if beam1 or debug_poll_steps or debug_row_groups or debug_skip_encoder_passes:
                raise ValueError("draws goes with neither beam1 nor the debug_* schedule parameters")
            ids = torch.empty((N * per, L), device="cuda", dtype=torch.int32)
            flags = (0 if use_graph else _lib.DECODE_NO_GRAPH) | (_lib.DECODE_SINGLE_STREAM if single_stream else 0)
            st = _lib.TranscribeStats()
            _lib.check(self._lib.mt3_engine_transcribe_draws(self._h, x.data_ptr(), N, per, num_steps or L, flags,
                                                             ids.data_ptr(), C.byref(st),
                                                             torch.cuda.current_stream().cuda_stream))
            self._batch = int(st.slots)
            self.transcribe_stats = {n: int(getattr(st, n)) for n, _ in st._fields_ if n != "reserved"}
            self.last_transcribe_stats = self.transcribe_stats
            self.steps_run = st.steps_run
            return ids
        ids = torch.empty((N, L), device="cuda", dtype=torch.int32)
        flags = (0 if use_graph else _lib.DECODE_NO_GRAPH) | (_lib.DECODE_BEAM1 if beam1 else 0) | \
            (_lib.DECODE_SINGLE_STREAM if single_stream else 0)
        st = _lib.TranscribeStats()
        if debug_poll_steps or debug_row_groups or debug_skip_encoder_passes:      # mt3_debug_engine_transcribe (A/B measurements only)
            _lib.check(self._lib.mt3_debug_engine_transcribe(self._h, x.data_ptr(), N, num_steps or L, flags,
                                                             debug_poll_steps, debug_row_groups,
                                                             1 if debug_skip_encoder_passes else 0, ids.data_ptr(),
                                                             C.byref(st), torch.cuda.current_stream().cuda_stream))
        else:
            _lib.check(self._lib.mt3_engine_transcribe(self._h, x.data_ptr(), N, num_steps or L, flags, ids.data_ptr(),
                                                       C.byref(st), torch.cuda.current_stream().cuda_stream))
        self._batch = min(N, self.max_batch)
        self.transcribe_stats = {n: int(getattr(st, n)) for n, _ in st._fields_ if n != "reserved"}
        self.last_transcribe_stats = self.transcribe_stats
        self.steps_run = st.steps_run
        return ids

    def decode_wait(self):
        """mt3_engine_decode_wait: join the decode a `decode(wait=False)` started; returns what that call would have."""
        ran = C.c_int32()
        _lib.check(self._lib.mt3_engine_decode_wait(self._h, C.byref(ran)))
        ids, logits = self._async
        self._async = None
        self.steps_run = ran.value
        return (ids, logits) if logits is not None else ids

    def debug_set_eos_schedule(self, lengths=None):
        """mt3_debug_engine_set_eos_schedule (include/mt3_hip_debug.h): impose output lengths -- row r's distribution at
        step lengths[r] - 1 becomes a point mass on EOS (SURVEY.md 8(d)'s synthetic EOS schedule).  None: off."""
        if lengths is None:
            _lib.check(self._lib.mt3_debug_engine_set_eos_schedule(self._h, None, 0))
            return
        a = np.ascontiguousarray(lengths, dtype=np.int32)
        _lib.check(self._lib.mt3_debug_engine_set_eos_schedule(self._h, a.ctypes.data, int(a.size)))

    def set_token_masks(self, masks, seg_mask=None):
        """mt3_engine_set_token_masks: constrain every later decode / decode_beams / transcribe call until
        `clear_token_masks`.  masks: uint32 [n_masks, ceil(vocab / 32)] (or one row), bit i % 32 of word i // 32 set =
        token i allowed (`vocabularies.token_mask`); seg_mask: int32 mask index per batch row / beam element / segment of
        the job, -1 = unconstrained (None: mask 0 everywhere, n_masks must be 1).  A disallowed token's logit counts as
        -inf in the token pick and the log-sum-exp; returned logits stay unmasked.  decode_forced / score /
        score_segments ignore masks."""
        m = np.ascontiguousarray(masks, dtype=np.uint32)
        m = m.reshape(1, -1) if m.ndim == 1 else m
        words = (self.config.vocab_size + 31) // 32
        if m.ndim != 2 or m.shape[1] != words:
            raise ValueError("masks must be [n_masks, %d] uint32 words for vocab %d" % (words, self.config.vocab_size))
        if seg_mask is None:
            _lib.check(self._lib.mt3_engine_set_token_masks(self._h, m.ctypes.data, int(m.shape[0]), None, 0))
            return
        sm = np.ascontiguousarray(seg_mask, dtype=np.int32).reshape(-1)
        _lib.check(self._lib.mt3_engine_set_token_masks(self._h, m.ctypes.data, int(m.shape[0]), sm.ctypes.data,
                                                        int(sm.size)))

    def clear_token_masks(self):
        _lib.check(self._lib.mt3_engine_set_token_masks(self._h, None, 0, None, 0))

    def set_prompts(self, prompts, seg_prompt=None):
        """mt3_engine_set_prompts: forced token prefixes for every later decode / decode_beams / transcribe call until
        cleared (`set_prompts(None)`).  prompts: a list of id sequences (padded with 0 to the longest) or a 2-D int array
        [n_prompts, stride], ids in [2, vocab), 0 = padding; None or [] clears.  seg_prompt: int32 prompt index per batch
        row / beam element / segment of the job, -1 = none (None: prompt 0 everywhere, n_prompts must be 1).  A segment's
        output begins with its prompt (`vocabularies.tie_section_prompt` builds MT3's: the tie section); the prompt's
        tokens are not scored, and the search continues from there.  decode_forced / score / score_segments ignore
        prompts."""
        if prompts is None or len(prompts) == 0:
            _lib.check(self._lib.mt3_engine_set_prompts(self._h, None, 0, 0, None, 0))
            return
        if isinstance(prompts, np.ndarray):
            p = np.ascontiguousarray(prompts, dtype=np.int32)
            p = p.reshape(1, -1) if p.ndim == 1 else p
        else:
            rows = [np.asarray(r, dtype=np.int32).reshape(-1) for r in prompts]
            p = np.zeros((len(rows), max(1, max(r.size for r in rows))), np.int32)
            for i, r in enumerate(rows):
                p[i, :r.size] = r
        if p.ndim != 2:
            raise ValueError("prompts must be a list of id sequences or a 2-D array")
        if seg_prompt is None:
            _lib.check(self._lib.mt3_engine_set_prompts(self._h, p.ctypes.data, int(p.shape[0]), int(p.shape[1]), None, 0))
            return
        sp = np.ascontiguousarray(seg_prompt, dtype=np.int32).reshape(-1)
        _lib.check(self._lib.mt3_engine_set_prompts(self._h, p.ctypes.data, int(p.shape[0]), int(p.shape[1]),
                                                    sp.ctypes.data, int(sp.size)))

    def set_token_grammar(self, grammar):
        """mt3_engine_set_token_grammar: well-formed decoding for every later decode / decode_beams / transcribe call
        until `clear_token_grammar`.  grammar: a `_lib.TokenGrammar` (`vocabularies.token_grammar`).  The token pick then
        never takes a shift that runs backwards, repeats or passes max_steps, a `tie` outside the tie section, or anything
        but program / pitch / tie inside it; with token masks the allowed set is the intersection, prompts win inside the
        prompt and advance the state.  decode_forced / score / score_segments ignore it."""
        _lib.check(self._lib.mt3_engine_set_token_grammar(self._h, C.byref(grammar)))

    def clear_token_grammar(self):
        _lib.check(self._lib.mt3_engine_set_token_grammar(self._h, None))

    def set_note_grammar(self, grammar):
        """mt3_engine_set_note_grammar: note-consistent decoding for every later decode / decode_beams / transcribe call
        until `clear_note_grammar`.  grammar: a `_lib.NoteGrammar` (`vocabularies.note_grammar`); its `g` member is the
        event grammar, so no token grammar may be set beside it.  On top of `set_token_grammar`'s rule the token pick never
        takes a note-off of a pitch that is not sounding on the current program, a second declaration of a pair in the tie
        section, or a drum at velocity 0.  decode_forced / score / score_segments ignore it."""
        _lib.check(self._lib.mt3_engine_set_note_grammar(self._h, C.byref(grammar)))

    def clear_note_grammar(self):
        _lib.check(self._lib.mt3_engine_set_note_grammar(self._h, None))

    def tie_prompts(self, ids, grammar, cap: int = 64, drop_redundant_programs: bool = True, return_held: bool = False):
        """mt3_op_tie_prompts: what each emitted id row left sounding, as the tie section of the file's next segment.
        ids: int32 CUDA [rows, n] engine id rows (what decode / transcribe return: prompt included, 0 after EOS); grammar:
        a `_lib.NoteGrammar`.  Returns int32 CUDA prompts [rows, 2 * cap + 1] (0-padded rows for `set_prompts`; the bare
        `tie` where nothing sounds) and counts [rows], the pairs held before the cut to `cap`; with return_held also the
        held tables uint32-as-int32 [rows, table_words].  The rule: `mt3_amd/ties.py`."""
        import torch
        if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 1:
            raise ValueError("ids must be a CUDA tensor [rows >= 1, n >= 1]")
        if int(cap) < 0:
            raise ValueError("cap must not be negative, got %r" % (cap,))
        ids = ids.to(dtype=torch.int32).contiguous()
        rows, cap = int(ids.shape[0]), int(cap)
        prompts = torch.empty((rows, 2 * cap + 1), device=ids.device, dtype=torch.int32)
        counts = torch.empty((rows,), device=ids.device, dtype=torch.int32)
        words = int(self._lib.mt3_note_grammar_table_words(C.byref(grammar)))
        held = torch.empty((rows, words), device=ids.device, dtype=torch.int32) if return_held else None
        _lib.check(self._lib.mt3_op_tie_prompts(
            C.byref(grammar), ids.data_ptr(), rows, int(ids.shape[1]), cap,
            _lib.TIE_DROP_REDUNDANT_PROGRAMS if drop_redundant_programs else 0, prompts.data_ptr(), counts.data_ptr(),
            held.data_ptr() if held is not None else None, torch.cuda.current_stream().cuda_stream))
        return (prompts, counts, held) if return_held else (prompts, counts)

    def set_sampling(self, params=None, seg_stream=None, seg_seed=None, **kw):
        """mt3_engine_set_sampling: every later decode / transcribe call (greedy path; not beam1) DRAWS its free tokens --
        t5x temperature_sample -- until `clear_sampling`.  params: a `sampling.SamplingParams`, or its fields as keywords
        (temperature=1.0, top_k=0, top_p=0.0, seed=0).  seg_stream: the uint64 noise stream of each batch row / segment of
        the job (None: row / segment i draws from stream i); a segment's sample depends on (seed, stream) and its logits
        only, not on the slot, the batch or the schedule.  seg_seed (mt3_engine_set_sampling_seeds): the uint64 Philox key
        of each batch row / segment / draw in place of params.seed (None: params.seed everywhere) -- what tells the draws
        of one segment in `transcribe(draws=per)` apart.  The sampled step graphs hold whether there is a seed table: a
        call that sets one after a call that set none (or the reverse) waits for the device and drops the captured step
        graphs, so alternating the two forms costs a recapture at each switch.  top_k=1 is greedy.  decode_beams, transcribe(num_beams=...),
        decode_forced, score and score_segments ignore it."""
        from . import sampling
        p = (params if params is not None else sampling.SamplingParams(**kw)).check()
        st = p.struct()
        if seg_stream is None:
            _lib.check(self._lib.mt3_engine_set_sampling(self._h, C.byref(st), None, 0))
        else:
            ss = np.ascontiguousarray(np.asarray(seg_stream).astype(np.uint64)).reshape(-1)
            _lib.check(self._lib.mt3_engine_set_sampling(self._h, C.byref(st), ss.ctypes.data, int(ss.size)))
        if seg_seed is None:
            _lib.check(self._lib.mt3_engine_set_sampling_seeds(self._h, None, 0))
        else:
            sd = np.ascontiguousarray(np.asarray(seg_seed).astype(np.uint64)).reshape(-1)
            _lib.check(self._lib.mt3_engine_set_sampling_seeds(self._h, sd.ctypes.data, int(sd.size)))

    def clear_sampling(self):
        _lib.check(self._lib.mt3_engine_set_sampling(self._h, None, None, 0))

    def debug_decode(self, num_steps: Optional[int] = None, skip_self_attn: bool = False,
                     skip_cross_attn: bool = False, chains: int = 0, use_graph: bool = True):
        """mt3_debug_engine_decode (include/mt3_hip_debug.h): a decode with kernels left out of every step, for
        differential timing only -- the ids it returns are meaningless."""
        import torch
        B, L = self._batch, self.max_decode_length
        ids = torch.empty((B, L), device="cuda", dtype=torch.int32)
        skip = (_lib.DEBUG_SKIP_SELF_ATTN if skip_self_attn else 0) | (_lib.DEBUG_SKIP_CROSS_ATTN if skip_cross_attn else 0)
        flags = (0 if use_graph else _lib.DECODE_NO_GRAPH) | ((chains & 0xF) << 8)
        _lib.check(self._lib.mt3_debug_engine_decode(self._h, B, num_steps or L, flags, skip, ids.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream))
        return ids

    def debug_poison_caches(self, pattern: int = 0xFF, cross: bool = False):
        """mt3_debug_engine_poison_caches: fill the K/V caches with a byte pattern (0xFF = NaN in every cache format)."""
        import torch
        _lib.check(self._lib.mt3_debug_engine_poison_caches(self._h, pattern, 1 if cross else 0,
                                                            torch.cuda.current_stream().cuda_stream))

    def decode_forced(self, forced_ids, num_steps: Optional[int] = None, use_graph: bool = True,
                      return_logits: bool = True, chains: int = 0):
        """Teacher-forced cached decode (network.Transformer.decode on given decoder inputs, one token per cached
        step): step 0 is fed BOS, step t+1 is fed forced_ids[:, t].  forced_ids: int32 [B, <= L].
        Returns (argmax ids int32 CUDA [B, L], logits f32 CUDA [num_steps, B, V] or None)."""
        import torch
        B, L = self._batch, self.max_decode_length
        f = torch.zeros((B, L), device="cuda", dtype=torch.int32)
        src = torch.as_tensor(forced_ids).to(device="cuda", dtype=torch.int32)
        if src.dim() != 2 or src.shape[0] != B or src.shape[1] > L:
            raise ValueError(f"forced_ids must be [B={B}, <= {L}], got {tuple(src.shape)}")
        f[:, : src.shape[1]] = src
        n = num_steps or L
        ids = torch.empty((B, L), device="cuda", dtype=torch.int32)
        logits = torch.empty((n, B, self.config.vocab_size), device="cuda", dtype=torch.float32) \
            if return_logits else None
        flags = (0 if use_graph else _lib.DECODE_NO_GRAPH) | ((chains & 0xF) << 8)
        _lib.check(self._lib.mt3_engine_decode_forced(self._h, B, n, flags, f.data_ptr(),
                                                      logits.data_ptr() if logits is not None else None,
                                                      ids.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.current_stream().synchronize()          # `f` must outlive the copy the call enqueued
        return ids, logits

    def score(self, targets, decoder_inputs=None, weights=None, return_token_scores: bool = False,
              return_logits: bool = False):
        """mt3_engine_score: t5x score_batch on the segments of the last `encode` (include/mt3_hip.h states the rule).
        targets: int32 [B, <= L] vocabulary ids (0 = padding; B <= the encoded batch), CUDA or host; decoder_inputs (same
        shape, default shift_right(targets) with BOS = 0) and weights (f32, default target > 0) likewise.  Narrower
        arrays are padded with 0 to the width of `targets`, the call's length.  Returns the f32 CUDA sequence scores [B],
        or a tuple (scores, token_scores [B, length] if asked, logits [B, length, V] if asked)."""
        import torch
        if self.config.kv_dtype:
            raise ValueError("scoring is not available with kv_dtype=%r (e4m3 cross caches are out of scope)"
                             % (self.config.kv_dtype,))
        tgt = torch.as_tensor(targets)
        if tgt.dim() != 2 or tgt.shape[1] < 1 or tgt.shape[1] > self.max_decode_length:
            raise ValueError(f"targets must be [B, 1 .. {self.max_decode_length}], got {tuple(tgt.shape)}")
        B, n = int(tgt.shape[0]), int(tgt.shape[1])
        if not 1 <= B <= getattr(self, "_batch", 0):
            raise ValueError(f"targets has {B} rows; the last encode holds {getattr(self, '_batch', 0)}")

        def padded(a, dtype):
            if a is None:
                return None
            a = torch.as_tensor(a).to(device="cuda", dtype=dtype)
            if a.dim() != 2 or a.shape[0] != B or a.shape[1] > n:
                raise ValueError(f"expected [B={B}, <= {n}], got {tuple(a.shape)}")
            out = torch.zeros((B, n), device="cuda", dtype=dtype)
            out[:, : a.shape[1]] = a
            return out

        tgt = padded(tgt, torch.int32)
        if int(tgt.min()) < 0 or int(tgt.max()) >= self.config.vocab_size:
            raise ValueError("target ids must lie in [0, vocab_size)")
        din = padded(decoder_inputs, torch.int32)
        if din is not None and (int(din.min()) < 0 or int(din.max()) >= self.config.vocab_size):
            raise ValueError("decoder input ids must lie in [0, vocab_size)")
        w = padded(weights, torch.float32)
        seq = torch.empty((B,), device="cuda", dtype=torch.float32)
        tok = torch.empty((B, n), device="cuda", dtype=torch.float32) if return_token_scores else None
        logits = torch.empty((B, n, self.config.vocab_size), device="cuda", dtype=torch.float32) if return_logits else None
        ptr = (lambda t: t.data_ptr() if t is not None else None)
        _lib.check(self._lib.mt3_engine_score(self._h, B, n, ptr(tgt), ptr(din), ptr(w), ptr(seq), ptr(tok), ptr(logits),
                                              torch.cuda.current_stream().cuda_stream))
        torch.cuda.current_stream().synchronize()          # the padded inputs must outlive the work the call enqueued
        if not (return_token_scores or return_logits):
            return seq
        return (seq,) + ((tok,) if return_token_scores else ()) + ((logits,) if return_logits else ())

    def score_segments(self, x, targets, return_token_scores: bool = False, return_top1: bool = False):
        """mt3_engine_score_segments: `encode` + `score` over ANY number of segments in chunks of `max_batch`, with the
        statistics a note confidence is made of (include/mt3_hip.h states the contract).  x: CUDA f32 [N, T, input_depth]
        log-mel; targets: int32 [N, 1 .. L] vocabulary ids (0 = padding), CUDA or host; decoder inputs are
        shift_right(targets), weights target > 0.  Returns the f32 CUDA sequence scores [N], or a tuple (scores,
        token_scores [N, length] if asked, top1_ids int32 [N, length] and top1_scores [N, length] if `return_top1`):
        the arg-max of each position's logits (lowest id on ties) and its log-probability.  Leaves the engine encoded
        with the last chunk, as a loop of `encode` calls would."""
        return self._score_job(x, targets, None, return_token_scores, return_top1)

    def score_candidates(self, x, targets, per: int, return_token_scores: bool = False, return_top1: bool = False):
        """mt3_engine_score_candidates: `per` target rows against every segment, each segment encoded ONCE (the table of an
        offset search; include/mt3_hip.h states the contract).  x: CUDA f32 [N, T, input_depth]; targets: int32
        [N * per, 1 .. L], row s * per + j = candidate j of segment s.  Returns what `score_segments` returns on
        `x.repeat_interleave(per, 0)` -- one row per target row, the same bits -- and leaves the engine as
        `score_segments(x, ...)` would.  `status(STATUS_SCORE_ENCODER_PASSES)` reports the encoder passes of the call."""
        per = int(per)
        if per < 1:
            raise ValueError("per must be at least 1, got %r" % (per,))
        return self._score_job(x, targets, per, return_token_scores, return_top1)

    def _score_job(self, x, targets, per, return_token_scores, return_top1):
        """the shared body of `score_segments` (per None) and `score_candidates`"""
        import torch
        if self.config.kv_dtype:
            raise ValueError("scoring is not available with kv_dtype=%r (e4m3 cross caches are out of scope)"
                             % (self.config.kv_dtype,))
        if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] != self.input_length or x.shape[2] != self.config.input_depth:
            raise ValueError(f"expected [N >= 1, {self.input_length}, {self.config.input_depth}], got {tuple(x.shape)}")
        x = x.to(device="cuda", dtype=torch.float32).contiguous()
        N = int(x.shape[0])
        R = N * (per or 1)                                 # target rows
        if R >= 1 << 31:
            raise ValueError("N * per must fit int32")
        tgt = torch.as_tensor(targets)
        if tgt.dim() != 2 or tgt.shape[0] != R or tgt.shape[1] < 1 or tgt.shape[1] > self.max_decode_length:
            rows = f"N={N}" if per is None else f"N * per = {R}"
            raise ValueError(f"targets must be [{rows}, 1 .. {self.max_decode_length}], got {tuple(tgt.shape)}")
        n = int(tgt.shape[1])
        tgt = tgt.to(device="cuda", dtype=torch.int32).contiguous()
        if int(tgt.min()) < 0 or int(tgt.max()) >= self.config.vocab_size:
            raise ValueError("target ids must lie in [0, vocab_size)")
        seq = torch.empty((R,), device="cuda", dtype=torch.float32)
        tok = torch.empty((R, n), device="cuda", dtype=torch.float32) if return_token_scores else None
        top_id = torch.empty((R, n), device="cuda", dtype=torch.int32) if return_top1 else None
        top_sc = torch.empty((R, n), device="cuda", dtype=torch.float32) if return_top1 else None
        ptr = (lambda t: t.data_ptr() if t is not None else None)
        out = (tgt.data_ptr(), ptr(seq), ptr(tok), ptr(top_id), ptr(top_sc), torch.cuda.current_stream().cuda_stream)
        if per is None:
            _lib.check(self._lib.mt3_engine_score_segments(self._h, x.data_ptr(), N, n, *out))
        else:
            _lib.check(self._lib.mt3_engine_score_candidates(self._h, x.data_ptr(), N, per, n, *out))
        torch.cuda.current_stream().synchronize()          # the converted inputs must outlive the work the call enqueued
        last = N - (N - 1) // self.max_batch * self.max_batch          # segments of the last chunk
        pad8 = self.config.dtype == "bfloat16" and N > self.max_batch  # (bf16: encoded in a pass of at least 8 rows)
        self._batch = max(last, min(8, self.max_batch)) if pad8 else last
        self._encoded_beams = 1
        if not (return_token_scores or return_top1):
            return seq
        return (seq,) + ((tok,) if return_token_scores else ()) + ((top_id, top_sc) if return_top1 else ())

    def debug_set_score_chunk(self, segments: int = 0):
        """mt3_debug_engine_set_score_chunk: segments per chunk of `score` (0: the workspace default)."""
        _lib.check(self._lib.mt3_debug_engine_set_score_chunk(self._h, int(segments)))

    def status(self, what: int) -> int:
        """mt3_engine_status: _lib.STATUS_* (graph fallbacks, row groups / compactions of the last decode, ...)."""
        rc = int(self._lib.mt3_engine_status(self._h, what))
        if rc < 0:
            _lib.check(rc)
        return rc
