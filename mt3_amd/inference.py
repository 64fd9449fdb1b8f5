"""Drop-in inference surface of MT3 on the MI355X engine.

`InferenceModel` mirrors the class the reference defines in its Colab notebook
(mt3/colab/music_transcription_with_transformers.ipynb, cell "Imports and
Definitions"): same constructor arguments, attributes (`inputs_length`,
`outputs_length`, `batch_size`, `sequence_length`, `encoding_spec`,
`spectrogram_config`, `codec`, `vocabulary`, `input_shapes`) and methods
(`restore_from_checkpoint`, `predict_tokens`, `__call__`, `audio_to_dataset`,
`preprocess`, `postprocess`, `_trim_eos`).  `write_inferences_to_file` mirrors
mt3/inference.py:34-138 (the t5x `infer` write_fn).

Differences that are deliberate: the t5x/gin/tf.data plumbing is gone -- segments
are cut and padded on the host exactly as the reference's preprocessors do
(`_audio_to_frames`, split into `inputs_length`-frame chunks, zero rows after the
log for a short last segment), everything numeric runs in libmt3hip.so.  `batch_size`
stays the reference's 8 as an ATTRIBUTE (`input_shapes`, NB:190), but the engine behind
`predict_tokens` is sized to the JOB -- up to `max_slots` decode slots, grown lazily -- and
runs mt3_engine_transcribe: a 10-minute file is ONE engine call whose finished rows are
refilled with the file's next segments, not 37 batch-synchronous calls of 8 rows
(`schedule="batch"` keeps the reference's loop for comparison); the log-mel stays on
the device between the frontend and `predict_tokens` (`_examples` returns it beside the examples).  What a call sets
on the engine -- masks, prompts, grammar, sampling -- is one `_Job` value, built in `_job`, passed down to
`_predict_ids` and cleared by `_engine_job`; the model object holds nothing about a call in flight.  Decoding
defaults to `decoding="beam1"`: the selection rule of t5x beam search with one beam and
alpha 0.6, which is what the reference's predict_batch_with_aux runs;
`decoding="greedy"` stops a row at its first arg-max EOS.
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import json
import math
import os
import re
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from . import audio_io
from . import metrics_utils
from . import network
from . import note_arrays
from . import note_sequences
from . import sampling
from . import spectrograms
from . import ties
from . import vocabularies

SAMPLE_RATE = 16000


def trim_eos(tokens: Sequence[int]) -> np.ndarray:
    """tasks.trim_eos (mt3/tasks.py:58-63) == InferenceModel._trim_eos."""
    tokens = np.array(tokens, np.int32)
    if vocabularies.DECODED_EOS_ID in tokens:
        tokens = tokens[: np.argmax(tokens == vocabularies.DECODED_EOS_ID)]
    return tokens


@dataclasses.dataclass(frozen=True)
class _Job:
    """What one decode job sets on the engine (`InferenceModel._job` builds it from the public keywords): a value that
    is passed from the transcribing method down to `_predict_ids`, never kept on the model."""
    decoding: str                                # the decoding rule of this job; the model's own unless `sample*` asks
    sampling: sampling.SamplingParams            # ... and its sampling parameters (decoding == "sample")
    masks: Optional[np.ndarray] = None           # constrained: uint32 [n_masks, words]
    mask_index: Optional[np.ndarray] = None      # ... and the mask of every segment (None: mask 0 everywhere)
    prompts: Optional[List[Any]] = None          # prompted: one id list or None per segment
    grammar: Any = None                          # well-formed: a _lib.TokenGrammar or _lib.NoteGrammar
    tied: bool = False                           # well_formed="tied": a wavefront over segment indices
    streams: Optional[np.ndarray] = None         # the noise stream of every segment (None: its index in the engine call)
    draws: Optional[int] = None                  # `sample` / `sample_many` as one job: the draws of every segment


class InferenceModel(object):
    """Wrapper of the MI355X engine for music transcription."""

    def __init__(self, checkpoint_path, model_type="mt3", *, config: Optional[network.T5Config] = None,
                 dtype: str = "float32", batch_size: int = 8, early_exit: bool = True,
                 decoding: str = "beam1", max_slots: int = 256, schedule: Optional[str] = None, num_beams: int = 4,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, seed: int = 0, cap: int = 64,
                 drop_redundant_programs: bool = True):
        """dtype: 'float32' (default) = the reference's own precision (gin/model.gin:50 restores and runs
        float32): f32 MFMA operands, f32 K/V cache, token-exact against the oracle.  'bfloat16' is the explicit
        opt-in fast path (bf16 operands and caches, f32 accumulation / residual / softmax; what bench.py times;
        logits within 3e-2 rel-L2 of f32 at every cache depth, tests/test_gpu_parity_deep.py).
        max_slots: the most decode slots the engine behind `predict_tokens` may hold (its K/V caches are allocated for
        that many rows: 3.2 GB per 64 slots in f32 at the MT3 shape); the engine starts at `batch_size` slots and is rebuilt
        with more (next power of two) when a job has more segments.  schedule: 'refill' = one mt3_engine_transcribe call
        per job (in-flight batching; needs early_exit); 'batch' = the reference's loop, one batch-synchronous engine call
        per `batch_size` segments (NB:295-301).  None (the default) = 'refill' for 'beam1' / 'greedy'; for decoding='beam'
        it is 'batch' until the comparison of tools/bench_beams.py --refill has been measured in favour of 'refill'
        (the beam row) -- pass schedule='refill' to run the beam search with in-flight batching.
        decoding: 'beam1' (default) / 'greedy' as above; 'beam' = t5x beam_search with num_decodes = `num_beams` (1 .. 8):
        each beam is a decode slot, so a job runs max_slots // num_beams segments at a time.  With schedule='refill' it
        is one mt3_engine_transcribe_beams call per job (Transformer.transcribe(num_beams=k): a segment whose search has
        closed hands its slots to the next segment); with schedule='batch' the segments are encoded and beam-decoded in
        batch-synchronous chunks of max_slots // num_beams (Transformer.decode_beams).  Same tokens either way.
        decoding='sample' = t5x temperature_sample (Transformer.set_sampling): every free token is DRAWN from
        softmax(logits / temperature), cut to the top_k (1 .. 256) most likely tokens or to the smallest set of
        probability top_p (0 .. 1); 0 turns either off, both on is an error.  The draw of a segment depends on `seed`, the
        segment's index within its own file and its logits only: a file's notes are the same alone, in any
        `transcribe_many` / `transcribe_wavs` job and on either schedule (f32; bf16 logits depend on the rows of a launch).
        `sample(audio, num_samples=n)` draws n transcriptions with seeds seed .. seed + n - 1, as ONE engine job in which
        every segment is encoded once (Transformer.transcribe(draws=n)).
        cap / drop_redundant_programs: for well_formed="tied" (`__call__`) -- the most (program, pitch) pairs a tie
        section carried from one segment into the next may declare, and whether it repeats a program id that does not
        change (True, the default, is the form MT3's targets have after remove_redundant_state_changes)."""
        if model_type == "ismir2021":
            num_velocity_bins = 127
            self.encoding_spec = note_sequences.NoteEncodingSpec
            self.inputs_length = 512
        elif model_type == "mt3":
            num_velocity_bins = 1
            self.encoding_spec = note_sequences.NoteEncodingWithTiesSpec
            self.inputs_length = 256
        else:
            raise ValueError("unknown model_type: %s" % model_type)

        self.num_velocity_bins = num_velocity_bins      # 1: every decoded note has the same velocity (see `velocities=`)
        self.batch_size = batch_size             # the reference's 8 (NB:190): what input_shapes reports
        if schedule is None:
            schedule = "batch" if decoding == "beam" else "refill"
        if schedule not in ("refill", "batch"):
            raise ValueError("schedule must be 'refill' or 'batch', got %r" % (schedule,))
        self.schedule = schedule
        self.max_slots = max(int(max_slots), batch_size)
        self.outputs_length = 1024
        self.sequence_length = {"inputs": self.inputs_length, "targets": self.outputs_length}
        self.early_exit = early_exit
        if decoding not in ("beam1", "greedy", "beam", "sample"):
            raise ValueError("decoding must be 'beam1', 'greedy', 'beam' or 'sample', got %r" % (decoding,))
        self.sampling = sampling.SamplingParams(float(temperature), int(top_k), float(top_p), int(seed)).check()
        if int(cap) < 0:
            raise ValueError("cap must not be negative, got %r" % (cap,))
        self.cap = int(cap)
        self.drop_redundant_programs = bool(drop_redundant_programs)
        if decoding == "beam" and not 1 <= int(num_beams) <= min(8, self.max_slots):
            raise ValueError("num_beams must be 1 .. 8 (and <= max_slots), got %r" % (num_beams,))
        self.decoding = decoding
        self.num_beams = int(num_beams) if decoding == "beam" else 1

        self.spectrogram_config = spectrograms.SpectrogramConfig()
        self.codec = vocabularies.build_codec(
            vocab_config=vocabularies.VocabularyConfig(num_velocity_bins=num_velocity_bins))
        self.vocabulary = vocabularies.vocabulary_from_codec(self.codec)
        self.output_features = {"inputs": None, "targets": self.vocabulary}

        base = config or network.T5Config()
        self.model_config = network.T5Config(**{
            **{f: getattr(base, f) for f in base.__dataclass_fields__},
            "vocab_size": vocabularies.num_embeddings(self.vocabulary), "dtype": dtype,
            "input_depth": spectrograms.input_depth(self.spectrogram_config)})
        self._params = None
        self.last_event_counts = None            # invalid_events / dropped_events of the most recent transcribing call
        self.model = network.Transformer(self.model_config, input_length=self.inputs_length,
                                         max_decode_length=self.outputs_length, max_batch=self.batch_size)
        self.restore_from_checkpoint(checkpoint_path)

    @property
    def input_shapes(self):
        return {"encoder_input_tokens": (self.batch_size, self.inputs_length),
                "decoder_input_tokens": (self.batch_size, self.outputs_length)}

    def restore_from_checkpoint(self, checkpoint_path):
        """Weights: a t5x checkpoint DIRECTORY (what the reference restores: msgpack index + one zarr
        array per `target.*` parameter, read by mt3_amd.checkpoints), a flat `.npz` (names = the
        reference's Flax tree joined by '/'; or the int8 form of checkpoints.save_compact_npz), a dict of arrays, or 'random:<seed>' / None for the
        reference's initialisers (no checkpoint ships with the repo)."""
        rnd = None if checkpoint_path is None or isinstance(checkpoint_path, dict) else \
            re.fullmatch(r"random(?::(\d+))?", str(checkpoint_path))
        if isinstance(checkpoint_path, dict):
            params = checkpoint_path
        elif checkpoint_path is not None and os.path.isdir(str(checkpoint_path)):      # real paths win over 'random'
            from . import checkpoints
            params = checkpoints.load_t5x_checkpoint(str(checkpoint_path),
                                                     expected=network.param_shapes(self.model_config))
        elif checkpoint_path is not None and str(checkpoint_path).endswith(".npz") and \
                os.path.exists(str(checkpoint_path)):
            with np.load(str(checkpoint_path)) as z:
                compact = any(k.endswith("|q") for k in z.files)      # checkpoints.save_compact_npz: int8 + per-column scales
                params = None if compact else {k: z[k] for k in z.files}
            if compact:
                from . import checkpoints
                params = checkpoints.load_compact_npz(str(checkpoint_path))
        elif checkpoint_path is None or rnd:
            params = network.init_random_params(self.model_config, seed=int(rnd.group(1) or 0) if rnd else 0)
        else:
            raise ValueError("unsupported checkpoint %r: pass a t5x checkpoint directory, a flat .npz, a dict, "
                             "or 'random:<seed>'"
                             % (checkpoint_path,))
        self._params = params                    # kept: the engine is rebuilt with more slots when a job asks for them
        self.model.load_params(params)

    @property
    def engine_slots(self) -> int:
        return self.model.max_batch

    def _ensure_slots(self, n_segments: int):
        """the engine sized to the job: min(n_segments, max_slots) decode slots, in powers of two so that a run of files
        of similar length rebuilds it once (the attribute `batch_size` does not change)"""
        want = min(max(n_segments, self.batch_size), self.max_slots)
        if want <= self.model.max_batch:
            return
        slots = self.batch_size
        while slots < want:
            slots *= 2
        slots = min(slots, self.max_slots)
        # the old engine goes FIRST: two engines' K/V caches must never be resident together (12.8 GB each in f32 at 256
        # slots, MT3 shape) -- Transformer.__del__ destroys the engine as soon as the last reference is dropped
        self.model = None
        self.model = network.Transformer(self.model_config, input_length=self.inputs_length,
                                         max_decode_length=self.outputs_length, max_batch=slots)
        self.model.load_params(self._params)

    # ------------------------------------------------------------------ constrained decoding
    def _token_masks(self, programs, drums, segments_per_file=None):
        """The `programs=` / `drums=` keywords of the transcribing methods -> None (unconstrained) or (masks uint32
        [n_masks, words], per-segment mask index or None).  programs: the MIDI programs the transcription may use (None:
        any); drums=False forbids drum notes.  segments_per_file (the `_many` / `wavs` forms): either keyword may then hold
        one entry per file -- programs=[[0], [33]], drums=[True, False] -- and every segment of a file carries its file's
        mask index (-1 for a file without a constraint)."""
        files = len(segments_per_file) if segments_per_file is not None else 0
        listy = (lambda v: isinstance(v, (list, tuple, np.ndarray)))
        per_file = segments_per_file is not None and (
            listy(drums) or (listy(programs) and any(p is None or listy(p) for p in programs)))
        if not per_file:
            if listy(drums):
                raise ValueError("drums must be one bool for a single file")
            if programs is None and drums:
                return None
            return self._mask_rows([(programs, drums)]), None
        prog = list(programs) if listy(programs) and any(p is None or listy(p) for p in programs) else [programs] * files
        drum = list(drums) if listy(drums) else [drums] * files
        if len(prog) != files or len(drum) != files:
            raise ValueError("programs / drums per file: %d / %d entries for %d files" % (len(prog), len(drum), files))
        keys, index = [], []
        for p, d in zip(prog, drum):
            key = (None if p is None else tuple(sorted(set(int(v) for v in p))), bool(d))
            if key == (None, True):
                index.append(-1)
                continue
            if key not in keys:
                keys.append(key)
            index.append(keys.index(key))
        if not keys:
            return None
        seg = np.repeat(np.asarray(index, np.int32), np.asarray(segments_per_file, np.int64))
        return self._mask_rows(keys), seg

    def _mask_rows(self, constraints):
        try:
            self.codec.event_type_range("program")
        except ValueError:
            raise ValueError("programs= / drums= need a vocabulary with program tokens") from None
        return np.stack([vocabularies.token_mask(self.codec, self.model_config.vocab_size,
                                                 None if p is None else list(p), bool(d)) for p, d in constraints])

    @staticmethod
    def _segment_prompts(prompts, n_segments: int):
        """The `prompts=` keyword for one file of `n_segments` segments -> None (no prompt at all) or a list with one
        entry per segment, an id list or None.  prompts: a sequence with one entry per segment -- an id sequence (the
        segment's output begins with it: `vocabularies.tie_section_prompt`), or None / empty for none; a shorter sequence
        is padded with None, a longer one raises ValueError."""
        if prompts is None:
            return None
        rows = [None if p is None or len(p) == 0 else [int(v) for v in p] for p in prompts]
        if len(rows) > n_segments:
            raise ValueError("prompts has %d entries; the audio has %d segments" % (len(rows), n_segments))
        rows += [None] * (n_segments - len(rows))
        return rows if any(r is not None for r in rows) else None

    def _max_steps(self) -> int:
        """a segment's length in steps of the codec: 204 for `mt3`, 409 for `ismir2021`"""
        cfg = self.spectrogram_config
        return int(math.floor(self.inputs_length * cfg.hop_width / cfg.sample_rate * self.codec.steps_per_second))

    def token_grammar(self):
        """the event grammar of this model's codec, spec and segment length (`vocabularies.token_grammar`): max_steps is
        the segment's length in steps, 204 for `mt3` and 409 for `ismir2021`"""
        return vocabularies.token_grammar(self.codec, self.model_config.vocab_size, self.encoding_spec, self._max_steps())

    def note_grammar(self):
        """the note grammar of this model's codec, spec and segment length (`vocabularies.note_grammar`); ValueError for a
        spec without a tie section"""
        return vocabularies.note_grammar(self.codec, self.model_config.vocab_size, self.encoding_spec, self._max_steps())

    def _job(self, segments_per_file, many: bool, *, programs=None, drums=True, prompts=None, well_formed=False,
             **rule) -> _Job:
        """The job of one transcribing call, from its public keywords and the segments of its files.  many: the `_many` /
        `wavs` forms -- programs / drums may hold one entry per file, prompts holds one sequence per file, and a segment's
        noise stream is its index within its own file; else one file, one constraint, one prompt sequence.  rule: `draws`,
        and the `decoding` / `sampling` of this job where they are not the model's.  Everything is checked here, before
        anything is set on the engine."""
        if isinstance(well_formed, str) and well_formed not in ("notes", "tied"):
            raise ValueError('well_formed is False, True, "notes" or "tied", got %r' % (well_formed,))
        tied = isinstance(well_formed, str) and well_formed == "tied"
        masks = self._token_masks(programs, drums, segments_per_file if many else None)
        rows = None
        if prompts is not None:
            per_file = prompts if many else [prompts]
            if len(per_file) != len(segments_per_file):
                raise ValueError("prompts has %d entries for %d files" % (len(per_file), len(segments_per_file)))
            rows = []
            for p, n in zip(per_file, segments_per_file):
                rows += self._segment_prompts(p, n) or [None] * n
            rows = rows if any(r is not None for r in rows) else None
        if tied:
            if rows is not None:
                raise ValueError('well_formed="tied" writes every segment\'s prompt itself: not together with prompts=')
            if 2 * self.cap + 1 >= self.outputs_length:
                raise ValueError('well_formed="tied": a tie section of cap = %d pairs (%d ids) leaves no room in a decode '
                                 "of %d steps" % (self.cap, 2 * self.cap + 1, self.outputs_length))
        if well_formed == "notes" or tied:
            grammar = self.note_grammar()
        else:
            grammar = self.token_grammar() if well_formed else None
        streams = np.concatenate([np.arange(n) for n in segments_per_file]) if many else None
        return _Job(rule.pop("decoding", None) or self.decoding, rule.pop("sampling", None) or self.sampling,
                    *(masks or (None, None)), prompts=rows, grammar=grammar, tied=tied, streams=streams, **rule)

    @contextlib.contextmanager
    def _engine_job(self, job: _Job):
        """the engine calls of `job` run inside; what the job set on the engine is cleared on the way out, also on error"""
        try:
            yield
        finally:
            if self.model is not None:
                if job.tied:
                    self.model.set_prompts(None)
                if isinstance(job.grammar, _lib.NoteGrammar):
                    self.model.clear_note_grammar()
                elif job.grammar is not None:
                    self.model.clear_token_grammar()
                if job.masks is not None:
                    self.model.clear_token_masks()
                if job.prompts is not None:
                    self.model.set_prompts(None)
                if job.decoding == "sample":
                    self.model.clear_sampling()

    def _set_masks(self, job: _Job, lo: int, hi: int, per: int = 0):
        """before an engine call on segments [lo, hi) of `job`: their masks and prompts on the engine that will run it.
        per > 0 (Transformer.transcribe(draws=per)): the tables of the job's draws -- every segment's mask index, prompt
        and stream `per` times in a row, and draw j of every segment under the seed (seed + j) mod 2^64."""
        rep = max(int(per), 1)
        if job.masks is not None:
            seg = job.mask_index
            self.model.set_token_masks(job.masks, None if seg is None else np.repeat(np.asarray(seg[lo:hi]), rep))
        if job.prompts is not None:
            rows, index = [], []
            for p in job.prompts[lo:hi]:
                if p is None:
                    index.append(-1)
                    continue
                if p not in rows:
                    rows.append(p)
                index.append(rows.index(p))
            self.model.set_prompts(rows, list(np.repeat(np.asarray(index, np.int32), rep)) if rows else None)
        if isinstance(job.grammar, _lib.NoteGrammar):
            self.model.set_note_grammar(job.grammar)
        elif job.grammar is not None:
            self.model.set_token_grammar(job.grammar)
        if job.decoding == "sample":
            # the stream of a segment is its index within its own file, whatever else the job or the engine call holds
            streams = job.streams[lo:hi] if job.streams is not None else np.arange(lo, hi)
            streams = np.repeat(np.asarray(streams, dtype=np.uint64), rep)
            seeds = None
            if per:
                seeds = np.tile(np.array([(job.sampling.seed + j) % (1 << 64) for j in range(rep)], dtype=np.uint64), hi - lo)
            self.model.set_sampling(job.sampling, streams, seeds)

    # ------------------------------------------------------------------ model call
    def predict_tokens(self, batch: Dict[str, Any], seed: int = 0) -> np.ndarray:
        """batch['encoder_input_tokens']: f32 [B, T, 512] (numpy or CUDA tensor) -> int32 [B, 1024]
        with -1 from EOS on and -2 for invalid ids (vocabulary.decode_tf)."""
        return self.vocabulary.decode_tf(self._predict_ids(batch)).cpu().numpy()

    def _predict_ids(self, batch: Dict[str, Any], job: Optional[_Job] = None, overflows: Optional[list] = None):
        """the engine's side of `predict_tokens`: the raw vocabulary ids, int32 CUDA [B, 1024].  Every decode reaches the
        engine through here.  job: what to set on the engine for it (None: nothing but the model's own decoding rule);
        whoever built the job clears it (`_engine_job`).  overflows: a list that a tied job appends its count to."""
        import torch
        x = batch["encoder_input_tokens"]
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, np.float32))
        x = x.cuda()
        job = job if job is not None else _Job(self.decoding, self.sampling)
        if job.tied:
            return self._predict_ids_tied(x, job, overflows)
        beam1 = job.decoding == "beam1"
        if job.decoding == "beam":
            return self._predict_ids_beam(x, job)
        if self.schedule == "refill" and self.early_exit and job.draws:
            # ONE engine call for all draws of the job's segments, each segment encoded once; row s * per + j = draw j
            per, n = int(job.draws), int(x.shape[0])
            self._ensure_slots(n * per)
            self.rows_per_engine_call = [n * per]
            self._set_masks(job, 0, n, per)
            return self.model.transcribe(x, draws=per)
        if self.schedule == "refill" and self.early_exit:
            # ONE engine call for the whole job: finished rows restart on the job's next segments
            self._ensure_slots(x.shape[0])
            self.rows_per_engine_call = [int(x.shape[0])]
            self._set_masks(job, 0, int(x.shape[0]))
            return self.model.transcribe(x, beam1=beam1)
        out = []
        step = min(self.batch_size, self.model.max_batch)
        self.rows_per_engine_call = []
        for s in range(0, x.shape[0], step):
            self.model.encode(x[s:s + step])
            self._set_masks(job, s, s + step)
            out.append(self.model.decode(early_exit=self.early_exit, beam1=beam1))
            self.rows_per_engine_call.append(int(min(step, x.shape[0] - s)))
        return torch.cat(out, 0)

    def _predict_ids_tied(self, x, job: _Job, overflows: Optional[list]):
        """well_formed="tied": the job as a wavefront.  Pass j decodes segment j of every file that has one through
        `_predict_ids` -- a job of its own: this one's masks, streams and decoding rule sliced to the pass's rows -- with
        segment 0 forced to the bare `tie` and segment j + 1 forced to `Transformer.tie_prompts` of the file's row from
        pass j."""
        import torch
        N = int(x.shape[0])
        seg = np.asarray(job.streams if job.streams is not None else np.arange(N), np.int64)
        ids = torch.empty((N, self.outputs_length), device=x.device, dtype=torch.int32)
        carried = {}                             # job row of segment j -> the prompt of the file's segment j + 1
        bare = [int(job.grammar.g.tie_id)]
        calls, over = [], 0
        for j in range(int(seg.max()) + 1 if N else 0):
            rows = np.flatnonzero(seg == j)
            one = dataclasses.replace(                                           # the pass itself takes the plain path
                job, tied=False, streams=seg[rows], prompts=[bare if j == 0 else carried[r - 1] for r in rows],
                mask_index=None if job.mask_index is None else np.asarray(job.mask_index)[rows])
            at = torch.from_numpy(rows).to(x.device)
            out = self._predict_ids({"encoder_input_tokens": x.index_select(0, at)}, one)
            ids.index_copy_(0, at, out)
            calls += self.rows_per_engine_call
            go_on = [i for i, r in enumerate(rows) if r + 1 < N and seg[r + 1] == j + 1]
            if not go_on:
                continue
            src = out if len(go_on) == len(rows) else out.index_select(0, torch.tensor(go_on, device=x.device))
            prompts, counts = self.model.tie_prompts(src, job.grammar, self.cap, self.drop_redundant_programs)
            prompts, counts = prompts.cpu().numpy(), counts.cpu().numpy()
            over += int((counts > self.cap).sum())
            carried = {int(rows[i]): ties.prompt_ids(p) for i, p in zip(go_on, prompts)}
        self.rows_per_engine_call = calls
        if overflows is not None:
            overflows.append(over)
        return ids

    def _predict_ids_beam(self, x, job: _Job):
        """decoding='beam', k engine rows (beams) per segment: one in-flight batched call (schedule='refill'), or
        batch-synchronous chunks of max_slots // k segments (schedule='batch')"""
        import torch
        k = self.num_beams
        chunk = max(1, self.max_slots // k)
        self._ensure_slots(min(x.shape[0], chunk) * k)
        if self.schedule == "refill" and self.early_exit:
            # ONE engine call for the whole job: a closed element restarts on the job's next segment
            self.rows_per_engine_call = [int(x.shape[0]) * k]
            self._set_masks(job, 0, int(x.shape[0]))
            return self.model.transcribe(x, num_beams=k)
        chunk = max(1, min(chunk, self.model.max_batch // k))
        out = []
        self.rows_per_engine_call = []
        for s in range(0, x.shape[0], chunk):
            self.model.encode(x[s:s + chunk], num_beams=k)
            self._set_masks(job, s, s + chunk)
            ids, _ = self.model.decode_beams(k, early_exit=self.early_exit)
            out.append(ids)
            self.rows_per_engine_call.append(int(min(chunk, x.shape[0] - s)) * k)
        return torch.cat(out, 0)

    def __call__(self, audio, sample_rate: int = SAMPLE_RATE, *, programs=None, drums: bool = True, prompts=None,
                 well_formed: bool = False, velocities=None, beats=False, harmony=False):
        """1-d array of samples at `sample_rate` -> NoteSequence.  At 16 kHz (the default) the samples go straight to the
        frontend; at any other rate they are resampled on the device first (`_device_examples`), which replaces the
        notebook's host `wav_data_to_samples_librosa(wav, sample_rate=16000)`.
        programs / drums (every transcribing method takes them): constrained decoding -- programs=[0, 33] lets the
        decode use those MIDI programs only, drums=False forbids drum notes; the excluded tokens are impossible at the
        token pick (Transformer.set_token_masks), so the search takes the best ALLOWED continuation.
        prompts (every transcribing method but the scoring-only ones takes it): prompted decoding -- one entry per segment,
        an id sequence the segment's output must begin with (`vocabularies.tie_section_prompt(codec, notes)`: the notes
        still sounding when the segment starts; `tie_section_prompt(codec, [])`: a known silent start) or None / empty for
        none; shorter than the segments: padded with None, longer: ValueError.  The decode continues from the prompt
        (Transformer.set_prompts) and the notes are read from prompt + continuation.  Composes with programs / drums.
        well_formed (every transcribing method takes it; default off): well-formed decoding -- the token pick follows the
        event grammar of the model's codec (Transformer.set_token_grammar), so no token is spent on a shift that runs
        backwards or past the segment's end, a `tie` outside the tie section or a malformed tie section, which the note
        decoder would count in invalid_events / dropped_events and throw away.  Composes with the rest.
        well_formed="notes": that rule plus the set of sounding notes (Transformer.set_note_grammar): no note-off of a
        pitch that is not sounding on the current program, no pair declared twice in a tie section, no drum at velocity 0.
        ValueError for a model whose spec has no tie section.  True keeps the event grammar alone, and its bits.
        well_formed="tied": the note rule, and every segment's tie section forced to what the file's previous segment left
        sounding (`Transformer.tie_prompts`; the bare `tie` for a file's first segment) -- the decoding mode under which the
        model sees at inference the tie sections it was trained with, and the host note decoder and the engine hold the
        same set of notes at every segment boundary.  The job runs as a wavefront: pass j decodes segment j of every file
        (`transcribe_many` / `transcribe_wavs`: all files' segment j in one engine call), so one file alone decodes its
        segments one after another.  A tie section declares at most `cap` pairs (the model's keyword; default 64).
        ValueError with prompts=, for a spec without a tie section, or when 2 * cap + 1 >= the decode length.
        `last_event_counts` holds the note decoder's invalid_events / dropped_events of the most recent call and
        tie_overflows, the segments whose held set exceeded `cap` on its way into the next (0 unless "tied").
        velocities (`__call__`, `transcribe_many`, `transcribe_wav`, `transcribe_wavs`; default None: off, and every bit
        stays where it is): note velocities from the log-mel this job's decode has just read, still on the device
        (`velocity.estimate`) -- the one-velocity-bin codec gives every note the same velocity (127); with
        True, or a dict of `estimate`'s keywords (window, harmonics, gamma, quantile, anchor_velocity), each note's
        velocity is its level at the onset relative to the file's median note.  Nothing else of the notes changes.  ValueError for a model whose
        codec has more than one velocity bin (ismir2021): it decodes them.  For known notes: `note_velocities`.
        beats (the same four methods; default False: off, and nothing changes): with True, or a dict of `beats.track`'s
        keywords (prior_bpm, tightness, width), the job's notes go through the beat tracker on the device (one
        `mt3_amd.beats.track` call for all files) and every returned NoteSequence carries the attribute
        `beats`, its file's `mt3_amd.beats.Beats` (times, period, qpm, score).  The notes themselves do not change;
        `midi_io.note_sequence_to_midi_bytes(ns, beats=ns.beats.times)` writes them with the tempo map.  For known notes:
        `InferenceModel.beats`.
        harmony (the same four methods; default False: off, and nothing changes): with True, or a dict of
        `harmony.analyze`'s keywords (change_penalty, onset_weight, change_weight, bass_weight), the beats are tracked
        (it implies beats=True; a dict given as beats= still sets the tracker's keywords) and the job's notes and beats go
        through one `mt3_amd.harmony.analyze` call for all files: every returned NoteSequence also carries
        `harmony`, its file's `mt3_amd.harmony.Harmony` (key, chords per beat, beats_per_bar, downbeats, segments).
        `midi_io.note_sequence_to_midi_bytes(ns, beats=ns.beats.times, harmony=ns.harmony)` writes the signatures and the
        chord markers.  For known notes: `InferenceModel.harmony`."""
        return self._transcribe([functools.partial(self._examples, audio, sample_rate)], False,
                                dict(programs=programs, drums=drums, prompts=prompts, well_formed=well_formed),
                                velocities=velocities, beats=beats, harmony=harmony)[0]

    def _transcribe(self, make_examples, many: bool, kw, *, scored: bool = False, velocities=None, beats=False,
                    harmony=False, **rule):
        """The one path from files to notes.  make_examples: one call per file that returns (its examples, its log-mel on
        the device); many and kw (programs, drums, prompts, well_formed) as `_job` reads them; rule: `_job`'s -- with
        draws=n the segments' n draws run as one job (row s * n + j of the job = draw j of segment s).  -> per file its
        NoteSequence; with draws the list of its n NoteSequences; with scored (one file) the pair (NoteSequence, scores).
        All segments go through the engine as one job, and the job's tables are cleared on the way out.  velocities (not
        with draws): the keywords of `velocity.estimate`, run on the job's log-mel after the decode, while it is still on
        the device."""
        import torch
        velocities = self._velocity_keywords(velocities)
        harmony = self._harmony_keywords(harmony)
        beats = self._beat_keywords(True if harmony is not None and (beats is None or beats is False) else beats)
        if harmony is not None and (scored or rule.get("draws")):
            raise ValueError("harmony= is for the transcribing methods that return one NoteSequence per file")
        if beats is not None and (scored or rule.get("draws")):
            raise ValueError("beats= is for the transcribing methods that return one NoteSequence per file")
        files = [make() for make in make_examples]
        if not files:
            return []
        per_file = [examples for examples, _ in files]
        job = self._job([len(examples) for examples in per_file], many, **kw, **rule)
        # the frontend kernel has already written the feature converter's form of every segment -- [T, 512] rows, 0.0
        # after a short last segment's frames (mt3/models.py:48-98 via models.convert_features) -- and it is still on the
        # device: no host round trip between the frontend and the engine
        x = files[0][1] if len(files) == 1 else torch.cat([logmel for _, logmel in files], 0)
        del files
        to_ns = metrics_utils.event_predictions_to_ns_traced if scored else metrics_utils.event_predictions_to_ns
        n, overflows = int(job.draws or 1), []
        with self._engine_job(job):
            ids = self._predict_ids({"encoder_input_tokens": x}, job, overflows)
            tokens = self.vocabulary.decode_tf(ids).cpu().numpy()
            out, at, results = [], 0, []
            for examples in per_file:
                runs = []
                for j in range(n):
                    rows = tokens[at * n + j:(at + len(examples)) * n:n]
                    preds = [self.postprocess(t, ex) for t, ex in zip(rows, examples)]
                    results.append(to_ns(preds, codec=self.codec, encoding_spec=self.encoding_spec))
                    runs.append(results[-1]["est_ns"])
                at += len(examples)
                out.append(runs if job.draws else runs[0])
            self._count_events(results, sum(overflows))
            if velocities is not None:
                from . import velocity
                # each file's rows of x beside its frame count: a short last segment's zero rows are not the file's
                at = note_arrays.offsets([len(examples) for examples in per_file])
                out = velocity.estimate(
                    [(x[at[f]: at[f + 1]], sum(len(ex["input_times"]) for ex in examples))
                     for f, examples in enumerate(per_file)], out,
                    frames_per_second=self.spectrogram_config.frames_per_second, **velocities)
            if scored:
                out = [(out[0], self._note_scores(x, ids, results[0]["note_tokens"]))]
        if beats is not None:
            from . import beats as beat_tracking
            for ns, found in zip(out, beat_tracking.track(out, **beats)):
                ns.beats = found
        if harmony is not None:
            from . import harmony as harmony_analysis
            for ns, found in zip(out, harmony_analysis.analyze(out, [ns.beats for ns in out], **harmony)):
                ns.harmony = found
        return out

    @staticmethod
    def _harmony_keywords(harmony):
        """the `harmony=` keyword of the transcribing methods -> `harmony.analyze`'s keywords, or None for off"""
        if harmony is None or harmony is False:
            return None
        if harmony is True:
            return {}
        unknown = set(harmony) - {"change_penalty", "onset_weight", "change_weight", "bass_weight"}
        if unknown:
            raise ValueError("harmony= takes change_penalty, onset_weight, change_weight, bass_weight, got %s"
                             % ", ".join(sorted(map(repr, unknown))))
        return dict(harmony)

    @staticmethod
    def _beat_keywords(beats):
        """the `beats=` keyword of the transcribing methods -> `beats.track`'s keywords, or None for off"""
        if beats is None or beats is False:
            return None
        if beats is True:
            return {}
        unknown = set(beats) - {"prior_bpm", "tightness", "width"}
        if unknown:
            raise ValueError("beats= takes prior_bpm, tightness, width, got %s" % ", ".join(sorted(map(repr, unknown))))
        return dict(beats)

    def _velocity_keywords(self, velocities):
        """the `velocities=` keyword of the transcribing methods -> `velocity.estimate`'s keywords, or None for off"""
        if velocities is None or velocities is False:
            return None
        if self.num_velocity_bins > 1:
            raise ValueError("velocities= is for a codec with one velocity bin: this model decodes its %d velocity bins"
                             % self.num_velocity_bins)
        if velocities is True:
            return {}
        unknown = set(velocities) - {"window", "harmonics", "gamma", "quantile", "anchor_velocity"}
        if unknown:
            raise ValueError("velocities= takes window, harmonics, gamma, quantile, anchor_velocity, got %s"
                             % ", ".join(sorted(map(repr, unknown))))
        return dict(velocities)

    def _draws_in_one_job(self, well_formed) -> bool:
        """whether `sample` runs its draws as one engine job: the refill schedule, and not well_formed="tied" (whose
        wavefront carries one tie chain per decode)"""
        tied = isinstance(well_formed, str) and well_formed == "tied"
        return self.schedule == "refill" and self.early_exit and not tied

    def _check_sample(self, num_samples):
        if int(num_samples) < 1:
            raise ValueError("num_samples must be at least 1, got %r" % (num_samples,))
        if self.decoding == "beam":
            raise ValueError("sample() draws on the greedy path: not for a model with decoding='beam'")

    def sample(self, audio, num_samples: int = 1, sample_rate: int = SAMPLE_RATE, **kw):
        """`num_samples` transcriptions of the same audio, drawn with seeds seed .. seed + num_samples - 1 of the model's
        sampling parameters (the job's decoding is 'sample', whatever the model's own decoding is) -> a list
        of NoteSequences, sample j equal note for note to a model with seed + j called on the audio.  kw: the keywords of
        `__call__` (programs, drums, prompts, well_formed).
        The samples are ONE engine job (Transformer.transcribe(draws=num_samples)): the frontend and the encoder run once,
        draw j of every segment decodes under the seed (seed + j) mod 2^64 in a slot of its own, and the engine is sized
        to min(segments * num_samples, max_slots).  well_formed="tied" keeps a loop of num_samples decodes: its wavefront
        carries one tie chain per decode (so does schedule='batch' / early_exit=False, which have no in-flight job)."""
        self._check_sample(num_samples)
        make = [functools.partial(self._examples, audio, sample_rate)]
        if self._draws_in_one_job(kw.get("well_formed", False)):
            return self._transcribe(make, False, kw, decoding="sample", draws=int(num_samples))[0]
        return self._sample_loop(lambda **rule: self._transcribe(make, False, kw, **rule)[0], num_samples)

    def _sample_loop(self, run, num_samples):
        """where the draws are no single engine job: run(decoding=, sampling=) once per sample, sample j under the
        model's sampling parameters with the seed (seed + j) mod 2^64 -> the list of what the runs return"""
        return [run(decoding="sample", sampling=dataclasses.replace(self.sampling, seed=(self.sampling.seed + j) % (1 << 64)))
                for j in range(int(num_samples))]

    def sample_many(self, audios: Sequence[Any], num_samples: int = 1, sample_rates: Optional[Sequence[int]] = None,
                    **kw) -> List[List[Any]]:
        """`sample` of several files as ONE job: one list of `num_samples` NoteSequences per file, each equal to
        `sample(audio, num_samples)` of that file.  sample_rates and kw as for `transcribe_many` (programs / drums /
        prompts: one entry per file where they differ).  well_formed="tied": num_samples `transcribe_many` jobs."""
        self._check_sample(num_samples)
        make = [functools.partial(self._examples, audio, sr) for audio, sr in zip(audios, self._rates(sample_rates, len(audios)))]
        if self._draws_in_one_job(kw.get("well_formed", False)):
            return self._transcribe(make, True, kw, decoding="sample", draws=int(num_samples))
        runs = self._sample_loop(lambda **rule: self._transcribe(make, True, kw, **rule), num_samples)
        return [[run[f] for run in runs] for f in range(len(audios))]

    @staticmethod
    def _rates(sample_rates, n: int):
        """the `sample_rates` keyword of the many-file methods for n files: one rate per file, 16 kHz where None"""
        if sample_rates is None:
            return [SAMPLE_RATE] * n
        if len(sample_rates) != n:
            raise ValueError("sample_rates has %d entries for %d files" % (len(sample_rates), n))
        return sample_rates

    def consensus(self, audio, num_samples: int = 8, sample_rate: int = SAMPLE_RATE, *, tolerance: float = 0.05,
                  min_votes: Optional[int] = None, return_votes: bool = False, **kw):
        """The notes that `min_votes` of `num_samples` sampled transcriptions agree on (self-consistency):
        `sample(audio, num_samples, sample_rate, **kw)`, then `consensus.consensus` of those voters on the device -- notes
        of one pitch, program and drum flag whose onsets lie within `tolerance` seconds form a cluster; a cluster that
        min_votes voters (default: a strict majority, num_samples // 2 + 1) take part in becomes one note with the
        cluster's median onset, offset and velocity.  -> the NoteSequence; with return_votes (NoteSequence, the
        `consensus.Consensus` record with votes, members and every sample's per-note votes, the samples).  The seeds and
        the ValueErrors are `sample`'s; the model's own decoding and sampling parameters are left as they were."""
        from . import consensus
        samples = self.sample(audio, num_samples, sample_rate, **kw)
        result = consensus.consensus([samples], tolerance=tolerance, min_votes=min_votes)[0]
        return (result.notes, result, samples) if return_votes else result.notes

    def consensus_many(self, audios: Sequence[Any], num_samples: int = 8, sample_rates: Optional[Sequence[int]] = None, *,
                       tolerance: float = 0.05, min_votes: Optional[int] = None, return_votes: bool = False, **kw):
        """`consensus` of several files: `sample_many(audios, num_samples, sample_rates, **kw)` -- ONE engine job -- then one
        vote per file, all in one `consensus.consensus` call.  -> per file what `consensus` returns for it."""
        from . import consensus
        samples = self.sample_many(audios, num_samples, sample_rates, **kw)
        results = consensus.consensus(samples, tolerance=tolerance, min_votes=min_votes)
        return [(r.notes, r, s) if return_votes else r.notes for r, s in zip(results, samples)]

    def transcribe_wav(self, wav_data, *, programs=None, drums: bool = True, prompts=None, well_formed: bool = False,
                       velocities=None, beats=False, harmony=False):
        """WAV bytes or path -> NoteSequence: the file-level form of `__call__`, equal to `self(*audio_io.read_wav(wav))`
        note for note.  The file's data chunk is uploaded as it is; the PCM decode, the channel mixdown and the resample
        to 16 kHz run on the device in one launch (`_wav_examples`)."""
        return self._transcribe([functools.partial(self._wav_examples, wav_data)], False,
                                dict(programs=programs, drums=drums, prompts=prompts, well_formed=well_formed),
                                velocities=velocities, beats=beats, harmony=harmony)[0]

    def _count_events(self, results, tie_overflows: int):
        """the note decoder's counts of the call that just ended, summed over its files, and its wavefront's overflows"""
        self.last_event_counts = {"invalid_events": int(sum(r["est_invalid_events"] for r in results)),
                                  "dropped_events": int(sum(r["est_dropped_events"] for r in results)),
                                  "tie_overflows": int(tie_overflows)}

    def transcribe_scored(self, audio, sample_rate: int = SAMPLE_RATE, *, programs=None, drums: bool = True,
                          prompts=None, well_formed: bool = False):
        """`__call__` with a confidence for every note: (NoteSequence, scores).  The notes are those of `__call__` (same
        decode: the model's `decoding` and `schedule`); afterwards the decoded id rows are scored teacher-forced in one
        `Transformer.score_segments` call (ids after EOS are 0 = padding; length = the longest row) and each note is
        linked to the tokens that made it (`metrics_utils.event_predictions_to_ns_traced`).  scores: float64 arrays
        aligned with the NoteSequence's notes --
          'onset_logprob'  log-probability of the PITCH / DRUM token that started the note
          'end_logprob'    log-probability of the token that ended it; NaN where no token did (flushed notes, drums)
          'onset_margin'   onset_logprob minus the log-probability of the model's best token at that position: 0 when
                           the decoded token is the model's arg-max, negative otherwise
          'note_tokens'    int64 [n_notes, 2, 2]: (segment, position) of the onset and the end token, (-1, -1) for none
        Not available with e4m3 K/V caches (ValueError, as `score`).  With programs / drums the DECODE is constrained; the
        scores stay the unconstrained model's log-probabilities (scoring ignores token masks).  With prompts the prompt's
        tokens are scored like any other decoded token (scoring ignores prompts)."""
        self._refuse_e4m3("transcribe_scored")
        return self._transcribe([functools.partial(self._examples, audio, sample_rate)], False,
                                dict(programs=programs, drums=drums, prompts=prompts, well_formed=well_formed),
                                scored=True)[0]

    def transcribe_wav_scored(self, wav_data, *, programs=None, drums: bool = True, well_formed: bool = False):
        """The file-level form of `transcribe_scored`: `transcribe_wav` plus the notes' confidences."""
        self._refuse_e4m3("transcribe_wav_scored")
        return self._transcribe([functools.partial(self._wav_examples, wav_data)], False,
                                dict(programs=programs, drums=drums, well_formed=well_formed), scored=True)[0]

    def _refuse_e4m3(self, who):
        if self.model_config.kv_dtype:
            raise ValueError("%s() is not available with kv_dtype=%r: e4m3 K/V caches cannot score"
                             % (who, self.model_config.kv_dtype))

    def _note_scores(self, x, ids, note_tokens):
        """x: the job's log-mel (CUDA); ids: its decoded rows int32 CUDA [N, 1024]; note_tokens [n_notes, 2, 2] ->
        the scores dict of `transcribe_scored`"""
        import torch
        eos = (ids == self.vocabulary.eos_id).int()
        ids = torch.where(torch.cumsum(eos, 1) - eos > 0, torch.zeros_like(ids), ids)      # 0 (padding) after the first EOS
        used = (ids != 0).any(0).nonzero()
        length = int(used.max()) + 1 if used.numel() else 1
        _, tok, _, top = self.model.score_segments(x, ids[:, :length].contiguous(), return_token_scores=True,
                                                   return_top1=True)
        tok, top = tok.cpu().numpy().astype(np.float64), top.cpu().numpy().astype(np.float64)
        seg, pos = note_tokens[:, :, 0], note_tokens[:, :, 1]
        have = seg >= 0
        at = (np.where(have, seg, 0), np.where(have, pos, 0))
        logp = np.where(have, tok[at], np.nan)
        return {"onset_logprob": logp[:, 0], "end_logprob": logp[:, 1],
                "onset_margin": np.where(have[:, 0], tok[at][:, 0] - top[at][:, 0], np.nan), "note_tokens": note_tokens}

    def score(self, audio, targets, return_token_scores: bool = False, *, sample_rate: int = SAMPLE_RATE):
        """Teacher-forced scores of token rows for this audio (t5x score_batch; the reference's infer(mode='score')
        path, which its write_inferences_to_file refuses to write).  The audio goes through the frontend and segmenting
        of `__call__`; targets[i] are the vocabulary ids of segment i in decoder_target_tokens form (EOS included, at
        most 1024).  Returns float64 [n_segments] sequence scores, with return_token_scores also a list of float64
        per-token scores (one array of len(targets[i]) per segment).  sample_rate: as for `__call__`."""
        import torch
        self._refuse_e4m3("score")
        examples, x = self._examples(audio, sample_rate)
        if len(targets) != len(examples):
            raise ValueError("targets has %d rows; the audio has %d segments" % (len(targets), len(examples)))
        rows = [np.asarray(t, np.int32).reshape(-1)[: self.outputs_length] for t in targets]
        n = max([len(r) for r in rows] + [1])
        tgt = np.zeros((len(rows), n), np.int32)
        for i, r in enumerate(rows):
            tgt[i, : len(r)] = r
        seq, tok = [], []
        step = self.model.max_batch
        for s in range(0, len(rows), step):
            self.model.encode(x[s:s + step])
            sc, ts = self.model.score(torch.from_numpy(tgt[s:s + step]), return_token_scores=True)
            seq.append(sc.cpu().numpy().astype(np.float64))
            tok.append(ts.cpu().numpy().astype(np.float64))
        scores = np.concatenate(seq) if seq else np.zeros((0,), np.float64)
        if not return_token_scores:
            return scores
        tok = np.concatenate(tok) if tok else np.zeros((0, n), np.float64)
        return scores, [tok[i, : len(r)] for i, r in enumerate(rows)]

    # ------------------------------------------------------------------ known notes against audio
    def _num_frames(self, audio_or_num_samples, sample_rate: int = SAMPLE_RATE) -> int:
        """the spectrogram frames `__call__` cuts audio of that many samples into (`_audio_to_frames` always pads)"""
        n = int(audio_or_num_samples) if np.ndim(audio_or_num_samples) == 0 else int(np.shape(audio_or_num_samples)[0])
        if int(sample_rate) != SAMPLE_RATE:
            n = audio_io.resampled_length(n, int(sample_rate), SAMPLE_RATE)
        return n // self.spectrogram_config.hop_width + 1

    def _tokenize_kw(self):
        return dict(stride=self.outputs_length, segment_frames=self.inputs_length,
                    frames_per_second=self.spectrogram_config.frames_per_second, vocab_size=self.model_config.vocab_size)

    @staticmethod
    def _sustained(sequences, sustain: bool):
        """sustain: the job's sequences with their sustain pedals applied on the device (`note_prep.prepare`: what the
        reference tokenizes for piano, mt3/preprocessors.py:154), the control changes cleared; else the sequences as given"""
        if not sustain:
            return list(sequences)
        from . import note_prep
        return note_prep.prepare(sequences, sustain=True)

    def _paired_examples(self, pairs, sample_rates, sustain: bool):
        """the (audio, NoteSequence) pairs of a job -> (the pairs with the notes under the sustain pedal if asked, each
        file's log-mel on the device, each file's frame count)"""
        pairs = list(zip([audio for audio, _ in pairs], self._sustained([ns for _, ns in pairs], sustain)))
        feats, n_frames = [], []
        for (audio, _), rate in zip(pairs, sample_rates):
            examples, logmel = self._examples(audio, rate)
            feats.append(logmel)
            n_frames.append(sum(len(ex["input_times"]) for ex in examples))
        return pairs, feats, n_frames

    def targets(self, audio_or_num_samples, ns, *, sample_rate: int = SAMPLE_RATE, granularity: str = "full",
                sustain: bool = False):
        """The training targets of `ns` for this audio (a 1-d array of samples, or just their number): one int32 id row
        per segment of `__call__`, in the form `score` takes -- the tie section, the segment's events, EOS; cut to
        `outputs_length` ids (`tokenize.target_rows`, on the device).  sustain: the sustain pedal of `ns.control_changes`
        is applied to the notes first (`note_prep.prepare`), as the reference does for piano."""
        from . import tokenize
        ns, = self._sustained([ns], sustain)
        rows = tokenize.target_rows([ns], [self._num_frames(audio_or_num_samples, sample_rate)], self.codec,
                                    self.encoding_spec, granularity, **self._tokenize_kw())
        ids, lengths = rows.ids.cpu().numpy(), rows.lengths.cpu().numpy()
        return [ids[i, : lengths[i]].copy() for i in range(len(ids))]

    def score_notes(self, audio, ns, *, sample_rate: int = SAMPLE_RATE, shifts=None, granularity: str = "full",
                    return_note_scores: bool = False):
        """How well do the notes `ns` explain `audio`?  The model's teacher-forced loss on the training targets of `ns`
        (t5x's eval loss of one (audio, MIDI) pair) -> a dict:
          'loss'                minus the sum of the token log-probabilities over all kept ids (EOS included), divided by
                                their number; with shifts: a float64 array, one loss per shift
          'segment_scores'      float64 [n_segments]: the sum of token log-probabilities of each segment (what `score`
                                returns for `targets(audio, ns)`); with shifts: of the best shift
          'token_accuracy'      the share of kept ids that are the model's arg-max at their position
          'truncated_segments'  segments whose targets did not fit `outputs_length` ids (they end without EOS)
          'best_shift'          with shifts: the shift of the lowest loss (the first of equals)
        shifts: offsets in seconds; the notes are scored once per offset, each added to every note time (clamped at 0) --
        all of them tokenized in one launch and scored in one engine call.  granularity: 'full', 'midi_class' or 'flat'.
        return_note_scores: also float64 arrays aligned with `ns.notes` (of the best shift) -- 'onset_logprob' and
        'onset_margin' of the note's onset pitch / drum id as in `transcribe_scored`, 'end_logprob' of its note-off pitch id;
        NaN for an id that was cut or does not exist (a drum has no end).
        Under the sustain pedal of `ns.control_changes`: `score_notes_many([(audio, ns)], sustain=True)[0]`.
        Frontend and segments are those of `__call__`; the rows are built on the device (`tokenize.target_rows`) and go
        straight to `Transformer.score_segments`.  ValueError with e4m3 K/V caches, as `score`."""
        return self.score_notes_many([(audio, ns)], sample_rates=[sample_rate], shifts=shifts, granularity=granularity,
                                     return_note_scores=return_note_scores)[0]

    def score_notes_many(self, pairs, *, sample_rates: Optional[Sequence[int]] = None, shifts=None,
                         granularity: str = "full", return_note_scores: bool = False,
                         sustain: bool = False) -> List[Dict[str, Any]]:
        """`score_notes` of several (audio, NoteSequence) pairs as ONE job: one tokenizer launch and one scoring call over
        the segments of all files (and all shifts).  Returns one dict per pair.  sustain: score the notes as they sound
        under the sustain pedal of each `ns.control_changes` (`note_prep.prepare`, one device call for the job) -- the
        targets a piano model was trained on; the per-note arrays are then aligned with the notes that survive it
        (`note_prep.prepare([ns])[0].notes`)."""
        import torch
        from . import tokenize
        self._refuse_e4m3("score_notes")
        sample_rates = self._rates(sample_rates, len(pairs))
        shift_list = None if shifts is None else [float(s) for s in shifts]
        if shift_list is not None and not shift_list:
            raise ValueError("shifts must not be empty")
        if not pairs:
            return []
        pairs, feats, n_frames = self._paired_examples(pairs, sample_rates, sustain)
        rows = tokenize.target_rows([ns for _, ns in pairs], n_frames, self.codec, self.encoding_spec, granularity,
                                    shifts=shift_list, **self._tokenize_kw())
        table = rows.rows_of_file                            # [files, shifts or 1, (first row, rows)]
        per = table.shape[1]
        seg0 = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])])
        source = np.concatenate([seg0[i] + np.arange(table[i, j, 1]) for i in range(len(pairs)) for j in range(per)])
        group = np.concatenate([np.full(table[i, j, 1], i * per + j) for i in range(len(pairs)) for j in range(per)])
        x = torch.cat(feats, 0)
        if per > 1 or len(source) != x.shape[0]:
            x = x.index_select(0, torch.from_numpy(source).to(x.device))
        width = max(int(rows.lengths.max()), 1)              # 4 bytes back: the width `score` would use
        self._ensure_slots(len(source))
        seq, tok, _, top = self.model.score_segments(x, rows.ids[:, :width].contiguous(), return_token_scores=True,
                                                     return_top1=True)
        kept = torch.arange(width, device=tok.device)[None, :] < rows.lengths[:, None]
        at_best = ((tok == top) & kept).sum(1)
        groups = torch.from_numpy(group).to(tok.device)
        zeros = torch.zeros(len(pairs) * per, device=tok.device, dtype=torch.float64)
        total = zeros.index_add(0, groups, seq.double()).cpu().numpy().reshape(len(pairs), per)
        count = zeros.index_add(0, groups, rows.lengths.double()).cpu().numpy().reshape(len(pairs), per)
        best = zeros.index_add(0, groups, at_best.double()).cpu().numpy().reshape(len(pairs), per)
        cut = zeros.index_add(0, groups, rows.truncated.double()).cpu().numpy().reshape(len(pairs), per)
        seq_host = seq.cpu().numpy().astype(np.float64)
        out = []
        for i, (_, ns) in enumerate(pairs):
            loss = -total[i] / count[i]
            j = int(np.argmin(loss))
            first, n = int(table[i, j, 0]), int(table[i, j, 1])
            rec = {"loss": loss if shift_list is not None else float(loss[0]), "segment_scores": seq_host[first: first + n],
                   "token_accuracy": float(best[i, j] / count[i, j]), "truncated_segments": int(cut[i, j])}
            if shift_list is not None:
                rec["best_shift"] = shift_list[j]
            if return_note_scores:
                note_of = rows.note_of[first: first + n, :width]
                have = (note_of >= 0) & kept[first: first + n]
                which = note_of[have].cpu().numpy()
                onset = rows.is_onset[first: first + n, :width][have].cpu().numpy().astype(bool)
                logp = tok[first: first + n][have].cpu().numpy().astype(np.float64)
                margin = (tok - top)[first: first + n][have].cpu().numpy().astype(np.float64)
                for key in ("onset_logprob", "onset_margin", "end_logprob"):
                    rec[key] = np.full(len(ns.notes), np.nan)
                rec["onset_logprob"][which[onset]] = logp[onset]
                rec["onset_margin"][which[onset]] = margin[onset]
                rec["end_logprob"][which[~onset]] = logp[~onset]
            out.append(rec)
        return out

    def align_notes(self, audio, ns, *, max_shift: float = 0.2, step: float = 0.02, shifts=None, smoothness=None,
                    max_jump=None, sample_rate: int = SAMPLE_RATE, granularity: str = "full", shared_encoder: bool = True,
                    return_table: bool = False, sustain: bool = False):
        """Repair the timing of the notes `ns` against `audio`: a time shift per segment, chosen as the smooth path of the
        highest log-probability through the (segment, shift) table, and the notes warped by it -> a dict:
          'notes'           the warped NoteSequence (`alignment.warp_notes`: the shift is interpolated between the
                            segments' centres and evaluated at each note time; every other field is kept)
          'segment_shifts'  float64 [n_segments]: the path, in seconds
          'path_score'      the path's log-probability minus its jump penalties (smoothness * |jump| per step)
          'flat_shift', 'flat_score'  the best constant path of the same table (one global shift, the lowest of equals)
                            and its log-probability (never above 'path_score')
          'scores'          with return_table: float64 [n_segments, n_shifts], the table
        The shifts are `alignment.shift_grid(max_shift, step)` or `shifts` (strictly increasing seconds, at most 64).
        smoothness: log-probability per second of jump (default `alignment.DEFAULT_SMOOTHNESS`); max_jump: the largest
        jump between neighbouring segments in seconds (default: any).  A grid on which a path may jump by a segment's
        length or more is refused (ValueError).  Every segment is scored under a GLOBAL shift of the notes, so a note
        near a jump may be counted in both neighbouring segments or in neither; the shifts are segment-granular.
        shared_encoder: every segment is encoded once for all shifts (`Transformer.score_candidates`); False: the table
        comes from `score_segments` on the log-mel replicated per shift, as `score_notes` gets it -- the same bits in
        float32.  sustain: the sustain pedal of `ns.control_changes` is applied first (`note_prep.prepare`): the sustained
        notes are aligned, and 'notes' are the sustained notes, warped.  ValueError with e4m3 K/V caches, as `score_notes`."""
        return self.align_notes_many([(audio, ns)], sample_rates=[sample_rate], max_shift=max_shift, step=step,
                                     shifts=shifts, smoothness=smoothness, max_jump=max_jump, granularity=granularity,
                                     shared_encoder=shared_encoder, return_table=return_table, sustain=sustain)[0]

    def align_notes_many(self, pairs, *, sample_rates: Optional[Sequence[int]] = None, max_shift: float = 0.2,
                         step: float = 0.02, shifts=None, smoothness=None, max_jump=None, granularity: str = "full",
                         shared_encoder: bool = True, return_table: bool = False,
                         sustain: bool = False) -> List[Dict[str, Any]]:
        """`align_notes` of several (audio, NoteSequence) pairs as ONE job: one tokenizer launch, one scoring call and one
        path call over the segments of all files.  Returns one dict per pair."""
        import torch
        from . import alignment, tokenize
        self._refuse_e4m3("align_notes")
        sample_rates = self._rates(sample_rates, len(pairs))
        grid = alignment.shift_grid(max_shift, step) if shifts is None else np.asarray(shifts, np.float64).reshape(-1)
        smoothness = alignment.DEFAULT_SMOOTHNESS if smoothness is None else float(smoothness)
        seconds = self.inputs_length / self.spectrogram_config.frames_per_second
        alignment._check([1], 1, grid, smoothness, max_jump)
        alignment.check_jumps(grid, max_jump, seconds)
        if not pairs:
            return []
        pairs, feats, n_frames = self._paired_examples(pairs, sample_rates, sustain)
        K = len(grid)
        rows = tokenize.target_rows([ns for _, ns in pairs], n_frames, self.codec, self.encoding_spec, granularity,
                                    shifts=[float(g) for g in grid], **self._tokenize_kw())
        table = rows.rows_of_file                            # [files, K, (first row, rows)]
        counts = [int(f.shape[0]) for f in feats]
        # the tokenizer's rows are (file, shift, segment); the table is (file, segment, shift)
        order = np.concatenate([(table[i, :, 0][None, :] + np.arange(counts[i])[:, None]).reshape(-1)
                                for i in range(len(pairs))])
        order_dev = torch.from_numpy(order).cuda()
        x = torch.cat(feats, 0)
        width = max(int(rows.lengths.max()), 1)
        if shared_encoder:
            self._ensure_slots(x.shape[0])
            seq = self.model.score_candidates(x, rows.ids.index_select(0, order_dev)[:, :width].contiguous(), K)
        else:
            seg0 = np.concatenate([[0], np.cumsum(counts)])
            source = np.concatenate([seg0[i] + np.arange(counts[i]) for i in range(len(pairs)) for _ in range(K)])
            self._ensure_slots(len(source))
            seq = self.model.score_segments(x.index_select(0, torch.from_numpy(source).to(x.device)),
                                            rows.ids[:, :width].contiguous()).index_select(0, order_dev)
        scores = seq.view(-1, K)
        path, total = alignment.best_paths(scores, counts, grid, smoothness, max_jump)
        flat, flat_total = alignment.best_paths(scores, counts, grid, 0.0, 0.0)      # max_jump 0: the constant paths
        path, total, flat, flat_total = path.cpu().numpy(), total.cpu().numpy(), flat.cpu().numpy(), flat_total.cpu().numpy()
        scores_host = scores.cpu().numpy().astype(np.float64) if return_table else None
        out, first = [], 0
        for i, (_, ns) in enumerate(pairs):
            seg_shifts = grid[path[first: first + counts[i]]]
            rec = {"notes": alignment.warp_notes(ns, seg_shifts, seconds), "segment_shifts": seg_shifts,
                   "path_score": -float(total[i]), "flat_shift": float(grid[flat[first]]), "flat_score": -float(flat_total[i])}
            if return_table:
                rec["scores"] = scores_host[first: first + counts[i]]
            out.append(rec)
            first += counts[i]
        return out

    def transcribe_many(self, audios: Sequence[Any], sample_rates: Optional[Sequence[int]] = None, *, programs=None,
                        drums=True, prompts=None, well_formed: bool = False, velocities=None, beats=False,
                        harmony=False) -> List[Any]:
        """Several files as ONE job (no counterpart in the notebook, which loops `model(audio)` over files): the segments of
        all files go through the engine's decode slots in one refilled call -- a finished slot restarts on the next
        segment, whichever file it belongs to -- and every file's tokens then become notes on their own (the note state
        machine is sequential within a file and independent across files, mt3/metrics_utils.py:92-116).  Returns one
        NoteSequence per file, each identical to `self(audio)`.  sample_rates: one rate per file (default: all 16 kHz),
        as for `__call__`.  programs / drums: as for `__call__`, or one entry per file (programs=[[0], [33]]): every segment
        of a file carries its file's mask, so one job holds files with different instruments.  prompts: one `__call__`-style
        sequence (or None) per file.  velocities: as for `__call__`, one `velocity.estimate` call for the job; every file's
        notes are ranked against its own anchor."""
        return self._transcribe([functools.partial(self._examples, audio, sr)
                                 for audio, sr in zip(audios, self._rates(sample_rates, len(audios)))], True,
                                dict(programs=programs, drums=drums, prompts=prompts, well_formed=well_formed),
                                velocities=velocities, beats=beats, harmony=harmony)

    def transcribe_wavs(self, wavs: Sequence[Any], *, programs=None, drums=True, prompts=None,
                        well_formed: bool = False, velocities=None, beats=False, harmony=False) -> List[Any]:
        """WAV files (bytes or paths) as ONE job: the file-level form of `transcribe_many`, each NoteSequence identical to
        `self.transcribe_wav(wav)`.  programs / drums / prompts / velocities: as for `transcribe_many`."""
        return self._transcribe([functools.partial(self._wav_examples, wav) for wav in wavs], True,
                                dict(programs=programs, drums=drums, prompts=prompts, well_formed=well_formed),
                                velocities=velocities, beats=beats, harmony=harmony)

    def note_velocities(self, audio, ns, *, sample_rate: int = SAMPLE_RATE, **kw):
        """Known notes `ns` with velocities estimated from `audio`: `note_velocities_many([(audio, ns)])[0]`; with
        return_levels the pair (NoteSequence, its record)."""
        out = self.note_velocities_many([(audio, ns)], sample_rates=[sample_rate], **kw)
        return (out[0][0], out[1][0]) if kw.get("return_levels") else out[0]

    def note_velocities_many(self, pairs, *, sample_rates: Optional[Sequence[int]] = None, **kw):
        """(audio, NoteSequence) pairs as one job: the frontend of `__call__` on each audio, then one `velocity.estimate`
        call on the log-mels, which stay on the device -> per pair a new NoteSequence, the notes of `ns` with the velocity
        their level at the onset gives them (a note outside the audio keeps its own).  kw: `estimate`'s keywords (window,
        harmonics, gamma, quantile, anchor_velocity, return_levels).  Any model type: the notes are given, not decoded."""
        from . import velocity
        pairs = list(pairs)
        _, feats, n_frames = self._paired_examples(pairs, self._rates(sample_rates, len(pairs)), False)
        return velocity.estimate(list(zip(feats, n_frames)), [ns for _, ns in pairs],
                                 frames_per_second=self.spectrogram_config.frames_per_second, **kw)

    def synchronize(self, audio, ns, *, sample_rate: int = SAMPLE_RATE, sustain: bool = False, **kw):
        """Synchronise the SCORE `ns` (quantised, another tempo, ritardandi) to the recording `audio`:
        `synchronize_many([(audio, ns)])[0]`, a dict with 'notes' (the NoteSequence in the recording's time), 'path',
        'total', 'mean_cost' and 'tempo_ratio' (`sync.synchronize`).  It composes with `align_notes`: `synchronize` for
        the tempo, then `align_notes` on its 'notes' for the last +-0.2 s."""
        return self.synchronize_many([(audio, ns)], sample_rates=[sample_rate], sustain=sustain, **kw)[0]

    def synchronize_many(self, pairs, *, sample_rates: Optional[Sequence[int]] = None, sustain: bool = False, **kw):
        """(audio, score NoteSequence) pairs as ONE job: the frontend of `__call__` on each audio (no decode is run), then
        one `sync.synchronize` call on the log-mels, which stay on the device: chroma of the audio, chroma of the notes and
        the dynamic-time-warping path of every file, one workgroup per file -> one dict per pair.  kw: `sync.synchronize`'s
        keywords (pool=5, harmonic_weights=(255,), range, floor, fmin, fmax).  sustain: the sustain pedal of
        `ns.control_changes` is applied first (`note_prep.prepare`), as `align_notes` does; 'notes' are then the sustained
        notes, in the recording's time.  Any model type: nothing is decoded."""
        from . import sync
        pairs = list(pairs)
        pairs, feats, n_frames = self._paired_examples(pairs, self._rates(sample_rates, len(pairs)), sustain)
        return sync.synchronize(list(zip(feats, n_frames)), [ns for _, ns in pairs],
                                frames_per_second=self.spectrogram_config.frames_per_second, **kw)

    @staticmethod
    def beats(ns, **kw):
        """The beats of a transcription: `mt3_amd.beats.track([ns], **kw)[0]`, a `Beats` (times in seconds, period in
        10 ms frames, qpm, score), found on the device from the notes' own onsets."""
        from . import beats
        return beats.track([ns], **kw)[0]

    @staticmethod
    def harmony(ns, beats=None, **kw):
        """The harmony and meter of known notes: `mt3_amd.harmony.analyze([ns], [beats], **kw)[0]`, a `Harmony` (key, chord
        per beat, beats_per_bar, downbeats, chord segments).  beats: a `Beats` or beat frames; None: `ns.beats` when the
        notes carry one, else they are tracked first (`InferenceModel.beats(ns)`)."""
        from . import harmony
        if beats is None:
            beats = getattr(ns, "beats", None)
        if beats is None:
            beats = InferenceModel.beats(ns)
        return harmony.analyze([ns], [beats], **kw)[0]

    @staticmethod
    def pianoroll(ns, fps: float = 62.5):
        """The piano roll of a transcription: a float32 CUDA tensor [128, int(fps * last end)], each note's velocity summed
        into its frames (`mt3_amd.pianoroll.pianorolls([ns], fps)[0]`; drum notes are silent, as in pretty_midi's roll)."""
        from . import pianoroll
        return pianoroll.pianorolls([ns], fps)[0]

    @staticmethod
    def render(ns, sample_rate: int = 16000):
        """A transcription as audio, to listen to: a float32 CUDA tensor [n] at `sample_rate`, peak 0.9
        (`mt3_amd.render.render([ns], sample_rate)[0]`; one timbre for every program, a noise burst per drum note)."""
        from . import render
        return render.render([ns], sample_rate)[0]

    # ------------------------------------------------------------------ host preprocessing
    def _examples(self, audio, sample_rate: int):
        """audio at `sample_rate` -> (the examples of `preprocess` without host 'inputs', their log-mel on the device)"""
        if int(sample_rate) == SAMPLE_RATE:
            return self._dataset_examples(self.audio_to_dataset(audio))
        if int(sample_rate) != sample_rate or sample_rate < 1:
            raise ValueError("sample_rate must be a positive integer, got %r" % (sample_rate,))
        return self._device_examples(audio, int(sample_rate))

    def _device_examples(self, audio, sample_rate: int):
        """Native-rate samples: uploaded as float32 and resampled to 16 kHz on the device (audio_io.resample_device, the
        kaiser_best filter of audio_io.resample) straight into the zeroed [n_segments, T*hop] buffer the frontend reads.
        Frames, segment counts and input_times are those `_audio_to_frames` + `preprocess` derive from the 16 kHz samples
        of length n_out (it always pads: n_out // hop + 1 frames).  The examples' 'raw_inputs' are None: the 16 kHz samples
        stay on the device."""
        x = audio if hasattr(audio, "data_ptr") else np.ascontiguousarray(np.asarray(audio).reshape(-1), np.float32)
        n_out = audio_io.resampled_length(x.shape[0], sample_rate, SAMPLE_RATE)
        return self._segment_device_audio(
            n_out, lambda capacity: audio_io.resample_device(x, sample_rate, SAMPLE_RATE, capacity=capacity))

    def _wav_examples(self, wav_data):
        """A WAV file (bytes or path): its data chunk is uploaded as it is and decoded, mixed down and resampled on the
        device (audio_io.read_wav_device) into the buffer `_device_examples` fills, with the same frames, segment counts
        and input_times.  A file audio_io.wav_info does not take is decoded by `read_wav` on the host and goes the way of
        `__call__`."""
        info = audio_io.wav_info(wav_data)
        if info is None:
            return self._examples(*audio_io.read_wav(wav_data))
        n_out = audio_io.resampled_length(info.frames, info.sample_rate, SAMPLE_RATE)
        return self._segment_device_audio(
            n_out, lambda capacity: audio_io.read_wav_device(wav_data, SAMPLE_RATE, capacity)[0])

    def _segment_device_audio(self, n_out: int, fill):
        """n_out 16 kHz samples that fill(capacity) puts at the head of a zero-padded device buffer of `capacity` samples
        -> (examples, log-mel): the buffer is the frontend's [n_segments, T*hop] layout"""
        hop, T = self.spectrogram_config.hop_width, self.inputs_length
        n_frames = n_out // hop + 1
        times = np.arange(n_frames) / self.spectrogram_config.frames_per_second
        counts = self._segment_counts(n_frames)
        audio_dev = fill(len(counts) * T * hop)
        return self._spectrogram_examples(audio_dev.view(len(counts), T * hop), counts, times, None)

    def audio_to_dataset(self, audio):
        frames, frame_times = self._audio_to_frames(audio)
        return {"inputs": frames, "input_times": frame_times}

    def _audio_to_frames(self, audio):
        frame_size = self.spectrogram_config.hop_width
        audio = np.asarray(audio)
        padding = [0, frame_size - len(audio) % frame_size]      # always pads (a full hop if aligned)
        audio = np.pad(audio, padding, mode="constant")
        frames = spectrograms.split_audio(audio, self.spectrogram_config)
        num_frames = len(audio) // frame_size
        times = np.arange(num_frames) / self.spectrogram_config.frames_per_second
        return frames, times

    def preprocess(self, ds) -> List[Dict[str, Any]]:
        """split_tokens_to_inputs_length + add_dummy_targets + compute_spectrograms
        (preprocessors.py:53-57,613-618), batched over all segments in one kernel launch.  The examples carry host
        arrays, as the reference's preprocess returns them; the transcribing methods take `_examples`, whose log-mel
        stays on the device, because the engine reads it there and nothing on that path looks at a host copy."""
        examples, logmel = self._dataset_examples(ds)
        logmel = logmel.cpu().numpy()
        for s, ex in enumerate(examples):
            ex["inputs"] = logmel[s, : len(ex["input_times"])]
        return examples

    def _dataset_examples(self, ds):
        """`preprocess` up to the frontend launch -> (examples with 'inputs' None, their log-mel on the device)"""
        import torch
        frames, times = ds["inputs"], ds["input_times"]
        T, hop = self.inputs_length, self.spectrogram_config.hop_width
        counts = self._segment_counts(len(frames))
        audio = np.zeros((len(counts), T * hop), np.float32)
        for s in range(len(counts)):
            chunk = frames[s * T:(s + 1) * T]
            audio[s, : chunk.size] = chunk.reshape(-1)
        return self._spectrogram_examples(torch.from_numpy(audio).cuda(), counts, times, audio)

    def _segment_counts(self, n_frames: int) -> List[int]:
        """frames of each `inputs_length`-frame segment (split_tokens_to_inputs_length; the last one may be short)"""
        T = self.inputs_length
        return [min(T, n_frames - s) for s in range(0, n_frames, T)]

    def _spectrogram_examples(self, audio_dev, counts, times, audio_host):
        """One frontend launch over the [n_segments, T*hop] device samples -> (the examples, 'inputs' None, and their
        log-mel [n_segments, T, depth] on the device).  The pair is the caller's: nothing is kept on the model.
        audio_host: the same samples on the host for 'raw_inputs' (None: not kept)."""
        T, hop = self.inputs_length, self.spectrogram_config.hop_width
        logmel = spectrograms.compute_spectrogram_batch(audio_dev, counts, self.spectrogram_config)
        return [{"inputs": None, "input_times": times[s * T:(s + 1) * T],
                 "raw_inputs": None if audio_host is None else audio_host[s, : counts[s] * hop],
                 "targets": np.zeros((0,), np.int32)}
                for s in range(len(counts))], logmel

    def postprocess(self, tokens, example):
        tokens = self._trim_eos(tokens)
        start_time = example["input_times"][0]
        start_time -= start_time % (1 / self.codec.steps_per_second)   # float64, as in the notebook
        return {"est_tokens": tokens, "start_time": start_time, "raw_inputs": []}

    @staticmethod
    def _trim_eos(tokens):
        return trim_eos(tokens)


def _varint(buf: bytes, i: int):
    v, shift = 0, 0
    while True:
        if i >= len(buf) or shift > 63:
            raise ValueError("note_sequence_id: truncated or malformed protobuf varint")
        b = buf[i]
        i += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, i
        shift += 7


def note_sequence_id(sequence) -> str:
    """`NoteSequence.id` of the task example's 'sequence' feature (mt3/inference.py:83-86,133: the reference parses the
    serialized proto with note_seq and writes `ref_ns.id`).  Accepts an object with an `.id`, a str (taken as the id),
    or the SERIALIZED proto bytes: `string id = 1` of note_seq's music.proto [field number from memory], read straight
    off the protobuf wire format (tag = field << 3 | wire type; 0 varint, 1 fixed64, 2 length-delimited, 5 fixed32)."""
    if hasattr(sequence, "id"):
        return str(sequence.id)
    if isinstance(sequence, str):
        return sequence
    buf = bytes(sequence)
    i = 0
    while i < len(buf):
        tag, i = _varint(buf, i)
        field, wt = tag >> 3, tag & 7
        if wt == 0:
            _, i = _varint(buf, i)
        elif wt == 1:
            i += 8
        elif wt == 5:
            i += 4
        elif wt == 2:
            n, i = _varint(buf, i)
            if i + n > len(buf):
                raise ValueError("note_sequence_id: length-delimited field runs past the end of the buffer")
            if field == 1:
                return buf[i:i + n].decode("utf-8")
            i += n
        else:
            raise ValueError("note_sequence_id: unsupported protobuf wire type %d" % wt)
    return ""                                     # proto3 default: an unset id is the empty string


class MissingSequenceError(AssertionError, ValueError):
    """A track of the task dataset has no NoteSequence (or a NoteSequence has no track).  The reference trips a bare
    `assert` there (mt3/inference.py:114), so callers that catch AssertionError keep working; it is a real exception
    here, not an assert statement, so `python -O` does not turn it into a KeyError further down."""


def write_inferences_to_file(path: str, inferences: Sequence[Any], task_ds, mode: str, vocabulary=None,
                             vocab_config=None, onsets_only=None, use_ties=None) -> None:
    """mt3/inference.py:34-138: one JSON line {"id", "est_notes": [...]} per track.
    `task_ds`: iterable of dicts with 'input_times', 'unique_id' (and optionally 'raw_inputs', 'sequence');
    `inferences`: one int32 id row per example (model ids, before decode_tf).
    "id": as in the reference (:83-86,133) the `id` of the NoteSequence the track's examples carry in 'sequence'
    (first non-empty one per `unique_id`; every track must then have one: the reference asserts it, :114); a task
    dataset WITHOUT a 'sequence' feature (plain inference, no ground truth) writes the `unique_id` itself."""
    if mode == "score":
        raise ValueError("`score` mode currently not supported in MT3")
    if not vocabulary:
        raise ValueError("`vocabulary` parameter required in `predict` mode")
    if vocab_config is None or onsets_only is None or use_ties is None:
        raise ValueError("vocab_config, onsets_only and use_ties are required")
    if onsets_only and use_ties:
        raise ValueError("ties not compatible with onset-only transcription")
    if onsets_only:
        encoding_spec = note_sequences.NoteOnsetEncodingSpec
    elif not use_ties:
        encoding_spec = note_sequences.NoteEncodingSpec
    else:
        encoding_spec = note_sequences.NoteEncodingWithTiesSpec
    codec = vocabularies.build_codec(vocab_config)

    def first(x):
        x = np.asarray(x)
        return x.reshape(-1)[0] if x.ndim else x[()]

    predictions, ref_ids, any_sequence = [], {}, False
    for inp, output in zip(task_ds, inferences):
        tokens = trim_eos(vocabulary.decode_tf(np.asarray(output, np.int32)))
        start_time = float(first(inp["input_times"]))
        start_time -= start_time % (1 / codec.steps_per_second)
        uid = first(inp["unique_id"])
        uid = uid.decode() if isinstance(uid, bytes) else str(uid)
        if "sequence" in inp:
            any_sequence = True
            seq = inp["sequence"]
            seq = seq if hasattr(seq, "id") or isinstance(seq, (str, bytes)) else first(seq)
            if isinstance(seq, (bytes, str)) and len(seq) == 0:
                seq = None                        # later segments of a track carry an empty string (:85)
            if seq is not None:
                ref_ids[uid] = note_sequence_id(seq)          # (the reference keeps the last one it sees as well, :104-108)
        predictions.append({"unique_id": uid,
                            "est_tokens": tokens, "start_time": start_time,
                            "raw_inputs": inp.get("raw_inputs", [])})
    full = metrics_utils.combine_predictions_by_id(
        predictions, lambda preds: metrics_utils.event_predictions_to_ns(preds, codec=codec,
                                                                         encoding_spec=encoding_spec))
    if any_sequence and sorted(ref_ids.keys()) != sorted(full.keys()):      # the reference asserts it, mt3/inference.py:114
        missing = sorted(set(full) - set(ref_ids))
        extra = sorted(set(ref_ids) - set(full))
        raise MissingSequenceError("write_inferences_to_file: tracks without a NoteSequence in 'sequence': %s; "
                                   "sequences without a track: %s" % (missing[:8], extra[:8]))
    with open(path, "w") as f:
        for uid in sorted(full.keys()):
            notes = [{"start_time": n.start_time, "end_time": n.end_time, "pitch": n.pitch, "velocity": n.velocity,
                      "program": n.program, "is_drum": n.is_drum} for n in full[uid]["est_ns"].notes]
            f.write(json.dumps({"id": ref_ids[uid] if any_sequence else uid, "est_notes": notes}) + "\n")
