"""Vocabulary layer (mirror of mt3/vocabularies.py:29-282) over libmt3hip.so."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Sequence

import numpy as np

from . import _lib
from . import event_codec

DECODED_EOS_ID = -1
DECODED_INVALID_ID = -2
DEFAULT_STEPS_PER_SECOND = 100
DEFAULT_MAX_SHIFT_SECONDS = 10
DEFAULT_NUM_VELOCITY_BINS = 127
DEFAULT_EXTRA_IDS = 100        # t5.data.DEFAULT_EXTRA_IDS (used at vocabularies.py:145)
MAX_MIDI_VELOCITY = 127


@dataclasses.dataclass
class VocabularyConfig:
    steps_per_second: int = DEFAULT_STEPS_PER_SECOND
    max_shift_seconds: int = DEFAULT_MAX_SHIFT_SECONDS
    num_velocity_bins: int = DEFAULT_NUM_VELOCITY_BINS


def num_velocity_bins_from_codec(codec: event_codec.Codec) -> int:
    lo, hi = codec.event_type_range("velocity")
    return hi - lo


def velocity_to_bin(velocity: int, num_velocity_bins: int) -> int:
    return 0 if velocity == 0 else math.ceil(num_velocity_bins * velocity / MAX_MIDI_VELOCITY)


def bin_to_velocity(velocity_bin: int, num_velocity_bins: int) -> int:
    return 0 if velocity_bin == 0 else int(MAX_MIDI_VELOCITY * velocity_bin / num_velocity_bins)


def build_codec(vocab_config: VocabularyConfig) -> event_codec.Codec:
    """shift | pitch | velocity | tie | program | drum, laid out by `mt3_build_codec`."""
    desc = _lib.CodecDesc()
    _lib.check(_lib.load().mt3_build_codec(vocab_config.steps_per_second, vocab_config.max_shift_seconds,
                                           vocab_config.num_velocity_bins, C.byref(desc)))
    return event_codec.Codec.from_desc(desc)


class GenericTokenVocabulary:
    """PAD=0, EOS=1, UNK=2, then `regular_ids` tokens, then `extra_ids` sentinels."""

    def __init__(self, regular_ids: int, extra_ids: int = 0):
        self._num_special_tokens = 3
        self._num_regular_tokens = int(regular_ids)
        self.extra_ids = int(extra_ids)

    pad_id, eos_id, unk_id = 0, 1, 2

    @property
    def _base_vocab_size(self) -> int:
        return self._num_special_tokens + self._num_regular_tokens

    @property
    def vocab_size(self) -> int:
        return self._base_vocab_size + self.extra_ids

    def encode(self, token_ids: Sequence[int]):
        out = []
        for t in token_ids:
            if not 0 <= t < self._num_regular_tokens:
                raise ValueError(f"token_id {t} does not fall within valid range of [0, {self._num_regular_tokens})")
            out.append(int(t) + self._num_special_tokens)
        return out

    def decode(self, ids: Sequence[int]):
        """Python-list path: truncates after the first EOS."""
        row = np.asarray(list(ids), np.int32).reshape(1, -1)
        toks = self.decode_tf(row)[0].tolist()
        return toks[: toks.index(DECODED_EOS_ID) + 1] if DECODED_EOS_ID in toks else toks

    def decode_tf(self, ids):
        """`_decode_tf` (mt3/vocabularies.py:241-271).  A CUDA int32 torch tensor goes through the
        `mt3_ids_to_tokens` kernel (returned as a tensor, no sync: the hot path).  Anything host-side (numpy,
        lists, CPU tensors: the `vocabulary.decode_tf(x).numpy()` use of the notebook and the t5x write_fn in
        inference.py) is remapped on the host with the same three-line rule, so host-only postprocessing needs
        no GPU and empty rows are fine."""
        try:
            import torch
            if isinstance(ids, torch.Tensor) and ids.is_cuda:
                shape, orig_dtype = ids.shape, ids.dtype
                if ids.numel() == 0:
                    return ids.clone()
                t2 = ids.reshape(-1, shape[-1]).to(dtype=torch.int32).contiguous()
                out = torch.empty_like(t2)
                _lib.check(_lib.load().mt3_ids_to_tokens(t2.data_ptr(), t2.shape[0], t2.shape[1],
                                                          self._num_regular_tokens, out.data_ptr(),
                                                          torch.cuda.current_stream().cuda_stream))
                out = out.reshape(shape)
                return out.to(orig_dtype) if orig_dtype != torch.int32 else out
            if isinstance(ids, torch.Tensor):
                return torch.from_numpy(self._decode_host(ids.numpy()))
        except ImportError:
            pass
        return self._decode_host(np.asarray(ids))

    def _decode_host(self, ids: np.ndarray) -> np.ndarray:
        src = np.asarray(ids)
        a = src.astype(np.int64)
        eos = a == self.eos_id
        after = np.cumsum(eos, axis=-1) > 0                     # from the first EOS to the end of the row
        ok = (a >= self._num_special_tokens) & (a < self._base_vocab_size)
        out = np.where(after, DECODED_EOS_ID, np.where(ok, a - self._num_special_tokens, DECODED_INVALID_ID))
        return out.astype(src.dtype if np.issubdtype(src.dtype, np.integer) else np.int32)

    def __eq__(self, other):
        return (self.extra_ids == other.extra_ids and self._num_regular_tokens == other._num_regular_tokens)


def vocabulary_from_codec(codec: event_codec.Codec) -> GenericTokenVocabulary:
    return GenericTokenVocabulary(codec.num_classes, extra_ids=DEFAULT_EXTRA_IDS)


def token_mask(codec: event_codec.Codec, vocab_size: int, programs=None, drums: bool = True) -> np.ndarray:
    """The token mask of a set of instruments (`mt3_codec_token_mask`), uint32 [ceil(vocab_size / 32)]: bit i % 32 of word
    i // 32 set = vocabulary id i allowed.  Every id below `vocab_size` is allowed except the program tokens of programs
    not listed (programs=None: every program stays) and, with drums=False, the drum tokens.  What
    `Transformer.set_token_masks` takes.  ValueError for a program the codec does not hold."""
    mask = np.zeros(((int(vocab_size) + 31) // 32,), np.uint32)
    if programs is None:
        prog, n = None, -1
    else:
        prog = np.ascontiguousarray(list(programs), dtype=np.int32)
        n = int(prog.size)
    lib = _lib.load()
    rc = lib.mt3_codec_token_mask(C.byref(codec.desc), int(vocab_size), prog.ctypes.data if n > 0 else None, n,
                                  1 if drums else 0, mask.ctypes.data)
    if rc != 0:
        raise ValueError(lib.mt3_last_error().decode())
    return mask


def token_grammar(codec: event_codec.Codec, vocab_size: int, spec, max_steps: int) -> _lib.TokenGrammar:
    """The event grammar of `codec` (`mt3_codec_token_grammar`): what `Transformer.set_token_grammar` takes.  spec: a
    `note_sequences` encoding spec or its id (ties: segments open with a tie section); max_steps: the largest shift a
    free pick may take, the segment's length in steps -- floor(input_length * hop_width / sample_rate *
    steps_per_second), 204 for `mt3` and 409 for `ismir2021`.  ValueError for what the library refuses."""
    g = _lib.TokenGrammar()
    lib = _lib.load()
    rc = lib.mt3_codec_token_grammar(C.byref(codec.desc), int(getattr(spec, "spec_id", spec)), int(vocab_size),
                                     int(max_steps), C.byref(g))
    if rc != 0:
        raise ValueError(lib.mt3_last_error().decode())
    return g


def note_grammar(codec: event_codec.Codec, vocab_size: int, spec, max_steps: int) -> _lib.NoteGrammar:
    """The note grammar of `codec` (`mt3_codec_note_grammar`): what `Transformer.set_note_grammar` takes -- the event
    grammar of `token_grammar` plus the codec's velocity and drum ids.  ValueError for what the library refuses, a spec
    without a tie section among it (the notes an earlier segment left sounding are then ended without being declared, which
    a per-segment rule cannot tell from a note-off of a silent pitch)."""
    n = _lib.NoteGrammar()
    lib = _lib.load()
    rc = lib.mt3_codec_note_grammar(C.byref(codec.desc), int(getattr(spec, "spec_id", spec)), int(vocab_size),
                                    int(max_steps), C.byref(n))
    if rc != 0:
        raise ValueError(lib.mt3_last_error().decode())
    return n


def tie_section_prompt(codec: event_codec.Codec, notes, remove_redundant_programs: bool = False) -> list:
    """The vocabulary ids of the tie section that declares `notes`, an iterable of (program, pitch), as still sounding: a
    prompt for `Transformer.set_prompts` / the `prompts=` keyword of the transcribing methods.  It is the section the
    encode side writes for those active notes -- `note_sequences.note_encoding_state_to_events`: a `program, pitch` pair
    per note, sorted by program, then pitch, then `tie` -- as `run_length_encoding.segment_targets` puts it in front of a
    segment, already shifted by the 3 special ids.  No notes: the bare `tie` id (a known silent start).
    remove_redundant_programs: drop a program token equal to the one before it, as `remove_redundant_state_changes`
    does to the targets the model is trained on.  ValueError for a codec without ties (or without the notes' events)."""
    try:
        codec.event_type_range("tie")
    except ValueError:
        raise ValueError("tie_section_prompt needs a codec with a tie event") from None
    E = event_codec.Event
    special = GenericTokenVocabulary(codec.num_classes)._num_special_tokens
    out, last_program = [], None
    for program, pitch in sorted(set((int(p), int(q)) for p, q in notes)):
        if not (remove_redundant_programs and program == last_program):
            out.append(codec.encode_event(E("program", program)) + special)
        last_program = program
        out.append(codec.encode_event(E("pitch", pitch)) + special)
    out.append(codec.encode_event(E("tie", 0)) + special)
    return out


def num_embeddings(vocabulary: GenericTokenVocabulary) -> int:
    return 128 * math.ceil(vocabulary.vocab_size / 128)


# mt3/vocabularies.py:94-117: the NoteSequence side of a program granularity (`program_map_fn`, idempotent); the token
# side (`tokens_map_fn`: drop_programs / programs_to_midi_classes) belongs to the training data pipeline, which is out of
# this path's scope.
PROGRAM_MAP_FNS = {
    "flat": lambda program: 0,                             # programs ignored
    "midi_class": lambda program: 8 * (program // 8),      # first program of the MIDI class
    "full": lambda program: program,
}
