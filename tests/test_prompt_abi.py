"""Prompted decoding on a box without a GPU: the new symbols are exported and typed, mt3_engine_set_prompts refuses every
bad argument with its name in front before it looks at the device, and vocabularies.tie_section_prompt writes the tie
section the encode side writes.

An engine cannot be finalized without a device, so -- as for the token masks (tests/test_token_mask_abi.py) -- the
argument checks come first and "not finalized" last: every argument error is reachable here.  What needs prompts that ARE
set (the status round trip, "a decode is in flight", the decode / transcribe calls' own refusals) is in
tests/test_gpu_prompt_engine.py."""
import ctypes as C
import inspect

import numpy as np
import pytest

from mt3_amd import _lib, event_codec, inference, network, vocabularies
from mt3_amd import note_sequences as NS, run_length_encoding as RLE

NEW = ("mt3_engine_set_prompts", "mt3_op_token_steps_prompted", "mt3_op_beam_search_prompted")
VOCAB, MAX_LEN = 128, 64


def test_the_symbols_are_exported_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.mt3_abi_version() == 4
    assert _lib.STATUS_PROMPTS == 13 and _lib.STATUS_TOKEN_MASKS == 12
    for old, new in (("mt3_op_token_steps_masked", "mt3_op_token_steps_prompted"),
                     ("mt3_op_beam_search_masked", "mt3_op_beam_search_prompted")):
        assert _lib.SIGNATURES[new][1][:-3] == _lib.SIGNATURES[old][1]          # the masked arguments, plus three
    assert hasattr(network.Transformer, "set_prompts")
    for method in ("__call__", "transcribe_wav", "transcribe_scored", "transcribe_many", "transcribe_wavs"):
        p = inspect.signature(getattr(inference.InferenceModel, method)).parameters["prompts"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, method


@pytest.fixture()
def engine():
    lib = _lib.load()
    ec = _lib.EngineConfig(VOCAB, 128, 2, 64, 128, 1, 1, 512, 256, MAX_LEN, 4, _lib.MT3_F32, 0, 0, 0, 0)
    h = C.c_void_p()
    _lib.check(lib.mt3_engine_create(C.byref(ec), C.byref(h)))
    yield lib, h
    lib.mt3_engine_destroy(h)


def _set(lib, h, prompts, seg, stride=None, n=None):
    p = np.ascontiguousarray(prompts, np.int32) if prompts is not None else None
    if p is not None and p.ndim == 1:
        p = p.reshape(1, -1)
    s = np.ascontiguousarray(seg, np.int32) if seg is not None else None
    return lib.mt3_engine_set_prompts(h, p.ctypes.data if p is not None else None,
                                      (0 if p is None else p.shape[0]) if n is None else n,
                                      (0 if p is None else p.shape[1]) if stride is None else stride,
                                      s.ctypes.data if s is not None else None, 0 if s is None else s.size)


def test_set_prompts_refuses_bad_arguments_before_any_device_work(engine):
    lib, h = engine
    ok = [5, 6, 7, 0]
    cases = [
        (dict(prompts=ok, seg=None, n=-1), b"n_prompts must not be negative"),
        (dict(prompts=ok, seg=None, stride=0), b"stride must be at least 1"),
        (dict(prompts=ok, seg=None, stride=-3), b"stride must be at least 1"),
        (dict(prompts=[5] * MAX_LEN, seg=None), b"stride must be below max_decode_len"),
        (dict(prompts=[ok, ok], seg=None), b"several prompts need a per-segment index"),
        (dict(prompts=ok, seg=[0, 1]), b"prompt index outside [-1, n_prompts)"),
        (dict(prompts=ok, seg=[-2]), b"prompt index outside [-1, n_prompts)"),
        (dict(prompts=[5, 1, 7, 0], seg=None), b"a prompt id outside {0} and [2, vocab)"),          # EOS cannot be forced
        (dict(prompts=[5, VOCAB, 7, 0], seg=None), b"a prompt id outside {0} and [2, vocab)"),
        (dict(prompts=[5, -4, 7, 0], seg=None), b"a prompt id outside {0} and [2, vocab)"),
        (dict(prompts=[5, 0, 7, 0], seg=None), b"a non-zero prompt id after a 0"),
        (dict(prompts=[0, 0, 0, 0], seg=None), b"an empty prompt (its first id is 0)"),
        (dict(prompts=[ok, [0, 5, 0, 0]], seg=[0, 1]), b"a non-zero prompt id after a 0"),
        (dict(prompts=[ok, [0, 0, 0, 0]], seg=[0, -1]), b"an empty prompt (its first id is 0)"),
        (dict(prompts=ok, seg=None), b"engine not finalized"),             # nothing wrong with the arguments: the state is next
        (dict(prompts=[ok, [9, 9, 9, 9]], seg=[1, -1, 0]), b"engine not finalized"),
        (dict(prompts=[5] * (MAX_LEN - 1), seg=None), b"engine not finalized"),                     # the longest stride
        (dict(prompts=None, seg=None), b"engine not finalized"),           # clearing needs a finalized engine too
    ]
    for kw, msg in cases:
        assert _set(lib, h, **kw) == _lib.MT3_ERR_INVALID, msg
        assert lib.mt3_last_error() == b"mt3_engine_set_prompts: " + msg, (kw, lib.mt3_last_error())
    p = np.array(ok, np.int32)
    assert lib.mt3_engine_set_prompts(None, p.ctypes.data, 1, 4, None, 0) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_engine_set_prompts: ")
    assert lib.mt3_engine_status(h, _lib.STATUS_PROMPTS) == 0                  # nothing was set


def test_prompted_drivers_check_their_arguments_first():
    lib = _lib.load()
    X = (C.c_float * 64)()
    p = C.cast(X, C.c_void_p)
    n = C.c_int32()
    assert lib.mt3_op_token_steps_prompted(p, None, 0, 0, 0, 8, 2, 0, 0, p, p, None, None, 0, None, p, 4,
                                           None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_op_token_steps_prompted: ")
    assert lib.mt3_op_beam_search_prompted(p, None, 0, 0, 1, 9, 16, 4, 0, None, None, 0, p, p, p, None, p, p, C.byref(n),
                                           C.byref(n), None, None, 0, None, p, 4, None) == _lib.MT3_ERR_INVALID
    assert lib.mt3_last_error().startswith(b"mt3_op_beam_search_prompted: ") and b"k must be 1 .. 8" in lib.mt3_last_error()


# ------------------------------------------------------------------------------------------------ the tie section
def _codec():
    return vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))


def test_tie_section_prompt_is_the_tie_section_the_encode_side_writes():
    """Notes held over the boundary between segments 0 and 1 (2.048 s): segment 1's targets begin with their tie section."""
    codec = _codec()
    N = NS.Note
    held = [(40, 60), (0, 72), (0, 64), (40, 48)]                      # (program, pitch), not in sorted order
    ns = NS.NoteSequence(notes=[N(0.5, 3.0, pitch, 100, program) for program, pitch in held] +
                         [N(0.2, 1.0, 50, 100, 7), N(2.5, 2.8, 55, 100, 7)], total_time=4.0)
    times, values = NS.note_sequence_to_onsets_and_offsets_and_programs(ns)
    frames = 2 * 256
    ev, si, ei, se, sidx = RLE.encode_and_index_events(NS.NoteEncodingState(), times, values, NS.note_event_data_to_events,
                                                       codec, np.arange(frames) / 125.0, NS.note_encoding_state_to_events)
    tie = codec.encode_event(event_codec.Event("tie", 0))
    vocab = vocabularies.vocabulary_from_codec(codec)
    for seg, notes in ((0, []), (1, held)):
        t = [int(x) for x in RLE.segment_targets(ev, si, ei, se, sidx, seg * 256, (seg + 1) * 256, codec, True)]
        lead = t[: t.index(tie) + 1]
        assert vocabularies.tie_section_prompt(codec, notes) == vocab.encode(lead), seg
        # ... and with the redundant program tokens removed, as the training targets have them
        lean = [int(x) for x in RLE.remove_redundant_state_changes(t, codec, ("velocity", "program"))]
        lean = lean[: lean.index(tie) + 1]
        assert vocabularies.tie_section_prompt(codec, notes, remove_redundant_programs=True) == vocab.encode(lean), seg
    assert len(vocabularies.tie_section_prompt(codec, held)) == 9
    assert len(vocabularies.tie_section_prompt(codec, held, remove_redundant_programs=True)) == 7
    assert vocabularies.tie_section_prompt(codec, []) == [tie + 3]
    assert min(vocabularies.tie_section_prompt(codec, held)) >= 3       # ids, shifted by the special ids: a valid prompt


def test_tie_section_prompt_needs_a_codec_with_ties():
    no_tie = event_codec.Codec(10, 100, [event_codec.EventRange("pitch", 21, 108), event_codec.EventRange("program", 0, 127)])
    with pytest.raises(ValueError, match="tie"):
        vocabularies.tie_section_prompt(no_tie, [(0, 60)])
    with pytest.raises(ValueError):
        vocabularies.tie_section_prompt(_codec(), [(0, 4000)])         # a pitch the codec does not hold


def test_segment_prompts_pads_and_refuses():
    f = inference.InferenceModel._segment_prompts
    assert f(None, 3) is None and f([], 3) is None and f([None, []], 3) is None
    assert f([[5, 6]], 3) == [[5, 6], None, None]
    assert f([None, np.array([7])], 2) == [None, [7]]
    with pytest.raises(ValueError, match="3 entries; the audio has 2 segments"):
        f([[5], None, [6]], 2)
