"""The engine calls each transcribing method of InferenceModel makes, in order, on a box without a GPU.

A recording stub stands in for `network.Transformer` (as in tests/test_inference_host.py), the frontend returns a log-mel
whose segment s of the k-th file of the test reads 100 * k + s everywhere, and `Tensor.cuda` is the identity.  Every case
states the literal sequence of engine calls -- which masks, prompts, grammar, sampling streams and seeds are set before
which decode call on which rows, and which clears follow -- and then checks that
  * the model's own `decoding` and `sampling` are what the constructor set,
  * no attribute of the model references a tensor,
  * every set has its clear, and the same clears are issued when the decode call raises.
Only 16 kHz arrays: the resampler and the WAV decoder are device code."""
import numpy as np
import pytest
import torch

from mt3_amd import _lib, inference, network, spectrograms, vocabularies
from mt3_amd.sampling import SamplingParams as P

SEG = 256 * 128                                   # samples of one segment
DECODES = ("transcribe", "decode", "decode_beams")
PAIRS = {"set_token_masks": "clear_token_masks", "set_token_grammar": "clear_token_grammar",
         "set_note_grammar": "clear_note_grammar", "set_sampling": "clear_sampling"}


def _audio(segments):
    return np.zeros((segments - 1) * SEG + 1000, np.float32)


A1, A2, A3 = _audio(1), _audio(2), _audio(3)


class StubFailure(RuntimeError):
    pass


def _reduce(v):
    """an argument as a literal: the rows of a log-mel by their tags, arrays as lists, grammars by their kind"""
    if isinstance(v, torch.Tensor):
        return [int(t) for t in (v[:, 0, 0] if v.dim() == 3 else v[:, 1])]      # log-mel rows / id rows: their tags
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, _lib.NoteGrammar):
        return "note_grammar"
    if isinstance(v, _lib.TokenGrammar):
        return "token_grammar"
    if isinstance(v, (list, tuple)):
        return [_reduce(x) for x in v]
    return v


@pytest.fixture
def make(monkeypatch):
    """make(**constructor keywords, fail=False) -> (model, log): the log holds (name, *args[, kwargs]) of every engine
    call; with fail the first decode call raises StubFailure"""
    state = {"files": 0}

    def logmel(audio_dev, counts, cfg=None):
        x = torch.zeros((len(counts), 256, 512), dtype=torch.float32)
        x += 100 * state["files"] + torch.arange(len(counts), dtype=torch.float32)[:, None, None]
        state["files"] += 1
        return x

    monkeypatch.setattr(spectrograms, "compute_spectrogram_batch", logmel)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)

    def build(fail=False, **kw):
        log = []
        state["files"] = 0                                                        # the tags restart with every model
        eos = vocabularies.GenericTokenVocabulary.eos_id

        class Stub:
            def __init__(self, cfg, input_length, max_decode_length, max_batch):
                self.config, self.max_batch, self.length = cfg, max_batch, max_decode_length
                self.transcribe_stats = {}

            def load_params(self, params):
                pass

            def _note(self, name, args, kwargs):
                log.append((name,) + tuple(_reduce(a) for a in args) + ((dict(kwargs),) if kwargs else ()))
                if fail and name in DECODES:
                    raise StubFailure("stub: the decode failed")

            def _ids(self, tags, per=1):
                ids = torch.zeros((len(tags) * per, self.length), dtype=torch.int32)
                ids[:, 0] = eos                                                   # every row ends at once
                ids[:, 1] = torch.tensor(tags, dtype=torch.int32).repeat_interleave(per)   # after EOS: the row's tag
                return ids

            def transcribe(self, x, **kw):
                self._note("transcribe", (x,), kw)
                return self._ids(_reduce(x), int(kw.get("draws") or 1))

            def encode(self, x, **kw):
                self._note("encode", (x,), kw)
                self._tags = _reduce(x)

            def decode(self, **kw):
                self._note("decode", (), kw)
                return self._ids(self._tags)

            def decode_beams(self, k, **kw):
                self._note("decode_beams", (k,), kw)
                return self._ids(self._tags), torch.zeros((len(self._tags),))

            def tie_prompts(self, ids, grammar, cap, drop):
                self._note("tie_prompts", (ids, grammar, cap, drop), {})
                prompts = torch.zeros((ids.shape[0], 2 * cap + 1), dtype=torch.int32)
                prompts[:, 0] = 1000 + ids[:, 1]                                  # the prompt the row hands on: 1000 + tag
                return prompts, torch.where(ids[:, 1] == 101, cap + 1, 0).int()   # row 101 held more than `cap` pairs

            def score_segments(self, x, ids, **kw):
                self._note("score_segments", (x,), kw)
                z = torch.zeros(ids.shape, dtype=torch.float32)
                return z[:, 0], z, z.int(), z

            def status(self, what):
                return 0

            def __getattr__(self, name):
                if name.startswith("_"):
                    raise AttributeError(name)
                return lambda *a, **k: self._note(name, a, k)

        monkeypatch.setattr(network, "Transformer", Stub)
        return inference.InferenceModel({"w": 0}, "mt3", **kw), log

    return build


def _tensors(v, depth=0):
    if isinstance(v, torch.Tensor):
        return True
    if depth < 4 and isinstance(v, (list, tuple)):
        return any(_tensors(x, depth + 1) for x in v)
    if depth < 4 and isinstance(v, dict):
        return any(_tensors(x, depth + 1) for x in v.values())
    return False


def _holds_tensor(m):
    return sorted(k for k, v in vars(m).items() if _tensors(v))


def _check_left_clean(m, log, kw):
    assert m.decoding == kw.get("decoding", "beam1")
    assert m.sampling == P(float(kw.get("temperature", 1.0)), int(kw.get("top_k", 0)), float(kw.get("top_p", 0.0)),
                           int(kw.get("seed", 0)))
    assert _holds_tensor(m) == []
    last = {}
    for entry in log:                                                            # the last call of each kind is its clear
        name = entry[0]
        if name in PAIRS:
            last[name] = "set"
        elif name in PAIRS.values():
            last[[s for s, c in PAIRS.items() if c == name][0]] = "clear"
        elif name == "set_prompts":
            last[name] = "clear" if entry[1] is None else "set"
    assert all(v == "clear" for v in last.values()), last


def _clears(expect):
    """what follows the last decode / tie_prompts / scoring call of the expected sequence"""
    at = max(i for i, e in enumerate(expect) if e[0] in DECODES + ("tie_prompts", "score_segments"))
    return expect[at + 1:]


def check(make, call, expect, **kw):
    """the call's engine calls are `expect`; when the first decode call raises they are `expect` up to that call, then
    the same clears; either way the model is left as the constructor made it"""
    m, log = make(**kw)
    out = call(m)
    assert log == expect
    _check_left_clean(m, log, kw)
    bad, bad_log = make(fail=True, **kw)
    with pytest.raises(StubFailure):
        call(bad)
    first = min(i for i, e in enumerate(expect) if e[0] in DECODES)
    assert bad_log == expect[:first + 1] + _clears(expect)
    _check_left_clean(bad, bad_log, kw)
    return m, out


def _mask_rows(m, *constraints):
    return [vocabularies.token_mask(m.codec, m.model_config.vocab_size, p, d).tolist() for p, d in constraints]


@pytest.fixture(scope="module")
def host():
    """codec-derived constants: the mask rows of ([0], no drums) and ([33], drums), the tie id"""
    m = object.__new__(inference.InferenceModel)
    m.codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    m.model_config = network.T5Config(vocab_size=vocabularies.num_embeddings(vocabularies.vocabulary_from_codec(m.codec)))
    tie = m.codec.encode_event(vocabularies.event_codec.Event("tie", 0)) + 3
    return {"M0": _mask_rows(m, ([0], False)), "M0_33": _mask_rows(m, ([0], False), ([33], True)),
            "M0_0and33": _mask_rows(m, ([0, 33], True)), "tie": int(tie)}


# ---------------------------------------------------------------------------------------------------- __call__
def test_call_plain(make):
    m, ns = check(make, lambda m: m(A3), [("transcribe", [0, 1, 2], {"beam1": True})])
    assert m.rows_per_engine_call == [3] and len(ns.notes) == 0
    assert m.last_event_counts == {"invalid_events": 0, "dropped_events": 0, "tie_overflows": 0}


def test_call_programs(make, host):
    assert len(host["M0"]) == 1 and len(host["M0"][0]) == 48
    check(make, lambda m: m(A3, programs=[0], drums=False),
          [("set_token_masks", host["M0"], None),
           ("transcribe", [0, 1, 2], {"beam1": True}),
           ("clear_token_masks",)])
    # a single file: programs=[0, 33] is ONE constraint, and a list for drums= is refused
    check(make, lambda m: m(A1, programs=[0, 33]),
          [("set_token_masks", host["M0_0and33"], None),
           ("transcribe", [0], {"beam1": True}),
           ("clear_token_masks",)])
    m, log = make()
    with pytest.raises(ValueError, match="drums must be one bool for a single file"):
        m(A1, drums=[True])
    assert log == []


def test_call_prompts(make):
    check(make, lambda m: m(A3, prompts=[[3, 4], None, [5]]),
          [("set_prompts", [[3, 4], [5]], [0, -1, 1]),
           ("transcribe", [0, 1, 2], {"beam1": True}),
           ("set_prompts", None)])
    check(make, lambda m: m(A3, prompts=[None, []]), [("transcribe", [0, 1, 2], {"beam1": True})])


def test_call_well_formed(make, host):
    check(make, lambda m: m(A3, well_formed=True),
          [("set_token_grammar", "token_grammar"),
           ("transcribe", [0, 1, 2], {"beam1": True}),
           ("clear_token_grammar",)])
    check(make, lambda m: m(A3, well_formed="notes", programs=[0], drums=False, prompts=[[7]]),
          [("set_token_masks", host["M0"], None),
           ("set_prompts", [[7]], [0, -1, -1]),
           ("set_note_grammar", "note_grammar"),
           ("transcribe", [0, 1, 2], {"beam1": True}),
           ("clear_note_grammar",),
           ("clear_token_masks",),
           ("set_prompts", None)])
    m, log = make()
    with pytest.raises(ValueError, match="well_formed is False, True"):
        m(A1, well_formed="ties")
    assert log == []


def test_call_tied_decodes_one_segment_per_pass(make, host):
    tie = host["tie"]
    m, _ = check(make, lambda m: m(A3, well_formed="tied"),
                 [("set_prompts", [[tie]], [0]),
                  ("set_note_grammar", "note_grammar"),
                  ("transcribe", [0], {"beam1": True}),
                  ("tie_prompts", [0], "note_grammar", 64, True),
                  ("set_prompts", [[1000]], [0]),
                  ("set_note_grammar", "note_grammar"),
                  ("transcribe", [1], {"beam1": True}),
                  ("tie_prompts", [1], "note_grammar", 64, True),
                  ("set_prompts", [[1001]], [0]),
                  ("set_note_grammar", "note_grammar"),
                  ("transcribe", [2], {"beam1": True}),
                  ("set_prompts", None),
                  ("clear_note_grammar",)])
    assert m.rows_per_engine_call == [1, 1, 1] and m.last_event_counts["tie_overflows"] == 0
    m, log = make()
    with pytest.raises(ValueError, match="not together with prompts="):
        m(A1, prompts=[[tie]], well_formed="tied")
    assert log == []


def test_call_scored(make, host):
    m, (ns, scores) = check(make, lambda m: m.transcribe_scored(A3, programs=[0], drums=False),
                            [("set_token_masks", host["M0"], None),
                             ("transcribe", [0, 1, 2], {"beam1": True}),
                             ("score_segments", [0, 1, 2], {"return_token_scores": True, "return_top1": True}),
                             ("clear_token_masks",)])
    assert len(ns.notes) == 0 and scores["onset_logprob"].shape == (0,)
    assert m.last_event_counts == {"invalid_events": 0, "dropped_events": 0, "tie_overflows": 0}


def test_a_refused_call_leaves_no_tensor_on_the_model(make):
    """the frontend has run when the prompts are counted against the segments: the refusal must not leave its log-mel
    referenced from the model"""
    m, log = make()
    with pytest.raises(ValueError, match="prompts has 99 entries; the audio has 3 segments"):
        m(A3, prompts=[[1]] * 99)
    with pytest.raises(ValueError, match="drums must be one bool"):
        m(A3, drums=[True])
    with pytest.raises(ValueError, match="well_formed is False, True"):
        m(A3, well_formed="ties")
    assert log == []
    assert _holds_tensor(m) == []


# ---------------------------------------------------------------------------------------------------- several files
def test_many_with_programs_and_prompts_per_file(make, host):
    m, out = check(make, lambda m: m.transcribe_many([A3, A2], programs=[[0], None], drums=[False, True],
                                                     prompts=[[[3, 4]], None], well_formed=True),
                   [("set_token_masks", host["M0"], [0, 0, 0, -1, -1]),
                    ("set_prompts", [[3, 4]], [0, -1, -1, -1, -1]),
                    ("set_token_grammar", "token_grammar"),
                    ("transcribe", [0, 1, 2, 100, 101], {"beam1": True}),
                    ("clear_token_grammar",),
                    ("clear_token_masks",),
                    ("set_prompts", None)])
    assert len(out) == 2 and m.rows_per_engine_call == [5]
    check(make, lambda m: m.transcribe_many([A1, A2, A1], programs=[[33], [0], [33]], drums=[True, False, True]),
          [("set_token_masks", [host["M0_33"][1], host["M0_33"][0]], [0, 1, 1, 0]),
           ("transcribe", [0, 100, 101, 200], {"beam1": True}),
           ("clear_token_masks",)])
    m, log = make()
    assert m.transcribe_many([]) == [] and log == []
    with pytest.raises(ValueError, match="sample_rates has 1 entries for 2 files"):
        m.transcribe_many([A1, A1], [16000])
    with pytest.raises(ValueError, match="prompts has 1 entries for 2 files"):
        m.transcribe_many([A1, A1], prompts=[None])
    assert log == [] and _holds_tensor(m) == []


def test_many_tied_is_a_wavefront_over_segment_indices(make, host):
    """files of 1, 3 and 2 segments, sampled so that the streams show: pass j holds segment j of every file that has one,
    with its file's mask index, its own stream j and the prompt the file's row of pass j - 1 handed on"""
    tie, kw = host["tie"], dict(decoding="sample", top_k=40, seed=7)
    params = P(1.0, 40, 0.0, 7)
    m, out = check(make, lambda m: m.transcribe_many([A1, A3, A2], programs=[[0], None, [0]], drums=[False, True, False],
                                                     well_formed="tied"),
                   [("set_token_masks", host["M0"], [0, -1, 0]),
                    ("set_prompts", [[tie]], [0, 0, 0]),
                    ("set_note_grammar", "note_grammar"),
                    ("set_sampling", params, [0, 0, 0], None),
                    ("transcribe", [0, 100, 200], {"beam1": False}),
                    ("tie_prompts", [100, 200], "note_grammar", 64, True),
                    ("set_token_masks", host["M0"], [-1, 0]),
                    ("set_prompts", [[1100], [1200]], [0, 1]),
                    ("set_note_grammar", "note_grammar"),
                    ("set_sampling", params, [1, 1], None),
                    ("transcribe", [101, 201], {"beam1": False}),
                    ("tie_prompts", [101], "note_grammar", 64, True),
                    ("set_token_masks", host["M0"], [-1]),
                    ("set_prompts", [[1101]], [0]),
                    ("set_note_grammar", "note_grammar"),
                    ("set_sampling", params, [2], None),
                    ("transcribe", [102], {"beam1": False}),
                    ("set_prompts", None),
                    ("clear_note_grammar",),
                    ("clear_token_masks",),
                    ("clear_sampling",)], **kw)
    assert len(out) == 3 and m.rows_per_engine_call == [3, 2, 1]
    assert m.last_event_counts["tie_overflows"] == 1                         # the stub's row 101
    m(A1)
    assert m.last_event_counts["tie_overflows"] == 0                         # of the most recent call only


def test_many_sampled_streams_are_the_segment_index_within_its_file(make):
    kw = dict(decoding="sample", temperature=0.5, top_p=0.9, seed=11)
    params = P(0.5, 0, 0.9, 11)
    check(make, lambda m: m.transcribe_many([A3, A2]),
          [("set_sampling", params, [0, 1, 2, 0, 1], None),
           ("transcribe", [0, 1, 2, 100, 101], {"beam1": False}),
           ("clear_sampling",)], **kw)
    check(make, lambda m: m(A3),
          [("set_sampling", params, [0, 1, 2], None),
           ("transcribe", [0, 1, 2], {"beam1": False}),
           ("clear_sampling",)], **kw)
    # the reference's loop, two rows per engine call: a chunk's streams are its rows of the job's table
    m, _ = check(make, lambda m: m.transcribe_many([A3, A2]),
                 [("encode", [0, 1]),
                  ("set_sampling", params, [0, 1], None),
                  ("decode", {"early_exit": True, "beam1": False}),
                  ("encode", [2, 100]),
                  ("set_sampling", params, [2, 0], None),
                  ("decode", {"early_exit": True, "beam1": False}),
                  ("encode", [101]),
                  ("set_sampling", params, [1], None),
                  ("decode", {"early_exit": True, "beam1": False}),
                  ("clear_sampling",)], schedule="batch", batch_size=2, **kw)
    assert m.rows_per_engine_call == [2, 2, 1]


def test_batch_schedule_sets_each_chunk_s_tables(make, host):
    m, _ = check(make, lambda m: m(A3, prompts=[None, None, [5]], programs=[0], drums=False),
                 [("encode", [0, 1]),
                  ("set_token_masks", host["M0"], None),
                  ("set_prompts", [], None),
                  ("decode", {"early_exit": True, "beam1": False}),
                  ("encode", [2]),
                  ("set_token_masks", host["M0"], None),
                  ("set_prompts", [[5]], [0]),
                  ("decode", {"early_exit": True, "beam1": False}),
                  ("clear_token_masks",),
                  ("set_prompts", None)], decoding="greedy", schedule="batch", batch_size=2)
    assert m.rows_per_engine_call == [2, 1]


# ---------------------------------------------------------------------------------------------------- sample
def test_sample_is_one_job_of_draws(make):
    m, out = check(make, lambda m: m.sample(A3, 3),
                   [("set_sampling", P(1.0, 0, 0.0, 5), [0, 0, 0, 1, 1, 1, 2, 2, 2], [5, 6, 7] * 3),
                    ("transcribe", [0, 1, 2], {"draws": 3}),
                    ("clear_sampling",)], seed=5)
    assert len(out) == 3 and m.rows_per_engine_call == [9]
    check(make, lambda m: m.sample(A2, 2, prompts=[None, [9]], well_formed=True),
          [("set_prompts", [[9]], [-1, -1, 0, 0]),
           ("set_token_grammar", "token_grammar"),
           ("set_sampling", P(1.0, 0, 0.0, (1 << 64) - 1), [0, 0, 1, 1], [(1 << 64) - 1, 0] * 2),
           ("transcribe", [0, 1], {"draws": 2}),
           ("clear_token_grammar",),
           ("set_prompts", None),
           ("clear_sampling",)], decoding="greedy", seed=(1 << 64) - 1)
    m, log = make(decoding="beam")
    with pytest.raises(ValueError, match="not for a model with decoding='beam'"):
        m.sample(A1, 2)
    with pytest.raises(ValueError, match="num_samples must be at least 1"):
        make()[0].sample(A1, 0)
    assert log == []


def test_sample_many_is_one_job_of_draws(make, host):
    m, out = check(make, lambda m: m.sample_many([A3, A2], 2, programs=[[0], None], drums=[False, True]),
                   [("set_token_masks", host["M0"], [0] * 6 + [-1] * 4),
                    ("set_sampling", P(1.0, 0, 0.0, 5), [0, 0, 1, 1, 2, 2, 0, 0, 1, 1], [5, 6] * 5),
                    ("transcribe", [0, 1, 2, 100, 101], {"draws": 2}),
                    ("clear_token_masks",),
                    ("clear_sampling",)], seed=5)
    assert [len(f) for f in out] == [2, 2] and m.rows_per_engine_call == [10]
    m, log = make()
    assert m.sample_many([], 2) == [] and log == []
    with pytest.raises(ValueError, match="sample_rates has 2 entries for 1 files"):
        m.sample_many([A1], 2, [16000, 16000])


def test_sample_on_the_batch_schedule_is_a_loop_of_jobs(make):
    first = [("encode", [0, 1, 2]),
             ("set_sampling", P(1.0, 0, 0.0, 5), list(range(8)), None),      # a lone file: the chunk's row numbers
             ("decode", {"early_exit": True, "beam1": False}),
             ("clear_sampling",)]
    second = [("encode", [100, 101, 102]),
              ("set_sampling", P(1.0, 0, 0.0, 6), list(range(8)), None),
              ("decode", {"early_exit": True, "beam1": False}),
              ("clear_sampling",)]
    m, out = check(make, lambda m: m.sample(A3, 2), first + second, schedule="batch", seed=5)
    assert len(out) == 2
    m, out = check(make, lambda m: m.sample_many([A3, A2], 2),
                   [("encode", [0, 1, 2, 100, 101]),
                    ("set_sampling", P(1.0, 0, 0.0, 5), [0, 1, 2, 0, 1], None),
                    ("decode", {"early_exit": True, "beam1": False}),
                    ("clear_sampling",),
                    ("encode", [200, 201, 202, 300, 301]),
                    ("set_sampling", P(1.0, 0, 0.0, 6), [0, 1, 2, 0, 1], None),
                    ("decode", {"early_exit": True, "beam1": False}),
                    ("clear_sampling",)], schedule="batch", seed=5)
    assert [len(f) for f in out] == [2, 2]


def test_sample_tied_is_a_loop_of_wavefronts(make, host):
    tie = host["tie"]

    def run(seed, tag):
        return [("set_prompts", [[tie]], [0]),
                ("set_note_grammar", "note_grammar"),
                ("set_sampling", P(1.0, 0, 0.0, seed), [0], None),
                ("transcribe", [tag], {"beam1": False}),
                ("tie_prompts", [tag], "note_grammar", 3, False),
                ("set_prompts", [[1000 + tag]], [0]),
                ("set_note_grammar", "note_grammar"),
                ("set_sampling", P(1.0, 0, 0.0, seed), [1], None),
                ("transcribe", [tag + 1], {"beam1": False}),
                ("set_prompts", None),
                ("clear_note_grammar",),
                ("clear_sampling",)]

    check(make, lambda m: m.sample(A2, 2, well_formed="tied"), run(5, 0) + run(6, 100), decoding="greedy", seed=5, cap=3,
          drop_redundant_programs=False)


# ---------------------------------------------------------------------------------------------------- beams
def test_beam_search_on_both_schedules(make, host):
    m, _ = check(make, lambda m: m(A3, programs=[0], drums=False),
                 [("set_token_masks", host["M0"], None),
                  ("transcribe", [0, 1, 2], {"num_beams": 2}),
                  ("clear_token_masks",)], decoding="beam", num_beams=2, schedule="refill")
    assert m.rows_per_engine_call == [6]
    m, _ = check(make, lambda m: m.transcribe_many([A2, A1], programs=[[0], None], drums=[False, True]),
                 [("encode", [0, 1], {"num_beams": 2}),
                  ("set_token_masks", host["M0"], [0, 0]),
                  ("decode_beams", 2, {"early_exit": True}),
                  ("encode", [100], {"num_beams": 2}),
                  ("set_token_masks", host["M0"], [-1]),
                  ("decode_beams", 2, {"early_exit": True}),
                  ("clear_token_masks",)], decoding="beam", num_beams=2, max_slots=4, batch_size=2)
    assert m.schedule == "batch" and m.rows_per_engine_call == [4, 2] and m.engine_slots == 4
