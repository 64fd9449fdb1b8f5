"""Tied decoding through InferenceModel (well_formed="tied"): a tiny random-weight f32 model whose logits favour note
events (synthetic.boost_note_events, as the smoke run's), and the trained fixture.

Seeds: tiny-model weights seed 4, audio synth_audio seed 0 (the smoke run's pair, which decodes notes); trained fixture
synth_music(seed=78), the first 6 segments of DESIGN.md 6g's audio -- under well_formed="notes" it has invalid events
(asserted below as the precondition: the test that fails without the feature)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, inference, network, synthetic, ties  # noqa: E402
from tests import note_grammar_ref as nr  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
SEG = 32768
CFG = network.T5Config(dtype="float32", num_encoder_layers=1, num_decoder_layers=2)


def _params():
    return synthetic.boost_note_events(network.init_random_params(CFG, seed=4, norm_scale_jitter=0.1), eos=3.0)


def _files():
    """three files of 1, 3 and 2 segments"""
    wav = synthetic.synth_audio(6, seed=0, device="cpu").reshape(-1).numpy()
    return [wav[: SEG - 4000], wav[SEG: 3 * SEG + 9000], wav[4 * SEG: 5 * SEG + 5000]]


def _model(**kw):
    m = inference.InferenceModel(_params(), "mt3", config=CFG, dtype="float32", **kw)
    m.seen = []
    predict = m._predict_ids

    def record(batch, *a, **k):
        out = predict(batch, *a, **k)
        m.seen.append(out.cpu().numpy())
        return out

    m._predict_ids = record                       # the job's ids are the LAST entry: the passes of a tied job come before it
    return m


def _check_chain(m, rows, counts):
    """property 2: every row is accepted with its prompt length; row j + 1 opens with ties.tie_prompt of row j"""
    n, grammar = nr.from_struct(m.note_grammar()), m.note_grammar()
    at = 0
    for c in counts:
        prompt = [int(grammar.g.tie_id)]
        for j in range(c):
            row = rows[at + j]
            assert list(row[: len(prompt)]) == prompt, (at, j)
            assert nr.accepts(n, row, len(prompt)), (at, j, nr.first_rejected(n, row, len(prompt)))
            prompt = ties.prompt_ids(ties.tie_prompt(grammar, row, m.cap, m.drop_redundant_programs)[0])
        at += c


def test_wavefront_equals_the_chain_and_leaves_the_engine_clean():
    """(1) the job's ids are those of each file alone, segment by segment, through prompts= and well_formed="notes" with
    the prompts computed on the host; (2) the chain property; (6) afterwards nothing is set and a plain call gives the plain
    run's ids"""
    files = _files()
    m = _model(decoding="greedy")
    m(files[1])
    plain = m.seen[-1]
    out = m.transcribe_many(files, well_formed="tied")
    job = m.seen[-1]
    assert len(out) == 3 and job.shape[0] == 6 and m.last_event_counts["tie_overflows"] == 0
    for what in (_lib.STATUS_PROMPTS, _lib.STATUS_TOKEN_MASKS, _lib.STATUS_TOKEN_GRAMMAR, _lib.STATUS_NOTE_GRAMMAR,
                 _lib.STATUS_SAMPLING):
        assert m.model.status(what) == 0
    _check_chain(m, job, [1, 3, 2])
    assert sum(len(ties.held_pairs(m.note_grammar(), ties.held_after(m.note_grammar(), r))) for r in job) > 0
    grammar, at = m.note_grammar(), 0
    for f, c in zip(files, [1, 3, 2]):
        prompts = [[int(grammar.g.tie_id)]]
        for j in range(c):
            m(f, prompts=prompts, well_formed="notes")
            row = m.seen[-1][j]
            assert np.array_equal(row, job[at + j]), (at, j)
            prompts = prompts + [ties.prompt_ids(ties.tie_prompt(grammar, row, 64, True)[0])]
        at += c
    m(files[1])
    assert np.array_equal(m.seen[-1], plain)


@pytest.mark.parametrize("kw", [dict(decoding="beam1"), dict(decoding="beam", num_beams=2),
                                dict(decoding="beam", num_beams=2, schedule="refill"),
                                dict(decoding="sample", temperature=1.0, top_k=40, seed=1234)],
                         ids=["beam1", "beam2", "beam2_refill", "sample"])
def test_other_decoding_rules_keep_the_chain(kw):
    """(3) beam-1, k = 2 beams (both schedules) and sampling: one short job each, property 2"""
    files = _files()
    m = _model(**kw)
    m.transcribe_many(files[1:], well_formed="tied")
    assert m.seen[-1].shape[0] == 5
    _check_chain(m, m.seen[-1], [3, 2])


def test_scored_and_wav_forms_take_tied():
    files = _files()
    m = _model(decoding="greedy")
    ns, scores = m.transcribe_scored(files[2], well_formed="tied")
    assert len(scores["onset_logprob"]) == len(ns.notes)
    _check_chain(m, m.seen[-1], [2])
    m.sample(files[2], num_samples=1, well_formed="tied")
    _check_chain(m, m.seen[-1], [2])


def test_refusals():
    """(5) prompts= with "tied"; a cap whose tie section leaves the decode no room; a spec without a tie section"""
    files = _files()
    m = _model(decoding="greedy")
    with pytest.raises(ValueError, match="prompts"):
        m(files[0], prompts=[[int(m.note_grammar().g.tie_id)]], well_formed="tied")
    with pytest.raises(ValueError, match="prompts"):
        m.transcribe_many(files[:1], prompts=[[[int(m.note_grammar().g.tie_id)]]], well_formed="tied")
    m.cap = 512                                   # 2 * 512 + 1 >= 1024
    with pytest.raises(ValueError, match="cap"):
        m(files[0], well_formed="tied")
    m.cap = 511                                   # 1023 < 1024: the largest cap a decode of 1024 steps takes
    m(files[0], well_formed="tied")
    with pytest.raises(ValueError, match="cap"):
        inference.InferenceModel(_params(), "mt3", config=CFG, cap=-1)
    assert m.model.status(_lib.STATUS_NOTE_GRAMMAR) == 0 and m.model.status(_lib.STATUS_PROMPTS) == 0
    old = inference.InferenceModel("random:0", "ismir2021", config=CFG)
    with pytest.raises(ValueError, match="tie section"):
        old(files[0], well_formed="tied")
    with pytest.raises(ValueError):
        m(files[0], well_formed="ties")


def test_trained_fixture_has_no_invalid_events_tied():
    """(4) f32 greedy on the trained fixture, synth_music(seed=78), 6 segments: "tied" leaves the note decoder nothing
    invalid and nothing dropped; the same audio under "notes" has invalid events (the precondition)"""
    audio = synthetic.synth_music(6 * 2.048 - 0.3, seed=78, device="cpu")[1]
    m = inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32", decoding="greedy")
    m(audio, well_formed="notes")
    notes_counts = dict(m.last_event_counts)
    ns = m(audio, well_formed="tied")
    tied_counts = dict(m.last_event_counts)
    print("TIED_FIXTURE notes-mode %s tied-mode %s notes %d" % (notes_counts, tied_counts, len(ns.notes)))
    assert notes_counts["invalid_events"] > 0
    assert len(ns.notes) > 0
    assert tied_counts["invalid_events"] == 0 and tied_counts["dropped_events"] == 0
    assert tied_counts["tie_overflows"] == 0
