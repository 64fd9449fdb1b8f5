"""Note-consistent decoding through the engine (mt3_engine_set_note_grammar): the tiny random-weight engines of
tests/test_gpu_grammar_engine.py (one encoder layer, two decoder layers, L = 64, 16 steps), f32 and bf16, the e4m3 caches
once; the real `mt3` codec with max_steps = 204.  Half the segments carry the bare-`tie` prompt, so both phases of the rule
(inside the tie section, after it) are reached within 16 steps.

Seeds: engine seed 5, audio seed 21 -- with them the decode of the same segments under the event grammar ALONE
(`well_formed=True`'s rule) gives rows the note acceptor rejects (asserted below as the precondition: the test that fails
without the feature); a seed that failed it would be replaced here."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, inference, network, note_sequences, spectrograms, synthetic, vocabularies  # noqa: E402
from tests import note_grammar_ref as nr  # noqa: E402

L, S, V = 64, 16, 1536
CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
ENGINES = [("float32", ""), ("bfloat16", ""), ("bfloat16", "fp8_e4m3")]
CODEC = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
TIES = note_sequences.NoteEncodingWithTiesSpec
NOTES = vocabularies.note_grammar(CODEC, V, TIES, 204)
GRAMMAR = vocabularies.token_grammar(CODEC, V, TIES, 204)
N = nr.from_struct(NOTES)
TIE = vocabularies.tie_section_prompt(CODEC, [])
SAMPLING = dict(temperature=1.0, top_k=40, seed=1234)


def _engine(dtype, B, kv="", seed=5):
    cfg = network.T5Config(dtype=dtype, kv_dtype=kv, num_encoder_layers=1, num_decoder_layers=2)
    params = network.init_random_params(cfg, seed=seed, norm_scale_jitter=0.1)
    eng = network.Transformer(cfg, input_length=256, max_decode_length=L, max_batch=B)
    eng.load_params(params)
    return eng


def _lm(n, seed=21):
    return spectrograms.compute_spectrogram_batch(synthetic.synth_audio(n, seed=seed), None)


def _prompt_index(n):
    return [0 if i % 2 == 0 else -1 for i in range(n)]


def _plen(i):
    return 1 if i % 2 == 0 else 0


def _everything(eng, lm):
    """decode, beam-1, decode_beams, transcribe, beam-1 transcribe, beam transcribe, sampled decode, sampled transcribe"""
    out = []
    eng.set_prompts([TIE], _prompt_index(8))
    eng.encode(lm[:8])
    out += [eng.decode(num_steps=S), eng.decode(num_steps=S, beam1=True, early_exit=True)]
    eng.set_prompts([TIE], _prompt_index(4))
    eng.encode(lm[:4], num_beams=2)
    out += list(eng.decode_beams(2, num_steps=S, return_all=True))
    eng.set_prompts([TIE], _prompt_index(len(lm)))
    out += [eng.transcribe(lm, num_steps=S), eng.transcribe(lm, num_steps=S, beam1=True)]
    out += list(eng.transcribe(lm, num_steps=S, num_beams=2, return_all=True))
    out = [o.clone() for o in out]
    eng.set_sampling(**SAMPLING)
    try:
        eng.set_prompts([TIE], _prompt_index(8))
        eng.encode(lm[:8])
        out.append(eng.decode(num_steps=S).clone())
        eng.set_prompts([TIE], _prompt_index(len(lm)))
        out.append(eng.transcribe(lm, num_steps=S).clone())
    finally:
        eng.clear_sampling()
        eng.set_prompts(None)
    return out


def _rows(out):
    """(segment, id row) of every decode in `_everything`'s outputs (out[3] and out[7] are the beam calls' scores)"""
    rows = []
    for o in (out[0], out[1], out[4], out[5], out[8], out[9]):
        rows += [(i, r) for i, r in enumerate(o.cpu().numpy()[:, :S])]
    for o in (out[2], out[6]):
        rows += [(i, r) for i, d in enumerate(o.cpu().numpy()) for r in d[:, :S]]
    return rows


@pytest.mark.parametrize("dtype,kv", ENGINES)
def test_off_changes_no_bit_and_on_is_note_consistent(dtype, kv):
    """(1) set and clear leave every decode as it was, bit for bit, the event grammar's decodes included; with the rule on
    every emitted row -- greedy, beam-1, all k of the beam calls, sampled -- is accepted by the note acceptor.  (2) THE
    PRECONDITION: under the event grammar alone the same segments give at least one row the note acceptor rejects."""
    eng, lm = _engine(dtype, 8, kv), _lm(11)
    plain = _everything(eng, lm)
    eng.set_token_grammar(GRAMMAR)
    formed = _everything(eng, lm)
    eng.clear_token_grammar()
    fallbacks = eng.status(_lib.STATUS_GRAPH_FALLBACKS)
    eng.set_note_grammar(NOTES)
    assert eng.status(_lib.STATUS_NOTE_GRAMMAR) == 1 and eng.status(_lib.STATUS_TOKEN_GRAMMAR) == 0
    with pytest.raises(_lib.Mt3Error, match="a note grammar is set"):
        eng.set_token_grammar(GRAMMAR)
    consistent = _everything(eng, lm)
    assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
    eng.clear_note_grammar()
    assert eng.status(_lib.STATUS_NOTE_GRAMMAR) == 0
    again = _everything(eng, lm)
    for i, (a, b) in enumerate(zip(plain, again)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
    eng.set_token_grammar(GRAMMAR)
    with pytest.raises(_lib.Mt3Error, match="a token grammar is set"):
        eng.set_note_grammar(NOTES)
    formed2 = _everything(eng, lm)
    eng.clear_token_grammar()
    for i, (a, b) in enumerate(zip(formed, formed2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
    eng.set_note_grammar(NOTES)
    consistent2 = _everything(eng, lm)
    eng.clear_note_grammar()
    for i, (a, b) in enumerate(zip(consistent, consistent2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == fallbacks
    bad = [(i, not nr.accepts(N, r, _plen(i))) for i, r in _rows(formed)]
    print("NOTE_REJECTED_UNDER_GRAMMAR_ALONE %s %s: %d of %d rows" % (dtype, kv, sum(b for _, b in bad), len(bad)))
    assert sum(b for _, b in bad) >= 1
    for i, r in _rows(consistent):
        assert nr.accepts(N, r, _plen(i)), (i, list(r), nr.first_rejected(N, r, _plen(i)))


@pytest.mark.parametrize("dtype,kv", ENGINES[:2])
def test_greedy_rule_end_to_end(dtype, kv):
    """(3) decode_forced on the emitted ids gives the model's own logits (it ignores the rule); at every free step the
    emitted id is the arg-max of those logits over the note rule's allowed vector, the state replayed by the reference"""
    eng, lm = _engine(dtype, 8, kv), _lm(8)
    eng.encode(lm)
    eng.set_prompts([TIE], _prompt_index(8))
    eng.set_note_grammar(NOTES)
    try:
        ids = eng.decode(num_steps=S)
        _, logits = eng.decode_forced(ids, num_steps=S)
    finally:
        eng.clear_note_grammar()
        eng.set_prompts(None)
    lg, got = logits.cpu().numpy(), ids.cpu().numpy()
    assert np.isfinite(lg).all()
    for b in range(8):
        state = nr.initial(N)
        for t in range(S):
            if t < _plen(b):
                want = TIE[t]
            else:
                want = int(np.argmax(np.where(nr.allowed_vector(N, state, V), lg[t, b], -np.inf)))
            assert got[b, t] == want, (b, t)
            state = nr.advance(N, state, want)
            if want == 1:
                assert (got[b, t + 1:] == 0).all()
                break


@pytest.mark.parametrize("dtype,kv", ENGINES)
def test_state_is_reset_on_refill_and_travels_with_compaction(dtype, kv):
    """(4) 11 segments through 8 slots -- more segments than slots, rows that end at different lengths -- give per segment
    the bits of the segment decoded alone (greedy, beam-1, k = 2); the early exit with compaction gives the ids of the
    schedule without it, up to each row's EOS"""
    eng, lm = _engine(dtype, 8, kv), _lm(11)
    eng.set_note_grammar(NOTES)
    try:
        eng.set_prompts([TIE], _prompt_index(11))
        job = [eng.transcribe(lm, num_steps=S).clone(), eng.transcribe(lm, num_steps=S, beam1=True).clone()]
        job_k = [o.clone() for o in eng.transcribe(lm, num_steps=S, num_beams=2, return_all=True)]
        for i in range(11):
            eng.set_prompts([TIE], [0 if i % 2 == 0 else -1])
            eng.encode(lm[i:i + 1])
            assert torch.equal(eng.decode(num_steps=S, early_exit=True)[0], job[0][i]), i
            assert torch.equal(eng.decode(num_steps=S, early_exit=True, beam1=True)[0], job[1][i]), i
            eng.set_prompts([TIE], [0 if i % 2 == 0 else -1] * 4)
            eng.encode(lm[i:i + 1].repeat(4, 1, 1), num_beams=2)
            alone = eng.decode_beams(2, num_steps=S, early_exit=True, return_all=True)
            assert torch.equal(alone[0][0], job_k[0][i]) and torch.equal(alone[1][0], job_k[1][i]), i
        eng.set_prompts([TIE], _prompt_index(8))
        eng.encode(lm[:8])
        full = eng.decode(num_steps=S).cpu().numpy()
        early = eng.decode(num_steps=S, early_exit=True).cpu().numpy()
        for b in range(8):
            n = int(np.argmax(full[b] == 1)) + 1 if (full[b] == 1).any() else S
            assert np.array_equal(full[b, :n], early[b, :n]), b
            assert nr.accepts(N, early[b], _plen(b)), b
    finally:
        eng.clear_note_grammar()
        eng.set_prompts(None)


def test_inference_model_notes():
    """(5) InferenceModel(...)(audio, well_formed="notes") on the trained fixture returns notes, and no row, decoded alone
    as in tests/test_note_grammar_ref.py, is rejected by the note acceptor (so none of the three per-segment kinds of
    invalid event occurs); a model whose spec has no tie section raises ValueError"""
    audio = synthetic.synth_music(3 * 2.048 - 0.3, seed=13, device="cpu")[1]
    m = inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32", decoding="greedy")
    seen = []
    predict = m._predict_ids
    m._predict_ids = lambda batch, *a, **kw: seen.append(predict(batch, *a, **kw)) or seen[-1]
    ns = m(audio, well_formed="notes")
    assert len(ns.notes) > 0 and m.last_event_counts["dropped_events"] == 0
    assert m.model.status(_lib.STATUS_NOTE_GRAMMAR) == 0 and m.model.status(_lib.STATUS_TOKEN_GRAMMAR) == 0
    n = nr.from_struct(m.note_grammar())
    rows = seen[0].cpu().numpy()
    assert len(rows) >= 3
    for r in rows:
        assert nr.accepts(n, r), (list(r[:40]), nr.first_rejected(n, r))
    with pytest.raises(ValueError):
        m(audio, well_formed="something")
    with pytest.raises(ValueError, match="tie section"):
        vocabularies.note_grammar(m.codec, m.model_config.vocab_size, note_sequences.NoteEncodingSpec, 204)


def _mask_words(forbid):
    m = np.full(V // 32, 0xFFFFFFFF, np.uint32)
    for i in forbid:
        m[i >> 5] &= np.uint32(~(1 << (i & 31)) & 0xFFFFFFFF)
    return m


def test_decodes_refuse_a_mask_that_leaves_the_rule_no_room():
    """(6) MT3_ERR_INVALID, before any device work, for a mask in use that leaves the worst state after the tie section --
    velocity zero, nothing held: no pitch, no drum -- fewer than 2 ids (the beam calls: 2k), though the event grammar alone
    has room under it; a spec without ties is refused by the engine as well; a set while a decode is in flight is refused"""
    eng, lm = _engine("float32", 8), _lm(8)
    keep = set(range(N.pitch_first, N.pitch_first + N.pitch_count)) | set(range(N.drum_first, N.drum_first + N.drum_count)) | \
        set(range(N.program_first, N.program_first + N.program_count)) | {1, N.tie_id}
    one = _mask_words([i for i in range(V) if i not in keep - set(range(N.program_first, N.program_first + N.program_count))])
    many = _mask_words([i for i in range(V) if i not in keep])                   # EOS + 128 programs after a note-off marker
    three = _mask_words([i for i in range(V) if i not in (keep - set(range(N.program_first + 2, N.program_first + 128)))])
    refused = pytest.raises(_lib.Mt3Error, match="note rule and a token mask in use leave fewer than")
    try:
        eng.set_token_grammar(GRAMMAR)                   # the event grammar alone has room under every one of them
        for m in (one, many, three):
            eng.set_token_masks(m)
            eng.encode(lm)
            eng.decode(num_steps=S)
        eng.clear_token_grammar()
        eng.set_note_grammar(NOTES)
        eng.set_token_masks(one)
        eng.encode(lm)
        for kw in (dict(), dict(beam1=True), dict(early_exit=True)):
            with refused:
                eng.decode(num_steps=S, **kw)
        with refused:
            eng.transcribe(lm, num_steps=S)
        eng.set_token_masks(three)                      # EOS and two programs: 3 >= 2, 3 < 2k = 4
        eng.decode(num_steps=S)
        eng.transcribe(lm, num_steps=S, beam1=True)
        eng.encode(lm[:4], num_beams=2)
        with refused:
            eng.decode_beams(2, num_steps=S)
        with refused:
            eng.transcribe(lm, num_steps=S, num_beams=2)
        eng.set_token_masks(many)
        eng.decode_beams(2, num_steps=S)
        eng.clear_token_masks()
        bad = vocabularies.note_grammar(CODEC, V, TIES, 204)
        bad.g.with_ties = 0
        with pytest.raises(_lib.Mt3Error, match="tie section"):
            eng.set_note_grammar(bad)
        assert eng.status(_lib.STATUS_NOTE_GRAMMAR) == 1
        eng.encode(lm)
        want = eng.decode(num_steps=S).clone()
        eng.decode(num_steps=S, wait=False)
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_set_note_grammar: a decode is in flight"):
            eng.clear_note_grammar()
        assert torch.equal(eng.decode_wait(), want)
    finally:
        eng.clear_note_grammar()
        eng.clear_token_grammar()
        eng.clear_token_masks()
