"""Well-formed decoding through the engine (mt3_engine_set_token_grammar): the tiny random-weight engines of
tests/test_gpu_token_mask_engine.py (one encoder layer, two decoder layers, L = 64, 16 steps), f32 and bf16, the e4m3
caches once; the real `mt3` codec with max_steps = 204.  Half the segments carry the bare-`tie` prompt, so both phases of
the grammar (inside the tie section, after it) are reached within 16 steps.

Seeds: engine seed 5, audio seed 21 -- with them the PLAIN decode of the same segments is not accepted by the grammar
(asserted below as the precondition of (c)); a seed that failed it would be replaced here."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, inference, network, note_sequences, spectrograms, synthetic, vocabularies  # noqa: E402
from tests import grammar_ref as gr  # noqa: E402

L, S, V = 64, 16, 1536
CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
ENGINES = [("float32", ""), ("bfloat16", ""), ("bfloat16", "fp8_e4m3")]
CODEC = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
GRAMMAR = vocabularies.token_grammar(CODEC, V, note_sequences.NoteEncodingWithTiesSpec, 204)
G = gr.from_struct(GRAMMAR)
TIE = vocabularies.tie_section_prompt(CODEC, [])


def _engine(dtype, B, kv="", seed=5):
    cfg = network.T5Config(dtype=dtype, kv_dtype=kv, num_encoder_layers=1, num_decoder_layers=2)
    params = network.init_random_params(cfg, seed=seed, norm_scale_jitter=0.1)
    eng = network.Transformer(cfg, input_length=256, max_decode_length=L, max_batch=B)
    eng.load_params(params)
    return eng


def _lm(n, seed=21):
    return spectrograms.compute_spectrogram_batch(synthetic.synth_audio(n, seed=seed), None)


def _prompt_index(n):
    """every second segment opens with the bare tie"""
    return [0 if i % 2 == 0 else -1 for i in range(n)]


def _plen(i):
    return 1 if i % 2 == 0 else 0


def _everything(eng, lm):
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
    eng.set_prompts(None)
    return [o.clone() for o in out]


def _rows(out, n):
    """(segment, id row) of every decode in `_everything`'s outputs: greedy, beam-1, all k of decode_beams, transcribe
    greedy / beam-1, all k of the beam transcribe (out[3] and out[7] are the beam calls' scores)"""
    rows = []
    for o in (out[0], out[1], out[4], out[5]):
        rows += [(i, r) for i, r in enumerate(o.cpu().numpy()[:, :S])]
    for o in (out[2], out[6]):
        rows += [(i, r) for i, d in enumerate(o.cpu().numpy()) for r in d[:, :S]]
    return rows


@pytest.mark.parametrize("dtype,kv", ENGINES)
def test_off_changes_no_bit_and_on_is_well_formed(dtype, kv):
    """(a) set and clear leave every decode as it was, bit for bit; (c) with the grammar every emitted row, all k decodes of
    the beam calls included, is accepted -- and the plain decode of the same segments is not; (f) set, clear, set again
    leave no stale graph: the decodes replay graphs and the fallback count stays"""
    eng, lm = _engine(dtype, 8, kv), _lm(11)
    plain = _everything(eng, lm)
    fallbacks = eng.status(_lib.STATUS_GRAPH_FALLBACKS)
    eng.set_token_grammar(GRAMMAR)
    assert eng.status(_lib.STATUS_TOKEN_GRAMMAR) == 1
    formed = _everything(eng, lm)
    assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
    eng.clear_token_grammar()
    assert eng.status(_lib.STATUS_TOKEN_GRAMMAR) == 0
    again = _everything(eng, lm)
    for i, (a, b) in enumerate(zip(plain, again)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
    eng.set_token_grammar(GRAMMAR)
    formed2 = _everything(eng, lm)
    assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
    eng.clear_token_grammar()
    for i, (a, b) in enumerate(zip(formed, formed2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == fallbacks
    # the precondition: the plain decode breaks the grammar on at least half of its rows, and in BOTH phases -- among the
    # rows that open with the tie prompt (behind the section from step 1) as among those that start inside the section
    bad = [(i, not gr.accepts(G, r, _plen(i))) for i, r in _rows(plain, len(lm))]
    assert 2 * sum(b for _, b in bad) >= len(bad)
    assert any(b for i, b in bad if _plen(i) == 1) and any(b for i, b in bad if _plen(i) == 0)
    for i, r in _rows(formed, len(lm)):
        assert gr.accepts(G, r, _plen(i)), (i, list(r))


@pytest.mark.parametrize("dtype,kv", ENGINES[:2])
def test_greedy_rule_end_to_end(dtype, kv):
    """(b) decode_forced on the emitted ids gives the model's own logits (it ignores the grammar); at every free step the
    emitted id is the arg-max of those logits over allowed_vector(state), the state replayed by grammar_ref"""
    eng, lm = _engine(dtype, 8, kv), _lm(8)
    eng.encode(lm)
    eng.set_prompts([TIE], _prompt_index(8))
    eng.set_token_grammar(GRAMMAR)
    try:
        ids = eng.decode(num_steps=S)
        _, logits = eng.decode_forced(ids, num_steps=S)
    finally:
        eng.clear_token_grammar()
        eng.set_prompts(None)
    lg, got = logits.cpu().numpy(), ids.cpu().numpy()
    assert np.isfinite(lg).all()
    for b in range(8):
        state = gr.initial(G)
        for t in range(S):
            if t < _plen(b):
                want = TIE[t]
            else:
                want = int(np.argmax(np.where(gr.allowed_vector(G, state, V), lg[t, b], -np.inf)))
            assert got[b, t] == want, (b, t)
            state = gr.advance(G, state, want)
            if want == 1:
                assert (got[b, t + 1:] == 0).all()
                break


@pytest.mark.parametrize("dtype,kv", ENGINES)
def test_state_is_reset_on_refill_and_travels_with_compaction(dtype, kv):
    """(d) 11 segments through 8 slots give, per segment, the bits of the segment decoded alone (greedy, beam-1, k = 2);
    (e) the early exit with compaction gives the ids of the schedule without it, up to each row's EOS"""
    eng, lm = _engine(dtype, 8, kv), _lm(11)
    eng.set_token_grammar(GRAMMAR)
    try:
        eng.set_prompts([TIE], _prompt_index(11))
        job = [eng.transcribe(lm, num_steps=S).clone(), eng.transcribe(lm, num_steps=S, beam1=True).clone()]
        job_k = [o.clone() for o in eng.transcribe(lm, num_steps=S, num_beams=2, return_all=True)]
        for i in range(11):
            eng.set_prompts([TIE], [0 if i % 2 == 0 else -1])
            eng.encode(lm[i:i + 1])
            assert torch.equal(eng.decode(num_steps=S, early_exit=True)[0], job[0][i]), i
            assert torch.equal(eng.decode(num_steps=S, early_exit=True, beam1=True)[0], job[1][i]), i
            # k = 2: the segment with no other segment beside it, in the launch shape of the job (4 elements = 8 rows: the
            # bf16 products depend on the number of rows of a launch, the scores are compared bit for bit)
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
    finally:
        eng.clear_token_grammar()
        eng.set_prompts(None)


def test_inference_model_well_formed():
    """(g) InferenceModel(...)(audio, well_formed=True) on a short synthetic file returns notes and drops no event"""
    audio = synthetic.synth_music(3 * 2.048 - 0.3, seed=13, device="cpu")[1]
    m = inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32", decoding="greedy")
    ns = m(audio, well_formed=True)
    assert len(ns.notes) > 0
    assert m.last_event_counts["dropped_events"] == 0
    assert m.model.status(_lib.STATUS_TOKEN_GRAMMAR) == 0                # cleared after the call


def _mask_words(forbid):
    m = np.full(V // 32, 0xFFFFFFFF, np.uint32)
    for i in forbid:
        m[i >> 5] &= np.uint32(~(1 << (i & 31)) & 0xFFFFFFFF)
    return m


def test_decodes_refuse_a_mask_that_leaves_the_grammar_no_room():
    """MT3_ERR_INVALID, before any device work, from decode / transcribe for a mask in use that leaves 1 id in the tie
    section, from decode_beams / transcribe_beams for one that leaves 2k - 1; the same masks are accepted where they are not
    in use, without a tie section (with_ties = 0), or by the calls that need fewer ids.  And a set or clear while a decode
    is in flight is refused."""
    eng, lm = _engine("float32", 8), _lm(8)
    section = list(range(G.pitch_first, G.pitch_first + G.pitch_count)) + \
        list(range(G.program_first, G.program_first + G.program_count)) + [G.tie_id]
    only_eos = _mask_words(section)                                              # the tie section keeps EOS alone
    three = _mask_words([i for i in section if i not in (G.tie_id, G.pitch_first)])   # EOS, tie, one pitch: 2k - 1 at k = 2
    all_ones = _mask_words([])
    no_ties = vocabularies.token_grammar(CODEC, V, note_sequences.NoteEncodingSpec, 204)
    refused = pytest.raises(_lib.Mt3Error, match="leave fewer than")
    try:
        eng.set_token_grammar(GRAMMAR)
        eng.set_token_masks(only_eos)
        eng.encode(lm)
        for kw in (dict(), dict(beam1=True), dict(early_exit=True)):
            with refused:
                eng.decode(num_steps=S, **kw)
        for kw in (dict(), dict(beam1=True)):
            with refused:
                eng.transcribe(lm, num_steps=S, **kw)
        # per segment: refused where the mask is in use among the job's segments, accepted where it is not
        eng.set_token_masks(np.stack([all_ones, only_eos]), [0] * 7 + [1])
        with refused:
            eng.decode(num_steps=S)
        eng.encode(lm[:7])
        eng.decode(num_steps=S)
        eng.transcribe(lm[:7], num_steps=S)
        with refused:
            eng.transcribe(lm, num_steps=S)
        # the beam calls need 2k
        eng.set_token_masks(three)
        eng.encode(lm)
        eng.decode(num_steps=S)                                                 # 3 >= 2
        eng.transcribe(lm, num_steps=S, beam1=True)
        eng.encode(lm[:4], num_beams=2)
        with refused:
            eng.decode_beams(2, num_steps=S)
        with refused:
            eng.transcribe(lm, num_steps=S, num_beams=2)
        eng.encode(lm[:8], num_beams=1)
        eng.decode_beams(1, num_steps=S)                                        # 3 >= 2k = 2
        # without a tie section the same masks leave room
        eng.set_token_grammar(no_ties)
        eng.encode(lm[:4], num_beams=2)
        eng.decode_beams(2, num_steps=S)
        eng.transcribe(lm, num_steps=S, num_beams=2)
        eng.set_token_masks(only_eos)
        eng.encode(lm)
        eng.decode(num_steps=S)
        eng.transcribe(lm, num_steps=S)
        # a decode in flight: set and clear are refused meanwhile, and the grammar stays as it was
        eng.clear_token_masks()
        eng.set_token_grammar(GRAMMAR)
        want = eng.decode(num_steps=S).clone()
        eng.decode(num_steps=S, wait=False)
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_set_token_grammar: a decode is in flight"):
            eng.clear_token_grammar()
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_set_token_grammar: a decode is in flight"):
            eng.set_token_grammar(no_ties)
        assert torch.equal(eng.decode_wait(), want)
        assert eng.status(_lib.STATUS_TOKEN_GRAMMAR) == 1
    finally:
        eng.clear_token_grammar()
        eng.clear_token_masks()
