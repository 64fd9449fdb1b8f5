"""Constrained decoding through the engine (mt3_engine_set_token_masks): tiny random-weight engines, f32 and bf16, the
e4m3 caches once; at most 16 steps.  An all-ones mask changes no bit; a mask is obeyed and the pick is the arg-max over
the allowed tokens of the model's own (unmasked) logits; the mask follows its segment through refills and row groups;
set / grow / clear leave no stale graph behind; teacher forcing and scoring ignore masks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, network, spectrograms, synthetic  # noqa: E402

L, S, V = 64, 16, 1536
WORDS = V // 32


def _engine(dtype, B, kv="", seed=5):
    cfg = network.T5Config(dtype=dtype, kv_dtype=kv, num_encoder_layers=1, num_decoder_layers=2)
    params = network.init_random_params(cfg, seed=seed, norm_scale_jitter=0.1)
    eng = network.Transformer(cfg, input_length=256, max_decode_length=L, max_batch=B)
    eng.load_params(params)
    return eng


def _lm(n, seed=21):
    return spectrograms.compute_spectrogram_batch(synthetic.synth_audio(n, seed=seed), None)


def _mask(forbid=()):
    m = np.full(WORDS, 0xFFFFFFFF, np.uint32)
    for i in forbid:
        m[i >> 5] &= np.uint32(~(1 << (i & 31)) & 0xFFFFFFFF)
    return m


def _emitted(ids, n=6):
    """up to n distinct ids > 1 the rows emitted before their EOS"""
    out = []
    for row in ids.cpu().numpy()[:, :S]:
        for t in row:
            if t == 1:
                break
            if t > 1 and t not in out:
                out.append(int(t))
    return out[:n]


def _allowed(mask):
    return np.array([(int(mask[i >> 5]) >> (i & 31)) & 1 for i in range(V)], bool)


ENGINES = [("float32", ""), ("bfloat16", ""), ("bfloat16", "fp8_e4m3")]


@pytest.mark.parametrize("dtype,kv", ENGINES)
def test_all_ones_mask_changes_no_bit(dtype, kv):
    eng, lm = _engine(dtype, 8, kv), _lm(11)

    def everything():
        out = []
        eng.encode(lm[:8])
        out += [eng.decode(num_steps=S), eng.decode(num_steps=S, beam1=True, early_exit=True)]
        eng.encode(lm[:4], num_beams=2)
        out += list(eng.decode_beams(2, num_steps=S, return_all=True))
        out += [eng.transcribe(lm, num_steps=S), eng.transcribe(lm, num_steps=S, beam1=True)]
        out += list(eng.transcribe(lm, num_steps=S, num_beams=2, return_all=True))
        return [o.clone() for o in out]

    plain = everything()
    eng.set_token_masks(_mask())
    assert eng.status(_lib.STATUS_TOKEN_MASKS) == 1
    masked = everything()
    eng.clear_token_masks()
    assert eng.status(_lib.STATUS_TOKEN_MASKS) == 0
    for i, (a, b) in enumerate(zip(plain, masked)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i


@pytest.mark.parametrize("dtype,kv", ENGINES[:2])
def test_greedy_rule_end_to_end(dtype, kv):
    eng, lm = _engine(dtype, 8, kv), _lm(8)
    eng.encode(lm)
    plain, first = eng.decode(num_steps=S, return_first_logits=True)
    forbid = _emitted(plain)
    assert forbid
    mask = _mask(forbid)
    eng.set_token_masks(mask)
    try:
        ids, first_m = eng.decode(num_steps=S, return_first_logits=True)
        assert torch.equal(first, first_m)                   # the logits handed back stay unmasked
        assert not np.isin(ids.cpu().numpy()[:, :S], forbid).any()
        assert not torch.equal(ids, plain)
        forced_ids, logits = eng.decode_forced(ids, num_steps=S)        # ignores the mask: the model's own logits
    finally:
        eng.clear_token_masks()
    ok = _allowed(mask)
    lg, got = logits.cpu().numpy(), ids.cpu().numpy()                   # [S, B, V]
    assert np.isfinite(lg).all()
    for b in range(got.shape[0]):
        for t in range(S):
            want = int(np.argmax(np.where(ok, lg[t, b], -np.inf)))       # np.argmax: the lowest id on ties
            assert got[b, t] == want, (b, t)
            if want == 1:
                assert (got[b, t + 1:] == 0).all()
                break


def _alone(eng, lm, i, mask, **kw):
    eng.encode(lm[i:i + 1], num_beams=kw.get("k", 1))
    if mask is None:
        eng.clear_token_masks()
    else:
        eng.set_token_masks(mask)
    if "k" in kw:
        return eng.decode_beams(kw["k"], num_steps=S, early_exit=True, return_all=True)
    return eng.decode(num_steps=S, early_exit=True, beam1=kw["beam1"])


@pytest.mark.parametrize("dtype,kv", ENGINES)
def test_the_mask_follows_the_segment(dtype, kv):
    eng, lm = _engine(dtype, 4, kv), _lm(11)
    plain = eng.transcribe(lm, num_steps=S)
    em = _emitted(plain, 8)
    assert len(em) >= 2
    masks = np.stack([_mask(em[0::2]), _mask(em[1::2])])
    seg = np.array(([0, 1, -1] * 4)[:11], np.int32)
    try:
        for beam1 in (False, True):
            want = []
            for i in range(11):
                want.append(_alone(eng, lm, i, None if seg[i] < 0 else masks[seg[i]], beam1=beam1)[0].clone())
            want = torch.stack(want)
            eng.set_token_masks(masks, seg)
            for use_graph in (True, False):
                got = eng.transcribe(lm, num_steps=S, beam1=beam1, use_graph=use_graph)
                assert torch.equal(got, want), (beam1, use_graph, (got != want).any(1).nonzero().flatten().tolist())
                assert eng.transcribe_stats["used_graph"] == (1 if use_graph else 0)
                assert eng.transcribe_stats["slots"] == 4 and eng.transcribe_stats["refills"] == 7
            if not beam1:
                assert not torch.equal(got, plain)
                g = got.cpu().numpy()
                for i in range(11):
                    if seg[i] >= 0:
                        assert _allowed(masks[seg[i]])[g[i]].all(), i
        # k = 2: 5 segments through 2 elements
        want_ids, want_sc = [], []
        for i in range(5):
            a, sc = _alone(eng, lm, i, None if seg[i] < 0 else masks[seg[i]], k=2)
            want_ids.append(a[0].clone())
            want_sc.append(sc[0].clone())
        eng.set_token_masks(masks, seg[:5])
        for use_graph in (True, False):
            got, sc = eng.transcribe(lm[:5], num_steps=S, num_beams=2, return_all=True, use_graph=use_graph)
            assert torch.equal(got, torch.stack(want_ids)) and torch.equal(sc, torch.stack(want_sc)), use_graph
            assert eng.transcribe_stats["used_graph"] == (1 if use_graph else 0)
            assert eng.transcribe_stats["slots"] == 4
        assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0
    finally:
        eng.clear_token_masks()


def test_row_groups_carry_per_row_masks():
    eng, lm = _engine("float32", 128), _lm(128)
    eng.encode(lm)
    plain = eng.decode(num_steps=8)
    em = _emitted(plain, 8)
    masks = np.stack([_mask(em[0::2]), _mask(em[1::2])])
    seg = np.zeros(128, np.int32)
    seg[60:70] = [1, -1, 1, 1, 0, 1, -1, 0, 1, 1]             # the group boundary is row 64
    seg[100:] = 1
    eng.set_token_masks(masks, seg)
    try:
        one = eng.decode(num_steps=8, single_stream=True)
        two = eng.decode(num_steps=8)
        assert eng.status(_lib.STATUS_LAST_DECODE_GROUPS) == 2
        assert torch.equal(one, two)
        early = eng.decode(num_steps=8, early_exit=True, beam1=True)
        early1 = eng.decode(num_steps=8, early_exit=True, beam1=True, single_stream=True)
        assert torch.equal(early, early1)
        eng.decode(num_steps=8, wait=False)                   # MT3_DECODE_ASYNC: set / clear are refused meanwhile
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_set_token_masks: a decode is in flight"):
            eng.clear_token_masks()
        assert torch.equal(eng.decode_wait(), two)
    finally:
        eng.clear_token_masks()
    g = two.cpu().numpy()
    assert not torch.equal(two, plain)
    for i in range(128):
        if seg[i] >= 0:
            assert _allowed(masks[seg[i]])[g[i, :8]].all(), i
        else:
            assert np.array_equal(g[i], plain.cpu().numpy()[i])


def test_set_grow_clear_with_graphs_and_refusals():
    eng, lm = _engine("float32", 8), _lm(8)
    eng.encode(lm)
    first = eng.decode(num_steps=S)
    em = _emitted(first, 6)
    m0, m1, m2 = _mask(em[:2]), _mask(em[2:4]), _mask(em[4:6])
    eng.set_token_masks(m0)
    second = eng.decode(num_steps=S)
    assert not np.isin(second.cpu().numpy()[:, :S], em[:2]).any() and not torch.equal(second, first)
    seg = np.array([2, 1, 0, -1, 2, 1, 0, -1], np.int32)
    eng.set_token_masks(np.stack([m0, m1, m2]), seg)         # more masks, and a per-segment index: larger arrays
    assert eng.status(_lib.STATUS_TOKEN_MASKS) == 3
    third = eng.decode(num_steps=S).cpu().numpy()
    for i in range(8):
        if seg[i] >= 0:
            assert _allowed((m0, m1, m2)[seg[i]])[third[i, :S]].all(), i
        else:
            assert np.array_equal(third[i], first.cpu().numpy()[i])
    # the calls' own refusals, before any device work
    with pytest.raises(_lib.Mt3Error, match="mt3_engine_transcribe: more rows or segments than the token masks"):
        eng.transcribe(_lm(9), num_steps=S)
    eng.set_token_masks(np.stack([m0, m1]), seg[:4] % 2)
    with pytest.raises(_lib.Mt3Error, match="mt3_engine_decode: more rows or segments than the token masks"):
        eng.decode(num_steps=S)
    few = np.zeros(WORDS, np.uint32)
    few[0] = 0b1011                                          # EOS and two more: enough for greedy, not for 2 beams
    eng.set_token_masks(few)
    eng.decode(num_steps=4)
    eng.encode(lm[:4], num_beams=2)
    with pytest.raises(_lib.Mt3Error, match="mt3_engine_decode_beams: a token mask in use allows fewer than 2 \\* num_beams"):
        eng.decode_beams(2, num_steps=S)
    with pytest.raises(_lib.Mt3Error, match="mt3_engine_transcribe_beams: a token mask in use allows fewer"):
        eng.transcribe(lm[:4], num_steps=S, num_beams=2)
    eng.clear_token_masks()
    assert eng.status(_lib.STATUS_TOKEN_MASKS) == 0
    eng.encode(lm)
    assert torch.equal(eng.decode(num_steps=S), first)


def test_one_mask_after_indexed_masks_leaves_no_stale_graph():
    """The step graphs hold whether the per-segment index is in use: a single mask without an index fits the arrays three
    indexed masks left, so no new address forces the drop -- the change of form must."""
    eng, lm = _engine("float32", 8), _lm(8)
    eng.encode(lm)
    first = eng.decode(num_steps=S)
    em = _emitted(first, 6)
    assert len(em) >= 3
    seg = np.array([2, 1, 0, -1, 2, 1, 0, -1], np.int32)
    try:
        eng.set_token_masks(np.stack([_mask(em[:2]), _mask(em[2:4]), _mask(em[4:6])]), seg)
        eng.decode(num_steps=S)
        assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
        one = _mask(em)                                      # forbids what every row emitted, the unindexed rows included
        eng.set_token_masks(one)
        assert eng.status(_lib.STATUS_TOKEN_MASKS) == 1
        got = eng.decode(num_steps=S).clone()
        assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
        assert torch.equal(eng.decode(num_steps=S, use_graph=False), got)
        assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 0
        assert _allowed(one)[got.cpu().numpy()[:, :S]].all()
    finally:
        eng.clear_token_masks()
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0


def test_forced_decode_and_scoring_ignore_masks():
    eng, lm = _engine("float32", 8), _lm(8)
    eng.encode(lm)
    ids = eng.decode(num_steps=S)
    tgt = ids[:, :S].contiguous()

    def all_three():
        eng.encode(lm)
        f_ids, f_logits = eng.decode_forced(ids, num_steps=S)
        sc = eng.score(tgt, return_token_scores=True)
        ss = eng.score_segments(lm, tgt, return_token_scores=True, return_top1=True)
        return [f_ids, f_logits] + [x.clone() for x in list(sc) + list(ss) if x is not None]

    plain = all_three()
    eng.set_token_masks(_mask(_emitted(ids)))
    try:
        masked = all_three()
    finally:
        eng.clear_token_masks()
    for i, (a, b) in enumerate(zip(plain, masked)):
        assert torch.equal(a, b), i
