"""Prompted decoding through the engine (mt3_engine_set_prompts): MT3-shaped random-weight engines, max_decode_len 64, 48
steps, batch 8.  A row prompted with its own unprompted prefix decodes the same ids bit for bit (f32, bf16, bf16 with e4m3
K/V caches); after an arbitrary prompt every id is the lowest-id arg-max of the teacher-forced logits of the same row; the
k-beam scores are the free tokens' log-probs over the absolute-length brevity penalty; every schedule gives the same ids;
a prompt follows its segment through refills; clearing restores the unprompted decode; masks hold from t = p; and
InferenceModel's `prompts=` on the trained fixture."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, inference, network, spectrograms, synthetic, vocabularies  # noqa: E402

L, S, B, V = 64, 48, 8, 1536
CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
ENGINES = [("float32", ""), ("bfloat16", ""), ("bfloat16", "fp8_e4m3")]


def _engine(dtype, batch, kv="", seed=0, length=L):
    cfg = network.T5Config(dtype=dtype, kv_dtype=kv)
    eng = network.Transformer(cfg, input_length=256, max_decode_length=length, max_batch=batch)
    eng.load_params(network.init_random_params(network.T5Config(dtype=dtype), seed=seed, norm_scale_jitter=0.2))
    return eng


def _lm(n, seed=21):
    return spectrograms.compute_spectrogram_batch(synthetic.synth_audio(n, seed=seed), None)


def _eos_at(row, steps=S):
    e = np.flatnonzero(row[:steps] == 1)
    return int(e[0]) if e.size else steps


def _random_prompts(n, lengths, seed=3):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.integers(3, 1391, lengths[i % len(lengths)])] or None for i in range(n)]


def _set(eng, prompts):
    """per-row prompts (None: none) -> set_prompts rows + index"""
    rows = [p for p in prompts if p]
    index, at = [], 0
    for p in prompts:
        index.append(at if p else -1)
        at += 1 if p else 0
    eng.set_prompts(rows, index)


@pytest.mark.parametrize("dtype,kv", ENGINES)
def test_a_row_prompted_with_its_own_prefix_decodes_the_same_ids(dtype, kv):
    eng, lm = _engine(dtype, B, kv), _lm(B)
    eng.encode(lm)
    for beam1 in (False, True):
        U = eng.decode(num_steps=S, beam1=beam1).clone()
        u = U.cpu().numpy()
        prompts = []
        for b, p in enumerate([0, 1, 7, 20, 20, 7, 1, 0]):
            p = min(p, _eos_at(u[b]))                      # cut before the row's EOS
            prompts.append([int(x) for x in u[b, :p]] or None)
        assert sum(1 for p in prompts if p) >= 4 and all(min(p) >= 2 for p in prompts if p)
        _set(eng, prompts)
        try:
            assert eng.status(_lib.STATUS_PROMPTS) == sum(1 for p in prompts if p)
            got = eng.decode(num_steps=S, beam1=beam1)
            assert torch.equal(got, U), (dtype, kv, beam1, (got != U).any(1).nonzero().flatten().tolist())
            assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
        finally:
            eng.set_prompts(None)
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0


def test_arbitrary_prompts_then_the_models_own_argmax():
    eng, lm = _engine("float32", B), _lm(B)
    eng.encode(lm)
    prompts = _random_prompts(B, [0, 1, 7, 20])
    _set(eng, prompts)
    try:
        ids, first = eng.decode(num_steps=S, return_first_logits=True)
        ids = ids.clone()
    finally:
        eng.set_prompts(None)
    _, first_plain = eng.decode(num_steps=S, return_first_logits=True)
    assert torch.equal(first, first_plain)                 # the logits handed back are the model's own
    _, logits = eng.decode_forced(ids, num_steps=S)        # the same step kernels on the same inputs: exact
    got, lg = ids.cpu().numpy(), logits.cpu().numpy()
    for b in range(B):
        p = len(prompts[b] or [])
        assert list(got[b, :p]) == (prompts[b] or [])
        for t in range(p, S):
            want = int(np.argmax(lg[t, b]))                # np.argmax: the lowest id on ties
            assert got[b, t] == want, (b, t)
            if want == 1:
                assert (got[b, t + 1:] == 0).all()
                break


def test_k_beam_prompts_scores_and_forks():
    k, n = 4, 4
    eng, lm = _engine("float32", n * k, seed=1), _lm(n, seed=33)
    prompts = _random_prompts(n, [7, 0, 20, 1], seed=9)
    eng.encode(lm, num_beams=k)
    _set(eng, prompts)
    try:
        all_ids, scores = eng.decode_beams(k, num_steps=S, return_all=True)
        all_ids, scores = all_ids.cpu().numpy()[:, :, :S], scores.cpu().numpy()
        assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
        eng.encode(lm, num_beams=k)
        _, tok = eng.score(all_ids.reshape(n * k, S), return_token_scores=True)        # ignores prompts
        tok = tok.cpu().numpy().astype(np.float64).reshape(n, k, S)
        checked = 0
        for b in range(n):
            p = len(prompts[b] or [])
            for j in range(k):
                ids, sc = all_ids[b, j], float(scores[b, j])
                if sc < -1e6:
                    continue                               # unfilled finished entry
                assert list(ids[:p]) == (prompts[b] or []), (b, j)
                eos = np.flatnonzero(ids == 1)
                m = int(eos[0]) + 1 if eos.size else S
                if np.any(ids[:m] == 0):
                    continue
                want = tok[b, j, p:m].sum() / (((5.0 + m) / 6.0) ** 0.6 if eos.size else 1.0)
                assert abs(sc - want) <= 1e-5 * abs(want), (b, j, sc, want)
                checked += 1
        assert checked >= n * k // 2
        # every element prompted with the same length: nothing forks before step p
        p = 12
        eng.set_prompts(_random_prompts(n, [p], seed=4), list(range(n)))
        eng.encode(lm, num_beams=k)
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_decode_beams: num_steps must exceed the longest prompt in use"):
            eng.decode_beams(k, num_steps=p)
        eng.decode_beams(k, num_steps=p + 1)
        one_free = eng.status(_lib.STATUS_LAST_DECODE_FORKS)
        assert one_free <= n * (k - 1)                     # the forks of step p alone: at most k - 1 per element
        eng.set_prompts(None)
        eng.decode_beams(k, num_steps=p + 1)
        assert eng.status(_lib.STATUS_LAST_DECODE_FORKS) > one_free
    finally:
        eng.set_prompts(None)
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0


def test_schedules_give_equal_ids():
    eng, lm = _engine("float32", B), _lm(B)
    eng.encode(lm)
    prompts = _random_prompts(B, [0, 1, 7, 20], seed=5)
    _set(eng, prompts)
    try:
        for beam1 in (False, True):
            ref = eng.decode(num_steps=S, beam1=beam1).clone()
            assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
            assert torch.equal(eng.decode(num_steps=S, beam1=beam1, use_graph=False), ref)
            assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 0
            early = eng.decode(num_steps=S, beam1=beam1, early_exit=True).cpu().numpy()
            r = ref.cpu().numpy()
            for b in range(B):
                e = _eos_at(r[b]) + 1
                assert np.array_equal(early[b, :e], r[b, :e]), (beam1, b)
                assert e > len(prompts[b] or [])           # never closed inside its prompt
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_decode: num_steps must exceed the longest prompt in use"):
            eng.decode(num_steps=20)
        eng.set_prompts([[5, 6, 7]], [0, -1, 0])
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_decode: more rows or segments than the prompts' n_segments"):
            eng.decode(num_steps=S)
    finally:
        eng.set_prompts(None)
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0


def test_row_groups_carry_per_row_prompts():
    n, steps = 128, 24
    eng, lm = _engine("float32", n, length=32), _lm(n)
    eng.encode(lm)
    prompts = _random_prompts(n, [0, 1, 7, 20, 3], seed=6)
    _set(eng, prompts)
    try:
        one = eng.decode(num_steps=steps, single_stream=True).clone()
        two = eng.decode(num_steps=steps)
        assert eng.status(_lib.STATUS_LAST_DECODE_GROUPS) == 2
        assert torch.equal(one, two)
        g = two.cpu().numpy()
        for b in range(n):
            p = prompts[b] or []
            assert list(g[b, :len(p)]) == p, b
        e1 = eng.decode(num_steps=steps, early_exit=True, beam1=True).clone()
        e2 = eng.decode(num_steps=steps, early_exit=True, beam1=True, single_stream=True)
        assert torch.equal(e1, e2)
        eng.decode(num_steps=steps, wait=False)            # MT3_DECODE_ASYNC: set / clear are refused meanwhile
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_set_prompts: a decode is in flight"):
            eng.set_prompts(None)
        assert torch.equal(eng.decode_wait(), two)
    finally:
        eng.set_prompts(None)
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0


def _alone(eng, lm, i, prompt, **kw):
    eng.encode(lm[i:i + 1], num_beams=kw.get("k", 1))
    eng.set_prompts([prompt] if prompt else None)
    if "k" in kw:
        return eng.decode_beams(kw["k"], num_steps=S, early_exit=True, return_all=True)
    return eng.decode(num_steps=S, early_exit=True, beam1=kw["beam1"])


@pytest.mark.parametrize("dtype,kv", ENGINES[:1])
def test_a_prompt_follows_its_segment_through_refills(dtype, kv):
    """20 segments through 8 slots against each segment decoded ALONE.  f32 only: the reference is a 1-row decode, and on
    this 8-layer model the bf16 step is not the same bit for bit at 1 row and at 8 rows: with NO prompt set at all, the bf16
    in-flight job differs from the 1-row decodes in 9 of these 20 rows (0, 4, 8, 9, 11, 14, 17, 18, 19; measured on an
    MI355X), so that comparison says nothing about prompts there.  bf16 and the e4m3 caches are held to bit identity in
    the same-batch tests above."""
    n = 20
    eng, lm = _engine(dtype, B, kv), _lm(n)
    lens = [7, 0, 0, 1, 20, 0, 0, 0, 3, 0, 12, 0, 0, 7, 0, 1, 0, 0, 20, 5]      # segments 8 .. 19 arrive by refill
    prompts = [p or None for p in (_random_prompts(1, [m], seed=40 + i)[0] if m else None for i, m in enumerate(lens))]
    try:
        for beam1 in (False, True):
            want = torch.stack([_alone(eng, lm, i, prompts[i], beam1=beam1)[0].clone() for i in range(n)])
            _set(eng, prompts)
            for use_graph in (True, False):
                got = eng.transcribe(lm, num_steps=S, beam1=beam1, use_graph=use_graph)
                assert torch.equal(got, want), (beam1, use_graph, (got != want).any(1).nonzero().flatten().tolist())
                assert eng.transcribe_stats["used_graph"] == (1 if use_graph else 0)
                assert eng.transcribe_stats["slots"] == B and eng.transcribe_stats["refills"] >= n - B
            g = got.cpu().numpy()
            for i in range(n):
                assert list(g[i, :len(prompts[i] or [])]) == (prompts[i] or []), i
        # k = 2: 10 segments through 4 elements
        m = 10
        want_ids, want_sc = [], []
        for i in range(m):
            a, sc = _alone(eng, lm, i, prompts[i], k=2)
            want_ids.append(a[0].clone())
            want_sc.append(sc[0].clone())
        _set(eng, prompts[:m])
        got, sc = eng.transcribe(lm[:m], num_steps=S, num_beams=2, return_all=True)
        assert torch.equal(got, torch.stack(want_ids)) and torch.equal(sc, torch.stack(want_sc))
        assert eng.transcribe_stats["used_graph"] == 1 and eng.transcribe_stats["slots"] == B
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_transcribe: more rows or segments than the prompts"):
            eng.transcribe(lm, num_steps=S)
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_transcribe_beams: num_steps must exceed the longest prompt"):
            eng.transcribe(lm[:m], num_steps=20, num_beams=2)
        assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0
    finally:
        eng.set_prompts(None)


def test_clearing_restores_the_unprompted_decode():
    eng, lm = _engine("float32", B), _lm(B)
    eng.encode(lm)
    before = eng.decode(num_steps=S).clone()
    used = eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH)
    eng.set_prompts([[9, 8, 7]])
    assert eng.status(_lib.STATUS_PROMPTS) == 1
    mid = eng.decode(num_steps=S)
    assert (mid[:, :3].cpu() == torch.tensor([9, 8, 7], dtype=torch.int32)).all() and not torch.equal(mid, before)
    eng.set_prompts(_random_prompts(B, [5, 30], seed=8), list(range(B)))      # more prompts, a longer stride, an index
    assert eng.status(_lib.STATUS_PROMPTS) == B
    eng.decode(num_steps=S)
    # teacher forcing and scoring ignore prompts
    f_ids, f_logits = eng.decode_forced(before, num_steps=S)
    sc = eng.score(before[:, :S].contiguous())
    eng.set_prompts(None)
    assert eng.status(_lib.STATUS_PROMPTS) == 0
    after = eng.decode(num_steps=S)
    assert torch.equal(after, before) and eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == used
    f_ids2, f_logits2 = eng.decode_forced(before, num_steps=S)
    assert torch.equal(f_ids, f_ids2) and torch.equal(f_logits, f_logits2)
    assert torch.equal(sc, eng.score(before[:, :S].contiguous()))
    eng.set_prompts([])                                                       # [] clears as None does
    assert eng.status(_lib.STATUS_PROMPTS) == 0 and eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0


def test_another_stride_or_form_within_capacity_leaves_no_stale_graph():
    """The step graphs hold the prompts' stride and whether the index is in use: a set call that changes either without
    growing an array (so no new address forces it) must still drop them."""
    eng, lm = _engine("float32", B), _lm(B)
    eng.encode(lm)

    def graph_equals_direct_and_rows_begin_with(prompts):
        got = eng.decode(num_steps=S).clone()
        assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
        assert torch.equal(eng.decode(num_steps=S, use_graph=False), got)
        assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 0
        g = got.cpu().numpy()
        for b in range(B):
            assert list(g[b, :len(prompts[b])]) == prompts[b], b

    try:
        wide = _random_prompts(B, [8, 3, 5, 1], seed=11)                      # stride 8, an index
        eng.set_prompts(wide, list(range(B)))
        graph_equals_direct_and_rows_begin_with(wide)
        narrow = _random_prompts(B, [4, 2, 1, 3], seed=12)                    # stride 4: fits the same arrays
        eng.set_prompts(narrow, list(range(B)))
        assert eng.status(_lib.STATUS_PROMPTS) == B
        graph_equals_direct_and_rows_begin_with(narrow)
        one = _random_prompts(1, [4], seed=13)                                # the same stride, no index
        eng.set_prompts(one)
        assert eng.status(_lib.STATUS_PROMPTS) == 1
        graph_equals_direct_and_rows_begin_with(one * B)
    finally:
        eng.set_prompts(None)
    assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0


def test_masks_and_prompts_together():
    eng, lm = _engine("float32", B), _lm(B)
    eng.encode(lm)
    plain = eng.decode(num_steps=S).cpu().numpy()
    forbid = []
    for row in plain:
        for t in row[:_eos_at(row)]:
            if t > 1 and int(t) not in forbid:
                forbid.append(int(t))
    forbid = forbid[:6]
    assert forbid
    mask = np.full(V // 32, 0xFFFFFFFF, np.uint32)
    for i in forbid:
        mask[i >> 5] &= np.uint32(~(1 << (i & 31)) & 0xFFFFFFFF)
    prompts = [[forbid[0]] * p or None for p in (0, 1, 7, 20, 20, 7, 1, 0)]      # the prompt IS a forbidden token
    eng.set_token_masks(mask)
    _set(eng, prompts)
    try:
        for beam1 in (False, True):
            ids = eng.decode(num_steps=S, beam1=beam1).cpu().numpy()
            for b in range(B):
                p = len(prompts[b] or [])
                assert list(ids[b, :p]) == (prompts[b] or [])
                assert not np.isin(ids[b, p:S], forbid).any(), (beam1, b)
    finally:
        eng.set_prompts(None)
        eng.clear_token_masks()


def _fields(ns):
    return [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum) for n in ns.notes]


def test_inference_model_prompts_on_the_trained_fixture():
    assert os.path.exists(CKPT)
    audio = synthetic.synth_music(3 * 2.048 - 0.3, seed=13, device="cpu")[1]
    m = inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32", decoding="greedy")
    plain = m(audio)
    _, x = m._examples(audio, 16000)
    ids = m._predict_ids({"encoder_input_tokens": x}).cpu().numpy()
    lead = [int(t) for t in ids[0, :min(5, _eos_at(ids[0], ids.shape[1]))]]
    assert lead and min(lead) >= 2
    assert _fields(m(audio, prompts=[lead])) == _fields(plain)                # the first segment's own leading tokens
    assert m.model.status(_lib.STATUS_PROMPTS) == 0                           # cleared after the call
    tie = vocabularies.tie_section_prompt(m.codec, [])
    seen = {}
    keep = m._predict_ids
    m._predict_ids = lambda batch, *a, **kw: seen.setdefault("ids", keep(batch, *a, **kw))
    try:
        m(audio, prompts=[tie, None, tie], programs=[0])                      # composes with programs=
    finally:
        m._predict_ids = keep
    rows = seen["ids"].cpu().numpy()
    assert rows[0, 0] == tie[0] and rows[2, 0] == tie[0]
    assert m.model.status(_lib.STATUS_PROMPTS) == 0 and m.model.status(_lib.STATUS_TOKEN_MASKS) == 0
    assert _fields(m(audio)) == _fields(plain)
    both = m.transcribe_many([audio, audio], prompts=[[lead], None])
    assert _fields(both[0]) == _fields(plain) and _fields(both[1]) == _fields(plain)
    with pytest.raises(ValueError, match="prompts has 9 entries"):
        m(audio, prompts=[tie] * 9)
