"""Graph chains (MT3_DECODE_CHAINS(n), mt3_engine_config::decode_chains) on the engine's one decode loop.

A chains decode is a GroupJob like every other: one group on the caller's stream whose step graph has `chains` parallel
branches (csrc/engine.hip: group_graph), or, launched directly, the chains back to back.  Rows are independent, so
whatever a chains decode returns -- ids, steps_run, first-step and per-step logits -- must be BIT-IDENTICAL to the same
engine's chains=1 decode of the same encode: with the early exit, with logits, asynchronous, from the engine's
configuration, across changes of batch and token rules (the step-graph cache is keyed by the chain count, not dropped),
and with rows that do not divide by the chains.  No case may fall back from a graph it asked for.

Shapes: one encoder and one decoder layer, 64 decode positions, 48 slots -- a chain needs 16 rows (chains_for), so 48
rows make 3 chains, 32 rows 2, and 40 rows over 3 chains deal 14 + 13 + 13.  The input length is 256 frames, the
shortest the engine takes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, network  # noqa: E402

T, L, B = 256, 64, 48


def _build(dtype, **kw):
    cfg = network.T5Config(dtype=dtype, num_encoder_layers=1, num_decoder_layers=1)
    eng = network.Transformer(cfg, input_length=T, max_decode_length=L, max_batch=B, **kw)
    eng.load_params(network.init_random_params(cfg, seed=3, norm_scale_jitter=0.1))
    return eng


@pytest.fixture(scope="module")
def inputs():
    x = np.random.default_rng(7).standard_normal((B, T, 512)).astype(np.float32)
    return torch.from_numpy(x).cuda()


@pytest.fixture(scope="module", params=["float32", "bfloat16"])
def eng(request):
    return _build(request.param)


class _Watch:
    """Every decode inside asks for a graph where `graph` says so and must get it; no fallback is counted."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.before = self.eng.status(_lib.STATUS_GRAPH_FALLBACKS)
        return self

    def used(self, graph=True):
        assert self.eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == (1 if graph else 0)
        assert self.eng.status(_lib.STATUS_GRAPH_FALLBACKS) == self.before

    def __exit__(self, *exc):
        if exc[0] is None:
            assert self.eng.status(_lib.STATUS_GRAPH_FALLBACKS) == self.before
        return False


def _np(t):
    return t.cpu().numpy()


def test_early_exit_under_chains(eng, inputs):
    eng.encode(inputs)
    rng = np.random.default_rng(1)
    short = rng.integers(1, 21, B).astype(np.int32)              # every row has finished by step 20
    late = short.copy()
    late[29] = 40                                                # one row of the middle chain outlives the first poll
    try:
        for lens, steps in ((short, 32), (late, 64)):
            eng.debug_set_eos_schedule(lens)
            ref = _np(eng.decode(num_steps=L, early_exit=True, chains=1, single_stream=True))
            assert eng.steps_run == steps
            assert (ref == 1).any(1).all() and int(((ref == 1).argmax(1) + 1).max()) <= int(lens.max())
            with _Watch(eng) as w:
                got = _np(eng.decode(num_steps=L, early_exit=True, chains=3))
                w.used()
            assert eng.steps_run == steps, (eng.steps_run, steps)
            assert np.array_equal(got, ref), np.nonzero((got != ref).any(1))[0]
            assert eng.status(_lib.STATUS_LAST_DECODE_COMPACTIONS) == 0
            assert eng.status(_lib.STATUS_LAST_DECODE_GROUPS) == 1
    finally:
        eng.debug_set_eos_schedule(None)


@pytest.mark.parametrize("graph", [True, False])
def test_logits_under_chains(eng, inputs, graph):
    eng.encode(inputs[:32])
    ids1, first1 = eng.decode(num_steps=8, chains=1, return_first_logits=True)
    dbg1 = _np(eng.debug_decode(num_steps=8, chains=1))
    forced = _np(ids1)[:, :8]
    f_ids1, step1 = eng.decode_forced(forced, num_steps=8, chains=1)
    assert np.array_equal(dbg1, _np(ids1)) and len(np.unique(dbg1[:, :8], axis=0)) > 1
    with _Watch(eng) as w:
        ids2, first2 = eng.decode(num_steps=8, chains=2, return_first_logits=True, use_graph=graph)
        w.used(graph)
        dbg2 = _np(eng.debug_decode(num_steps=8, chains=2, use_graph=graph))
        w.used(graph)
        f_ids2, step2 = eng.decode_forced(forced, num_steps=8, chains=2, use_graph=graph)
        w.used(graph)
    assert np.array_equal(_np(ids2), _np(ids1)) and np.array_equal(dbg2, dbg1)
    assert np.array_equal(_np(first2), _np(first1))              # first-step logits, bit for bit
    assert np.array_equal(_np(f_ids2), _np(f_ids1))
    assert step2.shape == (8, 32, eng.config.vocab_size)
    assert np.array_equal(_np(step2), _np(step1))                # per-step logits, bit for bit


def test_async_chains_decode(eng, inputs):
    eng.encode(inputs[:32])
    ref = _np(eng.decode(num_steps=24, chains=1))
    sync = _np(eng.decode(num_steps=24, chains=2))
    sync_steps = eng.steps_run
    with _Watch(eng) as w:
        assert eng.decode(num_steps=24, chains=2, wait=False) is None
        with pytest.raises(_lib.Mt3Error):
            eng.decode(num_steps=8)                              # a decode is in flight
        with pytest.raises(_lib.Mt3Error):
            eng.encode(inputs[:32])
        got = eng.decode_wait()
        torch.cuda.synchronize()
        w.used()
    assert eng.steps_run == sync_steps == 24
    assert np.array_equal(_np(got), sync) and np.array_equal(sync, ref)
    assert eng.status(_lib.STATUS_LAST_DECODE_GROUPS) == 1


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_configured_chains(dtype, inputs):
    eng = _build(dtype, decode_chains=2)
    eng.encode(inputs[:32])
    ref = _np(eng.decode(num_steps=24, chains=1))
    with _Watch(eng) as w:
        got = _np(eng.decode(num_steps=24, chains=0))
        w.used()
    assert eng.status(_lib.STATUS_LAST_DECODE_GROUPS) == 1
    assert np.array_equal(got, ref)


def test_chain_graphs_are_keyed_not_dropped(eng, inputs):
    ones = np.full((eng.config.vocab_size + 31) // 32, 0xFFFFFFFF, np.uint32)
    try:
        with _Watch(eng) as w:
            for rows, chains, masked in ((48, 3, False), (32, 2, False), (48, 3, False), (48, 3, True)):
                if masked:
                    eng.set_token_masks(ones)                    # a setup call: the step graphs are dropped and come back
                eng.encode(inputs[:rows])
                ref = _np(eng.decode(num_steps=16, chains=1))
                w.used()
                got = _np(eng.decode(num_steps=16, chains=chains))
                w.used()
                assert np.array_equal(got, ref), (rows, chains, masked)
                if not masked:
                    free = ref
            assert np.array_equal(ref, free)                     # a mask that allows every token changes nothing
    finally:
        eng.clear_token_masks()


def test_beam1_under_a_ragged_deal(eng, inputs):
    eng.encode(inputs[:40])
    ref = _np(eng.decode(num_steps=16, chains=1, beam1=True))
    with _Watch(eng) as w:
        got = _np(eng.decode(num_steps=16, chains=3, beam1=True))
        w.used()
    assert np.array_equal(got, ref)
    assert len(np.unique(ref[:, :16], axis=0)) > 1
