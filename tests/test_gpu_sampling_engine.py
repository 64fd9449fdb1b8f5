"""Temperature sampling through the engine (mt3_engine_set_sampling): the tiny random-weight engines of
tests/test_gpu_token_mask_engine.py (one encoder layer, two decoder layers, L = 64, 16 steps), f32 and bf16, with the
note-event logit boost of synthetic.boost_note_events so that the draws are over a peaked distribution.  A segment's
sample depends on (seed, stream) and its logits only: graph replay, row groups, the early exit and in-flight refills give
the same ids; top_k = 1 is today's greedy; clearing leaves the unsampled decode as it was; and the ids are linked back to
the rule through decode_forced's per-step logits and `sampling.pick`."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, inference, network, sampling, spectrograms, synthetic  # noqa: E402
from mt3_amd.sampling import SamplingParams as P  # noqa: E402

L, S, V = 64, 16, 1536
CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
DTYPES = ["float32", "bfloat16"]
STREAMS = np.array([(1 << 40) + 7 * i * i + 3 for i in range(11)], np.uint64)      # not the segment index, past 2^32
MODES = [P(temperature=0.9, seed=11), P(temperature=1.1, top_p=0.9, seed=12), P(temperature=0.8, top_k=40, seed=13)]
# the link to the rule needs the restatement's own cuts clear of f32 rounding on the MODEL's logits, which are flat (random
# weights, 1536 ids of about 6e-4 of mass each at T = 1): a low temperature puts the top-p cut and the top-k boundary among
# the few ids that then hold the mass (masses of percents, gaps of tenths)
LINK_MODES = [MODES[0], P(temperature=0.25, top_p=0.5, seed=12), P(temperature=0.25, top_k=5, seed=13)]
STATUS = range(16)


def _engine(dtype, B, seed=5):
    cfg = network.T5Config(dtype=dtype, num_encoder_layers=1, num_decoder_layers=2)
    params = synthetic.boost_note_events(network.init_random_params(cfg, seed=seed, norm_scale_jitter=0.1))
    eng = network.Transformer(cfg, input_length=256, max_decode_length=L, max_batch=B)
    eng.load_params(params)
    return eng


def _lm(n, seed=21):
    return spectrograms.compute_spectrogram_batch(synthetic.synth_audio(n, seed=seed), None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_schedules_seeds_and_clearing(dtype):
    eng, lm = _engine(dtype, 8), _lm(11)
    eng.encode(lm[:8])
    plain = eng.decode(num_steps=S).clone()
    status = [eng.status(i) for i in STATUS]
    assert status[_lib.STATUS_SAMPLING] == 0
    try:
        for p in MODES:
            eng.set_sampling(p, STREAMS[:8])
            assert eng.status(_lib.STATUS_SAMPLING) == 1
            eng.encode(lm[:8])
            replay = eng.decode(num_steps=S).clone()
            assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 1
            direct = eng.decode(num_steps=S, use_graph=False).clone()
            assert eng.status(_lib.STATUS_LAST_DECODE_USED_GRAPH) == 0
            assert torch.equal(replay, direct), p                          # graph replay equals direct launches
            assert torch.equal(eng.decode(num_steps=S), replay)             # the same seed twice
            eng.decode(num_steps=S, wait=False)
            assert torch.equal(eng.decode_wait(), replay)                   # MT3_DECODE_ASYNC
            early = eng.decode(num_steps=S, early_exit=True).cpu().numpy()
            full = replay.cpu().numpy()
            for b in range(8):
                n = int(np.argmax(full[b] == 1)) + 1 if (full[b] == 1).any() else S
                assert np.array_equal(full[b, :n], early[b, :n]) and not early[b, n:].any(), (p, b)
            assert not torch.equal(replay, plain)                           # it samples
            # a second seed gives other ids; another stream as well
            eng.set_sampling(P(p.temperature, p.top_k, p.top_p, p.seed + 1), STREAMS[:8])
            assert not torch.equal(eng.decode(num_steps=S), replay)
            eng.set_sampling(p, STREAMS[1:9])
            assert not torch.equal(eng.decode(num_steps=S), replay)
            # NULL streams: row i draws from stream i
            eng.set_sampling(p)
            by_default = eng.decode(num_steps=S).clone()
            eng.set_sampling(p, np.arange(8))
            assert torch.equal(eng.decode(num_steps=S), by_default)
            # beam-1 does not sample; the beam search ignores sampling
            with pytest.raises(_lib.Mt3Error, match="BEAM1"):
                eng.decode(num_steps=S, beam1=True)
        # top_k = 1 is today's greedy, whatever seed and temperature
        eng.set_sampling(P(temperature=0.3, top_k=1, seed=99), STREAMS)
        assert torch.equal(eng.decode(num_steps=S), plain)
        job_k1 = eng.transcribe(lm, num_steps=S).clone()
        eng.clear_sampling()
        assert torch.equal(eng.transcribe(lm, num_steps=S), job_k1)
        eng.encode(lm[:8])
        # more rows than streams
        eng.set_sampling(MODES[0], STREAMS[:4])
        with pytest.raises(_lib.Mt3Error, match="n_segments"):
            eng.decode(num_steps=S)
        with pytest.raises(_lib.Mt3Error, match="n_segments"):
            eng.transcribe(lm, num_steps=S)
        # a set while a decode is in flight is refused
        eng.set_sampling(MODES[0], STREAMS[:8])
        want = eng.decode(num_steps=S).clone()
        eng.decode(num_steps=S, wait=False)
        with pytest.raises(_lib.Mt3Error, match="mt3_engine_set_sampling: a decode is in flight"):
            eng.clear_sampling()
        assert torch.equal(eng.decode_wait(), want)
    finally:
        eng.clear_sampling()
    # cleared: the ids and every status item of the unsampled decode are what they were before the set
    eng.encode(lm[:8])
    assert torch.equal(eng.decode(num_steps=S), plain)
    assert [eng.status(i) for i in STATUS] == status


@pytest.mark.parametrize("dtype", DTYPES)
def test_job_against_single_calls(dtype):
    """11 segments through 8 slots: every segment gets the ids of encode + decode(EARLY_EXIT) of that segment alone with
    its stream -- the stream follows the segment through refills and compaction; with and without the step graph.  f32:
    the segment alone in a batch of one.  bf16: alone in a batch of 8 copies of itself, the documented condition under
    which a bf16 encoder pass gives a segment the bits it has in the job's passes (mt3_engine_encode: 8 or more segments)"""
    eng, lm = _engine(dtype, 8), _lm(11)
    n = 1 if dtype == "float32" else 8
    try:
        for p in MODES[:2]:
            eng.set_sampling(p, STREAMS)
            job = eng.transcribe(lm, num_steps=S).clone()
            assert eng.transcribe_stats["slots"] == 8 and eng.transcribe_stats["refills"] == 3
            assert eng.transcribe_stats["used_graph"] == 1
            assert torch.equal(eng.transcribe(lm, num_steps=S, use_graph=False), job)
            for i in range(11):
                eng.set_sampling(p, STREAMS[i:i + 1].repeat(n))
                eng.encode(lm[i:i + 1].repeat(n, 1, 1))
                assert torch.equal(eng.decode(num_steps=S, early_exit=True)[0], job[i]), (p, i)
        assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0
    finally:
        eng.clear_sampling()


def test_row_groups_equal_a_single_stream():
    eng, lm = _engine("float32", 128), _lm(128)
    eng.encode(lm)
    streams = (np.arange(128, dtype=np.uint64) * np.uint64(2654435761)) ^ np.uint64(1 << 50)
    try:
        eng.set_sampling(MODES[1], streams)
        one = eng.decode(num_steps=8, single_stream=True).clone()
        two = eng.decode(num_steps=8)
        assert eng.status(_lib.STATUS_LAST_DECODE_GROUPS) == 2
        assert torch.equal(one, two)
        eng.set_sampling(MODES[1])                                          # NULL streams: the row index, across groups
        one = eng.decode(num_steps=8, single_stream=True).clone()
        assert torch.equal(one, eng.decode(num_steps=8))
        assert len({tuple(r) for r in one.cpu().numpy()[:, :8].tolist()}) > 100      # the rows draw differently
    finally:
        eng.clear_sampling()


@pytest.mark.parametrize("dtype", DTYPES)
def test_link_to_the_rule(dtype):
    """decode_forced on the sampled ids gives the model's own per-step logits (it ignores sampling); sampling.pick on them
    reproduces the id at every position whose margins are at least 1e-3 (top-p masses: 1e-4); at most 2 % of the
    positions may fall below the margins (LINK_MODES keeps the restatement inside that share)"""
    eng, lm = _engine(dtype, 8), _lm(8)
    eng.encode(lm)
    try:
        for p in LINK_MODES:
            eng.set_sampling(p, STREAMS[:8])
            ids = eng.decode(num_steps=S)
            _, logits = eng.decode_forced(ids, num_steps=S)
            lg, got = logits.cpu().numpy(), ids.cpu().numpy()
            assert np.isfinite(lg).all()
            checked = below = 0
            for b in range(8):
                for t in range(S):
                    want, m = sampling.pick(lg[t, b], t, int(STREAMS[b]), p)
                    if m["pick"] >= 1e-3 and m["boundary"] >= 1e-3 and m["mass"] >= 1e-4:
                        checked += 1
                        assert got[b, t] == want, (p, b, t, m)
                    else:
                        below += 1
                    if got[b, t] == 1:
                        assert not got[b, t + 1:].any()
                        break
            print("LINK %s %s: %d positions checked, %d below the margins" % (dtype, p, checked, below))
            assert checked + below >= 24 and below <= 0.02 * (checked + below)
    finally:
        eng.clear_sampling()


def test_inference_model_samples_a_file_the_same_alone_and_in_a_job():
    a = synthetic.synth_music(3 * 2.048 - 0.3, seed=13, device="cpu")[1]
    b = synthetic.synth_music(2 * 2.048 - 0.5, seed=14, device="cpu")[1]
    m = inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32", decoding="sample",
                                 temperature=0.8, top_p=0.95, seed=5)
    notes = lambda ns: [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum) for n in ns.notes]  # noqa: E731
    alone_a, alone_b = notes(m(a)), notes(m(b))
    assert m.model.status(_lib.STATUS_SAMPLING) == 0                        # cleared after the call
    many = m.transcribe_many([b, a, b])
    assert [notes(ns) for ns in many] == [alone_b, alone_a, alone_b]
    assert len(alone_a) > 0
    draws = m.sample(a, num_samples=3)
    assert notes(draws[0]) == alone_a and len(draws) == 3
    assert any(notes(d) != alone_a for d in draws[1:])
