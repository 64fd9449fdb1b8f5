"""Per-segment sampling seeds (mt3_engine_set_sampling_seeds) and the draws job (mt3_engine_transcribe_draws,
Transformer.transcribe(draws=per)) through the engine: the tiny random-weight engines of tests/test_gpu_sampling_engine.py
(one encoder layer, two decoder layers, input_length 256, L = 64, 16 steps, boost_note_events).  A draw depends on its
segment's logits, stream and seed only, so every comparison is equality of ids: a seeded job against single calls under
that seed as the engine's seed, and the draws job against mt3_engine_transcribe on the inputs with every segment `per`
times in a row under the same tables.  Then InferenceModel.sample / sample_many / consensus on the trained fixture, which
run their samples as one such job, against models with seeds seed .. seed + n - 1."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, checkpoints, consensus, inference, network, spectrograms, synthetic  # noqa: E402
from mt3_amd.sampling import SamplingParams as P  # noqa: E402
from tests import consensus_ref  # noqa: E402

L, S, V = 64, 16, 1536
CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
STREAMS = np.array([(1 << 40) + 7 * i * i + 3 for i in range(11)], np.uint64)      # not the segment index, past 2^32
SEEDS = np.array([(1 << 33) + 1000003 * i * i + 17 * i for i in range(9)] + [(1 << 64) - 1, 1 << 32], np.uint64)
MODES = [P(temperature=0.9, seed=11), P(temperature=1.1, top_p=0.9, seed=12)]


def _engine(dtype, B, seed=5):
    cfg = network.T5Config(dtype=dtype, num_encoder_layers=1, num_decoder_layers=2)
    params = synthetic.boost_note_events(network.init_random_params(cfg, seed=seed, norm_scale_jitter=0.1))
    eng = network.Transformer(cfg, input_length=256, max_decode_length=L, max_batch=B)
    eng.load_params(params)
    return eng


def _lm(n, seed=21):
    return spectrograms.compute_spectrogram_batch(synthetic.synth_audio(n, seed=seed), None)


def _masks(index):
    """two masks over the vocabulary (the second forbids every third id from 5 on) and a per-draw index"""
    m = np.full((2, V // 32), 0xFFFFFFFF, np.uint32)
    for i in range(5, V, 3):
        m[1, i >> 5] &= np.uint32(~(1 << (i & 31)) & 0xFFFFFFFF)
    return m, np.asarray(index, np.int32)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_seeded_job_against_single_calls(dtype):
    """11 segments through 8 slots under 11 different seeds: every segment gets the ids of encode + decode(EARLY_EXIT) of
    that segment alone with its stream and ITS SEED AS THE ENGINE'S SEED and no table -- the seed follows the segment
    through refills and compaction; with and without the step graph.  f32: alone in a batch of one; bf16: in a batch of 8
    copies of itself (mt3_engine_encode: 8 or more segments)."""
    assert hasattr(_lib.load(), "mt3_engine_set_sampling_seeds")
    eng, lm = _engine(dtype, 8), _lm(11)
    n = 1 if dtype == "float32" else 8
    try:
        for p in MODES:
            eng.set_sampling(p, STREAMS, SEEDS)
            job = eng.transcribe(lm, num_steps=S).clone()
            assert eng.transcribe_stats["slots"] == 8 and eng.transcribe_stats["refills"] == 3
            assert eng.transcribe_stats["used_graph"] == 1
            assert torch.equal(eng.transcribe(lm, num_steps=S, use_graph=False), job)
            # the same table through mt3_engine_decode (rows 0 .. 7), graph and direct launches
            eng.encode(lm[:8])
            rows = eng.decode(num_steps=S, early_exit=True).clone()
            assert torch.equal(rows, job[:8])
            assert torch.equal(eng.decode(num_steps=S, early_exit=True, use_graph=False), rows)
            for i in range(11):
                eng.set_sampling(P(p.temperature, p.top_k, p.top_p, int(SEEDS[i])), STREAMS[i:i + 1].repeat(n))
                eng.encode(lm[i:i + 1].repeat(n, 1, 1))
                assert torch.equal(eng.decode(num_steps=S, early_exit=True)[0], job[i]), (p, i)
            # clear-by-NULL: the job under the parameters' seed alone, which is also a table of that seed everywhere
            eng.set_sampling(p, STREAMS, SEEDS)
            _lib.check(eng._lib.mt3_engine_set_sampling_seeds(eng._h, None, 0))
            plain = eng.transcribe(lm, num_steps=S).clone()
            assert not torch.equal(plain, job)
            eng.set_sampling(p, STREAMS, np.full(11, p.seed, np.uint64))
            assert torch.equal(eng.transcribe(lm, num_steps=S), plain)
            eng.set_sampling(p, STREAMS)
            assert torch.equal(eng.transcribe(lm, num_steps=S), plain)
        assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0
        # a table shorter than the job
        eng.set_sampling(MODES[0], STREAMS, SEEDS[:4])
        eng.encode(lm[:8])
        with pytest.raises(_lib.Mt3Error, match="sampling seeds' n_segments"):
            eng.decode(num_steps=S)
        with pytest.raises(_lib.Mt3Error, match="sampling seeds' n_segments"):
            eng.transcribe(lm, num_steps=S)
        with pytest.raises(_lib.Mt3Error, match="sampling seeds' n_segments"):
            eng.transcribe(lm[:2], num_steps=S, draws=3)
        # a set while a decode is in flight is refused; the decode is what it would have been
        eng.set_sampling(MODES[0], STREAMS[:8], SEEDS[:8])
        want = eng.decode(num_steps=S).clone()
        eng.decode(num_steps=S, wait=False)
        sd = np.ascontiguousarray(SEEDS)
        for args in ((sd.ctypes.data, 8), (None, 0)):
            assert eng._lib.mt3_engine_set_sampling_seeds(eng._h, *args) == _lib.MT3_ERR_INVALID
            assert b"mt3_engine_set_sampling_seeds: a decode is in flight" in eng._lib.mt3_last_error()
        assert torch.equal(eng.decode_wait(), want)
        # clearing sampling clears the seeds; a table needs sampling set
        eng.clear_sampling()
        assert eng._lib.mt3_engine_set_sampling_seeds(eng._h, sd.ctypes.data, 11) == _lib.MT3_ERR_INVALID
        assert b"sampling is not set" in eng._lib.mt3_last_error()
        eng.set_sampling(MODES[1], STREAMS)
        assert torch.equal(eng.transcribe(lm, num_steps=S), plain)
    finally:
        eng.clear_sampling()


def test_first_seed_table_does_not_replay_graphs_captured_without_one():
    """The two C setters driven directly, as a C caller would: sampling alone, a job on the step graph (captured without a
    seed table), then the engine's FIRST seed table and the same job again -- it must not be served by the graph captured
    before: equal to direct launches, other ids than without seeds; and the reverse when the table is cleared."""
    eng, lm = _engine("float32", 8), _lm(11)
    lib, h = eng._lib, eng._h
    st = MODES[0].struct()
    streams, seeds = np.ascontiguousarray(STREAMS), np.ascontiguousarray(SEEDS)
    try:
        _lib.check(lib.mt3_engine_set_sampling(h, C.byref(st), streams.ctypes.data, 11))
        unseeded = eng.transcribe(lm, num_steps=S).clone()
        assert eng.transcribe_stats["used_graph"] == 1
        eng.encode(lm[:8])
        unseeded_rows = eng.decode(num_steps=S, early_exit=True).clone()
        _lib.check(lib.mt3_engine_set_sampling_seeds(h, seeds.ctypes.data, 11))
        seeded = eng.transcribe(lm, num_steps=S).clone()
        assert eng.transcribe_stats["used_graph"] == 1
        assert torch.equal(seeded, eng.transcribe(lm, num_steps=S, use_graph=False))
        assert not torch.equal(seeded, unseeded)
        eng.encode(lm[:8])
        rows = eng.decode(num_steps=S, early_exit=True).clone()
        assert torch.equal(rows, seeded[:8]) and not torch.equal(rows, unseeded_rows)
        draws = eng.transcribe(lm[:5], num_steps=S, draws=2).cpu().numpy().reshape(5, 2, L)
        assert all(not np.array_equal(d[0], d[1]) for d in draws)
        # and the reverse: cleared, the graph captured with the table serves nothing
        _lib.check(lib.mt3_engine_set_sampling_seeds(h, None, 0))
        assert torch.equal(eng.transcribe(lm, num_steps=S), unseeded)
        assert eng.transcribe_stats["used_graph"] == 1
        assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0
    finally:
        eng.clear_sampling()


def test_draws_equal_the_replicated_job_f32():
    """5 segments x 3 draws in 8 slots: 15 draws, the first refill run starts in the middle of segment 2's draws.  Equal to
    transcribe(x.repeat_interleave(3, 0)) under the same stream, seed and mask tables; with and without the step graph;
    without sampling the three draws of a segment are equal; and the stats are the header's."""
    eng, lm = _engine("float32", 8), _lm(5)
    per, N = 3, 5
    wide = lm.repeat_interleave(per, 0)
    streams = np.repeat(STREAMS[:N], per)
    seeds = np.tile(SEEDS[[9, 10, 3]], N)
    try:
        for p in MODES:
            for masks in (None, _masks([0, 1, -1, 1, 0, 0, -1, -1, 1, 1, 0, 1, -1, 0, 1])):
                if masks is not None:
                    eng.set_token_masks(*masks)
                eng.set_sampling(p, streams, seeds)
                want = eng.transcribe(wide, num_steps=S).clone()
                got = eng.transcribe(lm, num_steps=S, draws=per).clone()
                st = dict(eng.transcribe_stats)
                assert got.shape == (N * per, L) and torch.equal(got, want), (p, masks is not None)
                assert st["slots"] == 8 and st["refills"] == N * per - 8 and st["encoder_chunks"] == 1, st
                assert st["used_graph"] == 1 and st["groups"] == 1
                assert torch.equal(eng.transcribe(lm, num_steps=S, draws=per, use_graph=False), want)
                assert eng.transcribe_stats["used_graph"] == 0
                assert torch.equal(eng.transcribe(lm, num_steps=S, draws=per, single_stream=True), want)
                rows = got.cpu().numpy().reshape(N, per, L)
                assert all(len({tuple(r) for r in seg}) > 1 for seg in rows)        # a segment's draws differ
                eng.clear_token_masks()
        # the same seed for every draw of a segment: equal draws, each the plain sampled job's row
        eng.set_sampling(MODES[0], streams)
        same = eng.transcribe(lm, num_steps=S, draws=per).cpu().numpy().reshape(N, per, L)
        eng.set_sampling(MODES[0], STREAMS[:N])
        one = eng.transcribe(lm, num_steps=S).cpu().numpy()
        assert all(np.array_equal(same[:, j], one) for j in range(per))
        # without sampling the draws of a segment are equal: legal, and the greedy job's rows
        eng.clear_sampling()
        greedy = eng.transcribe(lm, num_steps=S).clone()
        got = eng.transcribe(lm, num_steps=S, draws=per)
        assert torch.equal(got, greedy.repeat_interleave(per, 0))
        assert torch.equal(got, eng.transcribe(wide, num_steps=S))
        # per = 1 is the plain job; fewer draws than slots
        assert torch.equal(eng.transcribe(lm, num_steps=S, draws=1), greedy)
        assert eng.transcribe_stats["slots"] == 5 and eng.transcribe_stats["refills"] == 0
        # more segments than a staging chunk holds: 11 segments, chunks of 8
        lm11 = _lm(11)
        eng.set_sampling(MODES[1], np.repeat(STREAMS, 2), np.tile(SEEDS[:2], 11))
        want = eng.transcribe(lm11.repeat_interleave(2, 0), num_steps=S).clone()
        assert torch.equal(eng.transcribe(lm11, num_steps=S, draws=2), want)
        assert eng.transcribe_stats["encoder_chunks"] == 2 and eng.transcribe_stats["refills"] == 14
        # the flags and arguments the call refuses
        with pytest.raises(ValueError):
            eng.transcribe(lm, num_steps=S, draws=2, beam1=True)
        with pytest.raises(ValueError):
            eng.transcribe(lm, num_steps=S, draws=2, num_beams=2)
        with pytest.raises(ValueError):
            eng.transcribe(lm, num_steps=S, draws=0)
        assert eng.status(_lib.STATUS_GRAPH_FALLBACKS) == 0
    finally:
        eng.clear_sampling()
        eng.clear_token_masks()


def test_draws_equal_the_replicated_job_bf16():
    """11 segments x 2 draws in 8 slots, bf16: both sides' encoder passes are of 8 or more segments (the replicated job's
    first pass is its 8 slots, its staging passes and every pass of the draws job are padded to 8)"""
    eng, lm = _engine("bfloat16", 8), _lm(11)
    per = 2
    try:
        for p in MODES:
            eng.set_sampling(p, np.repeat(STREAMS, per), np.tile(SEEDS[[4, 10]], 11))
            want = eng.transcribe(lm.repeat_interleave(per, 0), num_steps=S).clone()
            got = eng.transcribe(lm, num_steps=S, draws=per)
            assert torch.equal(got, want), p
            assert eng.transcribe_stats["slots"] == 8 and eng.transcribe_stats["refills"] == 14
            assert eng.transcribe_stats["encoder_chunks"] == 2
            assert torch.equal(eng.transcribe(lm, num_steps=S, draws=per, use_graph=False), want)
    finally:
        eng.clear_sampling()


def test_draws_over_row_groups():
    """48 segments x 4 draws in 128 slots: two row groups, equal to the single stream and to the replicated job"""
    eng, lm = _engine("float32", 128), _lm(48)
    per = 4
    streams = np.repeat((np.arange(48, dtype=np.uint64) * np.uint64(2654435761)) ^ np.uint64(1 << 50), per)
    seeds = np.tile(SEEDS[[0, 9, 10, 5]], 48)
    try:
        eng.set_sampling(MODES[1], streams, seeds)
        two = eng.transcribe(lm, num_steps=S, draws=per).clone()
        st = dict(eng.transcribe_stats)
        assert st["groups"] == 2 and st["slots"] == 128 and st["refills"] == 64 and st["encoder_chunks"] == 1, st
        one = eng.transcribe(lm, num_steps=S, draws=per, single_stream=True)
        assert eng.transcribe_stats["groups"] == 1
        assert torch.equal(one, two)
        assert torch.equal(eng.transcribe(lm.repeat_interleave(per, 0), num_steps=S), two)
    finally:
        eng.clear_sampling()


def test_inference_model_samples_in_one_job():
    a = synthetic.synth_music(3 * 2.048 - 0.3, seed=13, device="cpu")[1]
    b = synthetic.synth_music(2 * 2.048 - 0.5, seed=14, device="cpu")[1]
    kw = dict(dtype="float32", decoding="sample", temperature=0.8, top_p=0.95)
    params = checkpoints.load_compact_npz(CKPT)
    notes = lambda ns: [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum) for n in ns.notes]  # noqa: E731
    want_a, want_b = [], []
    for j in range(3):                                       # three models with seeds seed .. seed + 2, called on the audio
        m = inference.InferenceModel(params, "mt3", seed=5 + j, **kw)
        want_a.append(notes(m(a)))
        want_b.append(notes(m(b)))
        m = None
    m = inference.InferenceModel(params, "mt3", seed=5, **kw)
    draws = m.sample(a, 3)
    assert [notes(d) for d in draws] == want_a and len(want_a[0]) > 0
    assert m.rows_per_engine_call == [3 * 3]                 # ONE engine job of segments x samples draws
    assert m.model.transcribe_stats["encoder_chunks"] == 1
    assert m.model.status(_lib.STATUS_SAMPLING) == 0 and m.decoding == "sample" and m.sampling.seed == 5
    assert len({tuple(x) for x in want_a}) > 1               # and the samples differ
    many = m.sample_many([b, a], 3)
    assert [[notes(d) for d in f] for f in many] == [want_b, want_a]
    assert m.rows_per_engine_call == [(2 + 3) * 3]
    assert [[notes(d) for d in f] for f in many] == [[notes(d) for d in m.sample(b, 3)], [notes(d) for d in draws]]
    # programs / prompts ride along as in __call__
    only = m.sample(a, 2, programs=[0])
    assert all(n.program == 0 for d in only for n in d.notes)
    # the vote on top
    ns, record, samples = m.consensus(a, 3, return_votes=True)
    assert [notes(s) for s in samples] == want_a
    consensus_ref.assert_same([record], consensus.consensus([draws]))
    assert ns == record.notes
    voted = m.consensus_many([b, a], 3, return_votes=True)
    consensus_ref.assert_same([voted[1][1]], [record])
    assert voted[1][0] == ns and [notes(s) for s in voted[0][2]] == want_b
    assert m.consensus_many([b, a], 3) == [voted[0][0], ns]
    # a model of another decoding samples too, and is left as it was
    m.decoding = "greedy"
    assert [notes(d) for d in m.sample(a, 3)] == want_a and m.decoding == "greedy"
    # well_formed="tied" keeps its loop of decodes, and still runs
    tied = m.sample(a, 2, well_formed="tied")
    assert len(tied) == 2 and m.rows_per_engine_call != [3 * 2]
    with pytest.raises(ValueError):
        m.sample(a, 0)
