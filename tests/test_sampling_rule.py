"""Temperature sampling without a GPU (mt3_engine_set_sampling; the rule: include/mt3_hip.h): the header's noise as the
library exports it against the numpy restatement mt3_amd/sampling.py, the restatement's kept sets on hand-written rows,
its distribution on one fixed row, and the argument checks of the setter and the scripted driver that come back before
any device work (on a box without a device anything later would be MT3_ERR_HIP)."""
import ctypes as C

import numpy as np
import pytest

from mt3_amd import _lib, sampling
from mt3_amd.sampling import SamplingParams as P

INF = np.inf


def test_status_item_struct_and_signatures():
    assert _lib.STATUS_SAMPLING == 15
    lib = _lib.load()
    for name in ("mt3_engine_set_sampling", "mt3_sampling_bits", "mt3_sampling_gumbel", "mt3_op_token_steps_sampled"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(_lib.Sampling) == 24 and _lib.Sampling.seed.offset == 16
    assert len(_lib.SIGNATURES["mt3_op_token_steps_sampled"][1]) == len(_lib.SIGNATURES["mt3_op_token_steps_grammar"][1]) + 2


def test_noise_bits_agree_with_the_restatement():
    """mt3_sampling_bits == sampling.philox_bits on 10,000 tuples: random 64-bit seeds and streams, values at and above
    2^32, words with the sign bit set, and the all-zero vector, whose word 0 is 0x6627e8d5"""
    lib = _lib.load()
    assert lib.mt3_sampling_bits(0, 0, 0, 0) == 0x6627E8D5
    assert int(sampling.philox_bits(0, 0, 0, 0)) == 0x6627E8D5
    rng = np.random.default_rng(7)
    n = 10000
    seed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    stream = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    t = rng.integers(0, 1024, n).astype(np.int32)
    tok = rng.integers(0, 2048, n).astype(np.int32)
    edge = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1, 0x80000000, 0xFFFFFFFF00000000]
    for i, v in enumerate(edge):                           # at and above 2^32, in the seed and in the stream
        seed[i], stream[i] = v, edge[-1 - i]
        seed[100 + i], stream[200 + i] = v, v
    t[:8] = [0, -1, -(1 << 31), (1 << 31) - 1, 1, 1023, -7, 64]          # negative-looking words
    tok[:8] = [0, -1, (1 << 31) - 1, -(1 << 31), 2047, 1, -2048, 256]
    seed[300], stream[300], t[300], tok[300] = 0, 0, 0, 0
    want = sampling.philox_bits(seed, stream, t, tok)
    got = np.array([lib.mt3_sampling_bits(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(seed, stream, t, tok)],
                   dtype=np.uint32)
    assert np.array_equal(got, want)
    assert want[300] == 0x6627E8D5
    assert len(np.unique(want)) > 9900                     # and it is noise, not a constant
    # python ints of any size and sign reduce as the C arguments do
    assert int(sampling.philox_bits(-1, (1 << 64) + 5, -1, 3)) == lib.mt3_sampling_bits((1 << 64) - 1, 5, -1, 3)


def test_gumbel_agrees_with_the_float64_formula():
    """mt3_sampling_gumbel (f32: two accurate logf) against -log(-log(u)) in float64 to 4 ulp.  The ulp is that of the
    larger of |g| and 1: a = -logf(u) carries a relative error of an ulp, which logf(a) turns into an ABSOLUTE error of
    about 2^-24 whatever g is, so near g = 0 (u near 1/e) no f32 evaluation can be held to ulps of g itself."""
    lib = _lib.load()
    rng = np.random.default_rng(11)
    bits = np.concatenate([rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32),
                           np.array([0, 511, 512, 0xFFFFFFFF, 0xFFFFFE00, 0x80000000, 0x5E2D58D8], np.uint32)])
    u = sampling.uniform(bits)
    assert (u > 0).all() and (u < 1).all()
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))           # exact in f32 (23 bits and the half)
    assert np.isfinite(sampling.gumbel(np.array([0, 0xFFFFFFFF], np.uint32))).all()
    want = sampling.gumbel(bits)
    got = np.array([lib.mt3_sampling_gumbel(int(b)) for b in bits], dtype=np.float32).astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(want), 1.0).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    print("GUMBEL max err %.3f ulp, range [%.3f, %.3f]" % (err.max(), want.min(), want.max()))
    assert err.max() <= 4.0


def test_top_k_of_one_is_the_first_arg_max():
    rng = np.random.default_rng(3)
    for trial in range(200):
        x = rng.normal(0, 3, 40).astype(np.float32)
        if trial % 3 == 0:
            x[rng.integers(0, 40, 3)] = x.max()            # ties: the lowest id wins
        if trial % 5 == 0:
            x[rng.integers(0, 40, 6)] = -INF
        p = P(temperature=float(rng.uniform(0.2, 3.0)), top_k=1, seed=int(rng.integers(0, 1 << 62)))
        tok, m = sampling.pick(x, trial, trial * 7, p)
        assert tok == int(np.argmax(x)) and list(m["kept"]) == [tok] and m["pick"] == INF


def test_kept_sets_on_hand_written_rows():
    """the top-k and top-p prefixes, ties and -inf entries included"""
    x = np.array([1.0, 3.0, -INF, 3.0, 2.0, 0.5, -INF, 2.0], np.float32)
    kept = lambda **kw: list(sampling.pick(x, 0, 0, P(**kw))[1]["kept"])      # noqa: E731
    assert kept() == [1, 3, 4, 7, 0, 5]                    # every finite id, larger first, lower id on ties
    assert kept(top_k=1) == [1]
    assert kept(top_k=2) == [1, 3]
    assert kept(top_k=3) == [1, 3, 4]                      # the tie at 2.0 is cut by id
    assert kept(top_k=5) == [1, 3, 4, 7, 0]
    assert kept(top_k=6) == kept(top_k=256) == [1, 3, 4, 7, 0, 5]              # -inf is never a candidate
    m = sampling.pick(x, 0, 0, P(top_k=3))[1]
    assert m["boundary"] == INF                            # an exact tie at the cut: the id decides
    assert sampling.pick(x, 0, 0, P(top_k=2, temperature=0.5))[1]["boundary"] == pytest.approx(2.0)     # (3 - 2) / 0.5
    # top-p: masses of softmax(x) over the candidates, in order
    e = np.exp(np.array([3.0, 3.0, 2.0, 2.0, 1.0, 0.5]) - 3.0)
    cum = np.cumsum(e) / e.sum()
    assert kept(top_p=0.01) == [1]                         # at least one
    assert kept(top_p=float(cum[0]) - 1e-3) == [1]
    assert kept(top_p=float(cum[0]) + 1e-3) == [1, 3]      # the shortest prefix with mass >= p
    assert kept(top_p=float(cum[2]) + 1e-3) == [1, 3, 4, 7]
    assert kept(top_p=0.999) == [1, 3, 4, 7, 0, 5]
    m = sampling.pick(x, 0, 0, P(top_p=float(cum[1]) + 1e-3))[1]
    assert list(m["kept"]) == [1, 3, 4] and m["mass"] == pytest.approx(1e-3, rel=1e-3)
    # the temperature sharpens the masses: at T = 0.25 the two 3.0 hold 0.96 of the mass
    assert kept(top_p=0.9, temperature=0.25) == [1, 3]
    # allowed: what the mask and the grammar leave
    allowed = np.ones(8, bool)
    allowed[[1, 4]] = False
    assert list(sampling.pick(x, 0, 0, P(top_k=3), allowed)[1]["kept"]) == [3, 7, 0]
    # the pick is one of the kept ids, the same for the same (seed, stream, t), and moves with each of them
    toks = {sampling.pick(x, t, s, P(seed=sd))[0] for t in range(4) for s in range(4) for sd in range(4)}
    assert toks <= {1, 3, 4, 7, 0, 5} and len(toks) >= 3
    assert sampling.pick(x, 2, 9, P(seed=5)) [0] == sampling.pick(x, 2, 9, P(seed=5))[0]


CHI_SEED = 2024


def test_chi_square_of_the_restatement():
    """an 8-id row at temperature 0.7: the picks of 4,096 streams with a fixed seed against softmax(x / 0.7); the statistic
    must stay under 24.3, the 0.999 quantile of chi-square with 7 degrees of freedom.  The run is deterministic."""
    x = np.array([0.3, 1.1, -0.4, 0.9, 0.0, -1.2, 0.6, 0.2], np.float32)
    p = P(temperature=0.7, seed=CHI_SEED)
    counts = np.zeros(8)
    for s in range(4096):
        counts[sampling.pick(x, 5, s, p)[0]] += 1
    z = x.astype(np.float64) / float(np.float32(0.7))
    prob = np.exp(z - z.max())
    prob /= prob.sum()
    chi2 = float(((counts - 4096 * prob) ** 2 / (4096 * prob)).sum())
    print("CHI2 %.3f counts %s" % (chi2, counts.astype(int).tolist()))
    assert chi2 < 24.3


def _engine(vocab=1536):
    lib = _lib.load()
    cfg = _lib.EngineConfig(vocab, 512, 6, 64, 1024, 1, 1, 512, 256, 64, 2, _lib.MT3_F32, 1)
    h = C.c_void_p()
    assert lib.mt3_engine_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


BAD = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=INF), dict(temperature=float("nan")),
       dict(top_k=-1), dict(top_k=257), dict(top_p=-0.1), dict(top_p=1.0), dict(top_p=float("nan")),
       dict(top_k=5, top_p=0.5)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_setter_and_driver_refuse_bad_parameters_before_device_work(bad):
    lib, h = _engine()
    try:
        s = _lib.Sampling(**{**dict(temperature=1.0, top_k=0, top_p=0.0, seed=1), **bad})
        assert lib.mt3_engine_set_sampling(h, C.byref(s), None, 0) == _lib.MT3_ERR_INVALID
        msg = lib.mt3_last_error()
        assert b"mt3_engine_set_sampling" in msg and b"finalized" not in msg
        fake = C.c_void_p(256)                             # never dereferenced: the refusal comes first
        rc = lib.mt3_op_token_steps_sampled(fake, None, 0, 0, 3, 300, 8, 0, 0, fake, fake, None, None, 0, None, None, 0,
                                            None, None, None, C.byref(s), None)
        assert rc == _lib.MT3_ERR_INVALID and b"mt3_op_token_steps_sampled" in lib.mt3_last_error()
        with pytest.raises(ValueError):
            P(**bad).check()
    finally:
        lib.mt3_engine_destroy(h)


def test_setter_refusals_that_need_no_device():
    good = _lib.Sampling(0.8, 0, 0.9, 3)
    streams = (C.c_uint64 * 4)(9, 1 << 40, 0, 5)
    lib, h = _engine()
    try:
        assert lib.mt3_engine_set_sampling(None, C.byref(good), None, 0) == _lib.MT3_ERR_INVALID
        assert lib.mt3_engine_set_sampling(h, C.byref(good), streams, 0) == _lib.MT3_ERR_INVALID
        assert b"n_segments" in lib.mt3_last_error()
        assert lib.mt3_engine_set_sampling(h, C.byref(good), streams, 4) == _lib.MT3_ERR_INVALID
        assert b"not finalized" in lib.mt3_last_error()
        assert lib.mt3_engine_set_sampling(h, C.byref(good), None, 0) == _lib.MT3_ERR_INVALID
        assert b"not finalized" in lib.mt3_last_error()
        assert lib.mt3_engine_set_sampling(h, None, None, 0) == _lib.MT3_ERR_INVALID      # clearing needs a finalized engine too
        assert lib.mt3_engine_status(h, _lib.STATUS_SAMPLING) == 0
    finally:
        lib.mt3_engine_destroy(h)
    lib, h = _engine(vocab=2176)                           # the kernel keeps the row in registers: vocab <= 2048
    try:
        assert lib.mt3_engine_set_sampling(h, C.byref(good), None, 0) == _lib.MT3_ERR_INVALID
        assert b"2048" in lib.mt3_last_error()
    finally:
        lib.mt3_engine_destroy(h)
    fake = C.c_void_p(256)
    call = lambda vocab, mode: lib.mt3_op_token_steps_sampled(fake, None, 0, 0, 3, vocab, 8, mode, 0, fake, fake, None, None,    # noqa: E731
                                                              0, None, None, 0, None, None, None, C.byref(good), None)
    assert call(2049, 0) == _lib.MT3_ERR_INVALID and b"2048" in lib.mt3_last_error()
    assert call(300, 1) == _lib.MT3_ERR_INVALID and b"beam-1" in lib.mt3_last_error()
