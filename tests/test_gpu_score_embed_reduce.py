"""score_embed_kernel and score_logprob_kernel / score_token_stats_kernel + score_sum_kernel alone (mt3_op_score_embed,
mt3_op_score_reduce; include/mt3_hip.h states the rules) against the numpy forms of tests/score_prefill_ref.py.

What each check would catch:
  embed, bit-equal rows       a token taken from the wrong position (shift-right off by one, BOS missing at t = 0), the
                              position row of another t, a row tail the 128 x 4 stride skips (dim 64 / 512 / 768: less than
                              one pass, exactly one, one and a half), ids that leave the table instead of being clamped
  seg0 in {0, 2}              a dropped or doubled chunk offset into the caller's [4][length] arrays
  rows past length            a padding row that reads the caller's arrays past the segment (token and target must be 0)
  sentinels                   a store outside the chunk's rows of y / tgt_pad / tok_pad, outside segments seg0 .. seg0 + 1
                              of the caller's token scores and sequence scores, or at t >= length of tok_pad
  token scores, 1e-5          a wrong maximum / sum reduction over vocabularies that are no multiple of the 256 threads
                              (tolerance and rows: tests/test_gpu_score_token_stats.py, the same arithmetic)
  sequence score, 1 f32 ulp   a sum that drops or doubles a position, reads t >= length of tok_pad (those hold 1e30
                              here), or runs in f32: the kernel sums <= 128 floats in double, which is exact to far below
                              f32 resolution, so float32(fsum(token scores the kernel wrote)) is the result up to the
                              final rounding -- one ulp allows for a tie there
  repeat, stats route         bits that depend on the run or on which of the two reduction kernels ran
MEASURED on MI355X: max |token score - float64| 2.2e-6 over all cases (bound 1e-5); every sequence score within one ulp;
the embed rows bit-equal.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import score_prefill_ref as R  # noqa: E402
from tests.test_gpu_score_token_stats import _rows  # noqa: E402

SEGS, BATCH, LP = 2, 4, 128                       # a chunk of 2 segments out of caller arrays of 4
TOL = 1e-5                                        # tests/test_gpu_score_token_stats.py


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ embed
@pytest.mark.parametrize("given", [False, True], ids=["shift_right", "dec_in_given"])
@pytest.mark.parametrize("seg0", [0, 2])
@pytest.mark.parametrize("length", [70, 128])
@pytest.mark.parametrize("dim", [64, 512, 768])
def test_embed_rows(dim, length, seg0, given):
    vocab, rows, guard = 37, SEGS * LP, 3
    rng = np.random.default_rng(dim + length + seg0)
    table = rng.standard_normal((vocab, dim)).astype(np.float32)
    pos = rng.standard_normal((LP, dim)).astype(np.float32)
    targets = rng.integers(1, vocab, (BATCH, length)).astype(np.int32)
    dec_in = rng.integers(0, vocab, (BATCH, length)).astype(np.int32)
    for a in (targets, dec_in):                   # in every segment: ids outside the vocabulary, and a padding target
        a[:, 5], a[:, 6], a[:, 9] = -4, 5000, 0
        a[:, length - 1] = 5000
    y = torch.full((rows + 2 * guard, dim), -7.5, device="cuda")
    tgt_pad = torch.full((rows + 2 * guard,), -77, device="cuda", dtype=torch.int32)
    d = [dev(table), dev(pos), dev(targets), dev(dec_in) if given else None]
    _lib.check(_lib.load().mt3_op_score_embed(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                              d[3].data_ptr() if given else None, tgt_pad[guard:].data_ptr(),
                                              y[guard:].data_ptr(), rows, LP, length, seg0, dim, vocab, stream()))
    torch.cuda.synchronize()
    want_y, want_t = R.embed_rows_ref(table, pos, targets, dec_in if given else None, SEGS, LP, length, seg0, vocab)
    y, tgt_pad = y.cpu().numpy(), tgt_pad.cpu().numpy()
    assert np.array_equal(tgt_pad[guard:guard + rows], want_t)
    assert np.array_equal(bits(y[guard:guard + rows]), bits(want_y))
    assert (y[:guard] == -7.5).all() and (y[guard + rows:] == -7.5).all()
    assert (tgt_pad[:guard] == -77).all() and (tgt_pad[guard + rows:] == -77).all()
    # spelled out, independent of embed_rows_ref: clamping, BOS, padding rows
    t2, y2 = want_t.reshape(SEGS, LP), y[guard:guard + rows].reshape(SEGS, LP, dim)
    assert (t2[:, 5] == 0).all() and (t2[:, 6] == vocab - 1).all() and (t2[:, length:] == 0).all()
    for s in range(SEGS):
        tok0 = int(np.clip(dec_in[seg0 + s, 0], 0, vocab - 1)) if given else 0
        assert np.array_equal(y2[s, 0], table[tok0] + pos[0])
        tok7 = vocab - 1                          # the input at t = 7 is id 5000 either way (dec_in[6] / targets[6])
        assert np.array_equal(y2[s, 7 if not given else 6], table[tok7] + pos[7 if not given else 6])
        if length < LP:
            assert np.array_equal(y2[s, length:], np.broadcast_to(table[0], (LP - length, dim)) + pos[length:])


# ----------------------------------------------------------------------------------------------------------- reduce
def chunk_logits(V, length, seed):
    """[SEGS * LP][V] logits and [SEGS * LP] padded targets: the scripted rows of test_gpu_score_token_stats.py first, random
    rows after them; targets 0 past `length` and at a few scripted positions"""
    x, tgt, _, _ = _rows(V, seed)
    rng = np.random.default_rng(seed)
    n = SEGS * LP
    logits = (rng.standard_normal((n, V)) * 3.0).astype(np.float32)
    tgts = rng.integers(1, V, n).astype(np.int32)
    for s in range(SEGS):
        logits[s * LP: s * LP + len(x)] = x
        tgts[s * LP: s * LP + len(x)] = tgt
    tgts = tgts.reshape(SEGS, LP)
    tgts[:, length:] = 0
    tgts[:, 40:44] = 0
    return logits, tgts.reshape(-1)


def run_reduce(logits, tgt_pad, weights, length, seg0, V, top1):
    """-> (tok_pad [rows], token_scores [BATCH][length], seq_scores [BATCH], top1_ids, top1_scores) with sentinels where
    the launch writes nothing"""
    rows = SEGS * LP
    tok_pad = torch.full((rows,), 1e30, device="cuda")
    token_scores = torch.full((BATCH, length), 7.0, device="cuda")
    seq = torch.full((BATCH,), 7.0, device="cuda")
    ids = torch.full((BATCH, length), -7, device="cuda", dtype=torch.int32) if top1 else None
    tsc = torch.full((BATCH, length), 7.0, device="cuda") if top1 else None
    d = [dev(logits), dev(tgt_pad), dev(weights) if weights is not None else None]
    _lib.check(_lib.load().mt3_op_score_reduce(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if d[2] is not None else None,
                                               tok_pad.data_ptr(), token_scores.data_ptr(), seq.data_ptr(), rows, LP, length,
                                               seg0, V, ids.data_ptr() if top1 else None, tsc.data_ptr() if top1 else None,
                                               stream()))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (tok_pad, token_scores, seq, ids, tsc))


def ulps(a, b):
    """distance of two finite f32 of one sign in units in the last place"""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("weighted", [False, True], ids=["weights_null", "weights_given"])
@pytest.mark.parametrize("seg0", [0, 2])
@pytest.mark.parametrize("length", [70, 128])
@pytest.mark.parametrize("V", [257, 1536])
def test_reduce(V, length, seg0, weighted):
    logits, tgt_pad = chunk_logits(V, length, seed=V + length)
    weights = np.random.default_rng(3).uniform(0.25, 1.0, (BATCH, length)).astype(np.float32) if weighted else None
    tok_pad, tok, seq, _, _ = run_reduce(logits, tgt_pad, weights, length, seg0, V, top1=False)
    sl = slice(seg0, seg0 + SEGS)
    w_rows = None
    if weighted:
        w_rows = np.ones((SEGS, LP), np.float32)
        w_rows[:, :length] = weights[sl]
        w_rows = w_rows.reshape(-1)
    ref = R.token_scores_ref(logits, tgt_pad, w_rows).reshape(SEGS, LP)
    pad2 = tok_pad.reshape(SEGS, LP)
    err = float(np.abs(pad2[:, :length] - ref[:, :length]).max())
    print(f"reduce V {V} length {length} seg0 {seg0} {'weighted' if weighted else 'unweighted'}: max |token score - "
          f"float64| {err:.2e} (bound {TOL:.0e})")
    assert err <= TOL
    live = tgt_pad.reshape(SEGS, LP)[:, :length] != 0
    assert (pad2[:, :length][~live] == 0).all() and (~live).sum() >= 4 * SEGS      # padding targets: exactly 0
    if weighted:                                  # the weights are applied (they are not all 1: a dropped weight shows)
        plain = R.token_scores_ref(logits, tgt_pad, None).reshape(SEGS, LP)
        assert float(np.abs(pad2[:, :length] - plain[:, :length]).max()) > 100 * TOL
    # placement: the caller's rows of segments seg0, seg0 + 1 hold the chunk's scores, everything else its sentinel
    assert np.array_equal(bits(tok[sl]), bits(pad2[:, :length]))
    others = [b for b in range(BATCH) if not seg0 <= b < seg0 + SEGS]
    assert (tok[others] == 7.0).all() and (seq[others] == 7.0).all()
    assert (pad2[:, length:] == np.float32(1e30)).all()                             # t >= length: not written ...
    for s in range(SEGS):                         # ... and not read: the sum is the sum of what the kernel wrote
        want = np.float32(math.fsum(float(v) for v in pad2[s, :length]))
        assert np.isfinite(seq[seg0 + s]) and ulps(seq[seg0 + s], want) <= 1, (s, seq[seg0 + s], want)
    # the same call again, and the statistics route: the same bits
    again = run_reduce(logits, tgt_pad, weights, length, seg0, V, top1=False)
    stats = run_reduce(logits, tgt_pad, weights, length, seg0, V, top1=True)
    for got in (again, stats):
        assert np.array_equal(bits(got[0]), bits(tok_pad)) and np.array_equal(bits(got[1]), bits(tok))
        assert np.array_equal(bits(got[2]), bits(seq))
    # the statistics route's own outputs: the arg-max (numpy: the first maximum) where the target is not 0
    ids = stats[3][sl]
    top = logits.astype(np.float64).argmax(-1).reshape(SEGS, LP)[:, :length]
    assert np.array_equal(ids[live], top[live]) and (ids[~live] == 0).all() and (stats[3][others] == -7).all()
    assert (stats[4][sl] <= 0).all() and (stats[4][others] == 7.0).all()
