"""The token-rule kernels alone, on the scripted logits of tests/beam_script.py: beam_step / beam_finalize
(mt3_op_beam_search_scripted), argmax_step<false/true> (mt3_op_token_steps_scripted) and beam_reorder
(mt3_op_beam_reorder) against tests/beam_search_ref.py and plain numpy.  Every decision of every case is separated by
ten times the f32 score bound or is an exact tie in both arithmetics (tests/test_beam_script.py), so ids, parents,
retirement steps and the cache-row map must equal the reference bit for bit; no case is skipped or filtered.

Not covered: an OLD finished entry that exactly equals a NEW one (the header's "old entry on equal scores") -- the two
scores are divided by different brevity penalties and cannot be made equal in f32 and f64 alike.

Scores: the bound 1e-5 + 1e-6 |s| of tests/test_gpu_beam_search.py is in force, unraised; every case prints its maximum
error and its share of the bound (SCORE_ERR, with -s) before it asserts."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import beam_script as bs  # noqa: E402

DIM_E = 32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Run:
    pass


_runs = {}


def beam_run(case):
    """One run of the scripted search per case, shared by the tests below (with tables: the next-input rows too)."""
    if case.name in _runs:
        return _runs[case.name]
    k, n, T, V = case.k, case.elems * case.k, case.num_steps, case.V
    g = torch.Generator().manual_seed(len(case.name))
    r = Run()
    r.table, r.pos = torch.randn(V, DIM_E, generator=g), torch.randn(T + 1, DIM_E, generator=g)
    logits, ss = _dev(case.logits), (_dev(case.ss) if case.ss is not None else None)
    table, pos = r.table.cuda(), r.pos.cuda()
    ids = torch.full((case.elems, T), -7, dtype=torch.int32, device="cuda")
    all_ids = torch.full((case.elems, k, T), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((case.elems, k), float("nan"), device="cuda")
    y = torch.full((n, DIM_E), float("nan"), device="cuda")
    r.trace, r.live = np.full((T, 4, n), -9, np.int32), np.full((T, n), np.nan, np.float32)
    forks, ran = C.c_int32(-1), C.c_int32(-1)
    torch.cuda.synchronize()
    _lib.check(_lib.load().mt3_op_beam_search_scripted(
        _p(logits), _p(ss), case.n_ss, case.dim, case.elems, k, V, T, case.max_len, _p(table), _p(pos), DIM_E, _p(ids),
        _p(all_ids), _p(scores), _p(y), r.trace.ctypes.data, r.live.ctypes.data, C.byref(forks), C.byref(ran), None))
    torch.cuda.synchronize()
    assert torch.equal(logits.cpu(), torch.from_numpy(case.logits))           # the beam step never writes its logits
    r.ids, r.all_ids, r.scores, r.y = ids.cpu().numpy(), all_ids.cpu().numpy(), scores.cpu().numpy(), y.cpu()
    r.forks, r.steps_run = forks.value, ran.value
    _runs[case.name] = r
    return r


BEAM = pytest.mark.parametrize("case", bs.beam_cases(), ids=lambda c: c.name)


@BEAM
def test_beam_search_ids_scores_and_retirement(case):
    run, ref = beam_run(case), case.ref
    assert run.steps_run == ref.steps_run
    assert np.array_equal(run.all_ids, ref.decodes), case.name
    assert np.array_equal(run.ids, ref.decodes[:, -1])
    for t in range(ref.steps_run):
        done = run.trace[t, 2].reshape(case.elems, case.k)
        assert np.array_equal(done, np.repeat(ref.retired[t][:, None], case.k, 1).astype(np.int32)), (case.name, t)
    err = np.abs(run.scores.astype(np.float64) - ref.scores)
    bound = bs.SCORE_TOL[0] + bs.SCORE_TOL[1] * np.abs(ref.scores)
    print("SCORE_ERR %s max_abs %.3e max_over_bound %.3f" % (case.name, err.max(), (err / bound).max()))
    assert (err <= bound).all(), (case.name, err.max(), (err / bound).max())


@BEAM
def test_cache_row_protocol(case):
    """From the per-step trace: the slot -> row map stays a permutation of the element's rows, exactly the second and
    later children of a parent fork, no fork writes a row another fork reads, the fork count is the reference's, and a
    numpy "cache" of input tokens driven by the trace holds every live beam's input prefix after every step."""
    run, ref, k, n, T = beam_run(case), case.ref, case.k, case.elems * case.k, case.num_steps
    cache = np.full((n, T + 1), -1, np.int64)
    row_prev, tok_prev = np.arange(n), np.zeros(n, np.int64)              # identity map, BOS
    closed = np.zeros(case.elems, bool)
    forks = 0
    for t in range(run.steps_run):
        slot_row, fork_src, done, cur_tok = (x.astype(np.int64) for x in run.trace[t])
        for b in range(case.elems):
            sl = slice(b * k, (b + 1) * k)
            if closed[b]:                                                  # a closed element's state is final
                assert np.array_equal(run.trace[t][:, sl], run.trace[t - 1][:, sl]), (case.name, t, b)
                assert np.array_equal(run.live[t][sl], run.live[t - 1][sl])
                continue
            rows, src, parents = slot_row[sl], fork_src[sl], ref.index[t][sl] - b * k
            assert sorted(rows) == list(range(b * k, (b + 1) * k)), (case.name, t, b, rows)
            later = np.array([p in parents[:j] for j, p in enumerate(parents)])
            assert np.array_equal(src >= 0, later), (case.name, t, b, src, parents)
            old_rows = row_prev[sl][parents]
            assert np.array_equal(src[later], old_rows[later]) and np.array_equal(rows[~later], old_rows[~later])
            assert not set(rows[later]) & set(src[later]), (case.name, t, b)
            now_closed = bool(ref.retired[t][b])
            cache[row_prev[sl], t] = tok_prev[sl]                          # the step's attention appends its input token
            if not now_closed:                                             # (a closed element's forks are never copied)
                forks += k - len(set(parents))
                before = cache.copy()
                for j in np.flatnonzero(later):
                    cache[rows[j], :t + 1] = before[src[j], :t + 1]
                for j in range(k):
                    want = np.concatenate([[0], ref.live_seq[t][b, j, :t]])
                    assert np.array_equal(cache[rows[j], :t + 1], want), (case.name, t, b, j)
            assert np.array_equal(cur_tok[sl], ref.live_seq[t][b, :, t]), (case.name, t, b)
            lp = ref.live_lp[t][b]
            assert (np.abs(run.live[t][sl] - lp) <= bs.SCORE_TOL[0] + bs.SCORE_TOL[1] * np.abs(lp)).all(), (case.name, t, b)
            closed[b] = now_closed
        row_prev, tok_prev = slot_row, cur_tok
    assert forks == int(case.forks.sum()) and run.forks == forks, (case.name, run.forks, forks)
    assert (run.trace[run.steps_run:] == -9).all()


@BEAM
def test_next_input_row(case):
    """y_next[slot] = table[cur_tok] + pos[t + 1] exactly, t the last step the slot's element ran."""
    run, ref, k = beam_run(case), case.ref, case.k
    for b in range(case.elems):
        closed_at = [t for t in range(ref.steps_run) if ref.retired[t][b]]
        t = closed_at[0] if closed_at else ref.steps_run - 1
        for j in range(k):
            tok = int(run.trace[t, 3, b * k + j])
            assert tok == ref.live_seq[t][b, j, t]
            assert torch.equal(run.y[b * k + j], run.table[tok] + run.pos[t + 1]), (case.name, b, j)


def test_beam_search_without_tables_and_on_a_stream():
    """The optional tables left out, on a stream of the caller's: the same ids."""
    case = next(c for c in bs.beam_cases() if c.name == "table_v130_k7")
    k, n, T = case.k, case.elems * case.k, case.num_steps
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        logits = _dev(case.logits)
        ids = torch.zeros((case.elems, T), dtype=torch.int32, device="cuda")
        all_ids = torch.zeros((case.elems, k, T), dtype=torch.int32, device="cuda")
        scores = torch.zeros((case.elems, k), device="cuda")
        trace, live = np.zeros((T, 4, n), np.int32), np.zeros((T, n), np.float32)
        forks, ran = C.c_int32(-1), C.c_int32(-1)
        _lib.check(_lib.load().mt3_op_beam_search_scripted(
            _p(logits), None, 0, 0, case.elems, k, case.V, T, 0, None, None, 0, _p(ids), _p(all_ids), _p(scores), None,
            trace.ctypes.data, live.ctypes.data, C.byref(forks), C.byref(ran), C.c_void_p(s.cuda_stream)))
    assert np.array_equal(all_ids.cpu().numpy(), case.ref.decodes) and forks.value == case.forks.sum()


# ------------------------------------------------------------------------------------------------- token steps
def token_run(case, mode):
    B, T, V = case.elems, case.num_steps, case.V
    logits, ss = _dev(case.logits), (_dev(case.ss) if case.ss is not None else None)
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    done = np.full((T, B), -9, np.int32)
    torch.cuda.synchronize()
    _lib.check(_lib.load().mt3_op_token_steps_scripted(_p(logits), _p(ss), case.n_ss, case.dim, B, V, T, mode, case.max_len,
                                                       _p(ids), done.ctypes.data, None))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), done, logits.cpu().numpy()


TOKEN = pytest.mark.parametrize("case", bs.token_cases(), ids=lambda c: c.name)


@TOKEN
def test_greedy_token_steps(case):
    ids, done, logits = token_run(case, 0)
    want_ids, want_done = case.greedy()
    assert np.array_equal(ids, want_ids), case.name
    assert np.array_equal(done, want_done)
    if case.ss is None:
        assert np.array_equal(logits, case.logits)
    else:
        # the scaled logits are written back (these cases retire no row): rsqrtf of an f32 sum of <= 64 terms and one
        # product, under 8 ulp of f32 against the float64 scale
        assert not case.max_len
        for t in range(case.num_steps):
            assert np.allclose(logits[t], case.scaled(t), rtol=8 * 2.0 ** -23, atol=0), (case.name, t)


@TOKEN
def test_beam1_token_steps(case):
    ids, done, _ = token_run(case, 1)
    ref, T = case.ref, case.num_steps
    assert np.array_equal(ids, ref.decodes[:, 0]), case.name
    for t in range(T):
        want = ref.retired[t] if t < ref.steps_run else np.ones(case.elems, bool)
        assert np.array_equal(done[t], want.astype(np.int32)), (case.name, t)
    if case.V <= 2048:                     # "at k = 1 this is MT3_DECODE_BEAM1, and the ids are bit-identical to it"
        assert np.array_equal(ids, beam_run(case).ids), case.name
        assert beam_run(case).steps_run == ref.steps_run


# ----------------------------------------------------------------------------------------------------- reorder
LAYERS, H, CAP, SLOTS = 2, 2, 260, 16
STEPS = (1, 3, 255, 256, 257, 260)


@pytest.mark.parametrize("with_scale", (False, True), ids=("noscale", "scale"))
@pytest.mark.parametrize("esize", (1, 2, 4))
def test_beam_reorder_copies_the_forked_prefixes_and_nothing_else(esize, with_scale):
    """16 slots: 8 that do not fork (their rows are the sources), 6 that fork at the six step values, 2 that fork but
    are done (no copy).  Random bytes with runs of 0xFF (NaN in every cache type); afterwards positions [0, step) of a
    destination row equal its source in K, V and the scale pairs, and every other byte is what it was."""
    rng = np.random.default_rng(esize * 2 + with_scale)
    shape = (SLOTS, H, CAP, 64 * esize)

    def cache(last):
        x = rng.integers(0, 256, shape[:3] + (last,), dtype=np.uint8)
        x[rng.random(x.shape[:3]) < 0.1] = 0xFF
        return x

    k_h, v_h = [cache(64 * esize) for _ in range(LAYERS)], [cache(64 * esize) for _ in range(LAYERS)]
    s_h = [cache(8) for _ in range(LAYERS)]                                   # float2 per position
    slot_row = rng.permutation(SLOTS).astype(np.int32)
    slots = rng.permutation(SLOTS)
    plain, forking, done_fork = slots[:8], slots[8:14], slots[14:]
    fork_src = np.full(SLOTS, -1, np.int32)
    fork_src[forking] = slot_row[plain[:6]]
    fork_src[done_fork] = slot_row[plain[6:]]
    step = rng.integers(1, CAP + 1, SLOTS).astype(np.int32)
    step[forking] = STEPS
    step[done_fork] = 200
    done = np.zeros(SLOTS, np.int32)
    done[done_fork] = 1
    k_d, v_d, s_d = [_dev(x) for x in k_h], [_dev(x) for x in v_h], [_dev(x) for x in s_h]
    arr = lambda ts: (C.c_void_p * LAYERS)(*[t.data_ptr() for t in ts])      # noqa: E731
    dev = [_dev(x) for x in (fork_src, slot_row, step, done)]
    torch.cuda.synchronize()
    _lib.check(_lib.load().mt3_op_beam_reorder(LAYERS, H, CAP, esize, SLOTS, arr(k_d), arr(v_d),
                                               arr(s_d) if with_scale else None, *[_p(x) for x in dev], None))
    torch.cuda.synchronize()
    for name, host, devs, copied in (("k", k_h, k_d, True), ("v", v_h, v_d, True), ("scale", s_h, s_d, with_scale)):
        for l in range(LAYERS):
            want = host[l].copy()
            if copied:
                for s, n in zip(forking, STEPS):
                    want[slot_row[s], :, :n] = host[l][fork_src[s], :, :n]
            assert np.array_equal(devs[l].cpu().numpy(), want), (name, l)
            assert not np.array_equal(want, host[l]) or not copied
