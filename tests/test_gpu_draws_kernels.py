"""The two kernel changes behind mt3_engine_transcribe_draws, each alone on scripted state.

Seeds (mt3_op_token_steps_seeded): sample_step_kernel with a per-row Philox key.  5 rows x 8 steps of scripted logits at
vocabulary 1536, drawn as tests/sampling_script.py draws its rows (logits on a grid of 1/64, a head of a few ids holding
the mass) and, as there, re-drawn on the CPU until every pick of the numpy restatement is clear of sampling_script's
margins -- the GPU is not asked.  Streams and seeds lie past 2^32; two rows share a stream and differ in the seed alone.

Refill copy (mt3_op_slot_refill_draws): `per` consecutive restarted slots copy one staged entry.  The expectation is
tests/slot_moves_ref.refill on a staging chunk in which every entry stands `per` times in a row -- the replicated job the
engine call is held to -- and the whole of every allocation is compared, guards included, as tests/test_gpu_slot_moves.py
does."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, sampling  # noqa: E402
from tests import sampling_script as ss  # noqa: E402
from tests import slot_moves_ref as ref  # noqa: E402
from tests import test_gpu_slot_moves as sm  # noqa: E402

ROWS, STEPS, V = 5, 8, 1536
MODES = {"plain": dict(temperature=0.8), "p90": dict(temperature=1.2, top_p=0.9), "k5": dict(temperature=0.7, top_k=5)}


def _reference(logits, streams, seeds, params):
    """the sampled greedy loop of sampling_script.reference with row b's picks under seeds[b]"""
    T, B, _ = logits.shape
    ids, done, margins = np.zeros((B, T), np.int32), np.zeros((T, B), np.int32), []
    for b in range(B):
        over = False
        for t in range(T):
            if not over:
                tok, m = sampling.pick(logits[t, b], t, int(streams[b]), params, seed=int(seeds[b]))
                margins.append((b, t, m))
                ids[b, t] = tok
                over = tok == ss.EOS
            done[t, b] = over
    return ids, done, margins


def _case(mode):
    """logits f32 [T][B][V], streams, seeds, params, and the reference's ids and done flags: the first draw whose picks
    are all clear of the margins"""
    for draw in range(ss.MAX_DRAWS):
        rng = np.random.default_rng(7000 + 97 * sorted(MODES).index(mode) + draw)
        x = np.round((rng.normal(0, 1.0, (STEPS, ROWS, V)) - 8.0) * 64) / 64
        for t in range(STEPS):
            for b in range(ROWS):
                head = rng.choice(V, int(rng.integers(3, 30)), replace=False)
                x[t, b, head] = 6.0 + np.round(rng.uniform(0, 3, head.size) * 64) / 64
                if rng.random() < 0.15:
                    x[t, b, ss.EOS] = 7.5
                x[t, b, rng.choice(V, 4, replace=False)] = x[t, b].max()
        x[:, 1] = x[:, 0]                                   # rows 0 and 1: the same logits and stream, seeds apart
        logits = x.astype(np.float32)
        streams = (rng.integers(0, 1 << 62, ROWS, dtype=np.uint64) | np.uint64(1 << 40)).astype(np.uint64)
        streams[1] = streams[0]
        seeds = (rng.integers(0, 1 << 63, ROWS, dtype=np.uint64) | np.uint64(1 << 33)).astype(np.uint64)
        seeds[2], seeds[3] = np.uint64((1 << 64) - 1), np.uint64(1 << 32)
        params = sampling.SamplingParams(seed=int(rng.integers(0, 1 << 63)), **MODES[mode])
        ids, done, margins = _reference(logits.astype(np.float64), streams, seeds, params)
        if ss.clear(margins):
            return logits, streams, seeds, params, ids, done, margins
    raise AssertionError("%s: no draw with every pick clear of the margins" % mode)


def _run(logits, streams, params, seeds=None, driver="seeded"):
    T, B, vocab = logits.shape
    d_logits = torch.from_numpy(np.ascontiguousarray(logits)).cuda()
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    done = np.full((T, B), -9, np.int32)
    st = params.struct()
    streams = np.ascontiguousarray(streams, dtype=np.uint64)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64) if seeds is not None else None
    torch.cuda.synchronize()
    lib = _lib.load()
    args = (C.c_void_p(d_logits.data_ptr()), None, 0, 0, B, vocab, T, 0, 0, C.c_void_p(ids.data_ptr()), done.ctypes.data,
            None, None, 0, None, None, 0, None, None, None, C.byref(st), streams.ctypes.data, None, None)
    if driver == "notes":
        _lib.check(lib.mt3_op_token_steps_notes(*args))
    else:
        _lib.check(lib.mt3_op_token_steps_seeded(*args, seeds.ctypes.data if seeds is not None else None))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), done


@pytest.mark.parametrize("mode", sorted(MODES))
def test_seeds_in_the_sampling_kernel(mode):
    logits, streams, seeds, params, want_ids, want_done, margins = _case(mode)
    assert len(margins) >= 20
    ids, done = _run(logits, streams, params, seeds)
    assert np.array_equal(ids, want_ids), np.argwhere(ids != want_ids)[:5]
    assert np.array_equal(done, want_done)
    assert not np.array_equal(ids[0], ids[1])               # one segment's logits and stream, two seeds: two draws
    # a row with seed k is that row alone under mt3_sampling.seed = k, without a table
    for b in range(ROWS):
        alone = sampling.SamplingParams(**{**MODES[mode], "seed": int(seeds[b])})
        for driver in ("notes", "seeded"):
            one_ids, one_done = _run(logits[:, b:b + 1], streams[b:b + 1], alone, None, driver)
            assert np.array_equal(one_ids[0], ids[b]) and np.array_equal(one_done[:, 0], done[:, b]), (b, driver)
    # every row under the parameters' own seed: the table and no table agree
    same = np.full(ROWS, params.seed, np.uint64)
    by_table, by_params = _run(logits, streams, params, same), _run(logits, streams, params, None)
    assert np.array_equal(by_table[0], by_params[0]) and np.array_equal(by_table[1], by_params[1])
    # NULL seeds: the _notes driver, bit for bit
    notes = _run(logits, streams, params, None, "notes")
    assert np.array_equal(notes[0], by_params[0]) and np.array_equal(notes[1], by_params[1])
    assert not np.array_equal(by_params[0], ids)            # and the seeds matter


# ---------------------------------------------------------------------------------------------------- refill copy
def _refill_draws(rng, rows, n_new, done, slot_seg, src_batch, entry0, per, row_bytes, sc_bytes, scales, what,
                  driver="draws"):
    """one mt3_op_slot_refill_draws (driver 'plain': mt3_op_slot_refill, per = 1) against slot_moves_ref.refill on the
    chunk with every entry `per` times in a row; returns the expected owned state"""
    dim, q_n, form, stride = 16, 4, sm.FORMS[2], 9
    batch, n_segs, first_seg = rows + 7, 2 * rows + 5 + n_new, rows + 5
    cbufs = sm.cross_bufs(rng, src_batch, batch, row_bytes, sc_bytes, scales)
    for l, layer in enumerate(cbufs["src"]):                 # every staged row filled with its own byte pattern
        img = layer.host[layer.g:layer.g + layer.n].reshape(2, src_batch, row_bytes)
        for kv in range(2):
            for e in range(src_batch):
                img[kv, e] = (np.arange(row_bytes) * 7 + 31 * e + 101 * kv + 13 * l) % 251
    b = sm.refill_state(rng, rows, batch, done, slot_seg)
    b.update(sm.row_bufs(rng, rows, dim, q_n, form))
    b["n_done"] = sm.Buf(rng, np.array([int((done != 0).sum())], np.int32), "n_done")
    b["ids"] = sm.Buf(rng, sm.bits(rng, np.int32, (batch, stride)), "ids")
    b["out_ids"] = sm.Buf(rng, sm.bits(rng, np.int32, (n_segs, stride)), "out_ids")
    b.update(cbufs)
    s = sm.owned(b)
    wide = dict(s)
    wide["src"] = [np.repeat(a, per, axis=1) for a in s["src"]]
    wide["src_sc"] = [None if a is None else np.repeat(a, per, axis=0) for a in s["src_sc"]]
    want, plan_ref = ref.refill(wide, rows, n_new, first_seg, entry0, sm.tables(dim, q_n)["bos"], 0)
    want["src"], want["src_sc"] = s["src"], s["src_sc"]      # the chunk itself is an input: untouched
    plan, keep = np.full(rows + 1, -5, np.int32), []

    def call():
        x = sm.cross_view(cbufs, src_batch, entry0, batch, row_bytes, sc_bytes, keep)
        head = (C.byref(sm.state_view(b)), C.byref(sm.row_view(b, dim, q_n, sm.MAX_POS)), None, 0, None, None, b["ids"].ptr,
                stride, b["out_ids"].ptr, rows, n_new, first_seg, C.byref(x))
        if driver == "plain":
            return _lib.load().mt3_op_slot_refill(*head, plan.ctypes.data, None)
        return _lib.load().mt3_op_slot_refill_draws(*head, per, plan.ctypes.data, None)

    sm.run(b, want, call, what)
    assert np.array_equal(plan, plan_ref), what
    return want, s


@pytest.mark.parametrize("row_bytes,sc_bytes,scales", [(48, 16, False), (sm.BIG_ROW8, 2064, True)])
def test_refill_copies_one_staged_entry_into_per_slots(row_bytes, sc_bytes, scales):
    """8 slots, 2 layers, staged batch 3, per = 3, src_entry0 = 2, n_new = 5: restarted slot i holds entry (2 + i) / 3 --
    the run starts in the middle of entry 0's draws -- and the e4m3 scale rows follow where the view has them"""
    rng = np.random.default_rng(row_bytes)
    rows, per, entry0, n_new, src_batch = 8, 3, 2, 5, 3
    done = np.array([1, 0, 1, 1, 1, 0, 1, 1])
    seg = np.array([4, 9, -1, 2, 7, 1, -1, 5])
    want, s = _refill_draws(rng, rows, n_new, done, seg, src_batch, entry0, per, row_bytes, sc_bytes, scales, "per 3")
    # (of the SCRIPT, in the issue's own words: the i-th restarted slot holds entry (2 + i) / 3)
    fin = np.flatnonzero(done)
    for i, slot in enumerate(fin[:n_new]):
        row, entry = s["slot_row"][slot], (entry0 + i) // per
        for layer in range(2):
            for kv in range(2):
                assert np.array_equal(want["dst"][layer][kv, row], s["src"][layer][kv, entry]), (i, layer, kv)
        if scales:
            assert np.array_equal(want["dst_sc"][1][row], s["src_sc"][1][entry]), i
        assert want["slot_seg"][slot] == rows + 5 + i
    assert [int((entry0 + i) // per) for i in range(n_new)] == [0, 1, 1, 1, 2]
    assert all(want["slot_seg"][slot] == -1 for slot in fin[n_new:])


def test_refill_draws_with_per_1_is_the_plain_refill():
    rows, entry0, n_new, src_batch = 8, 2, 5, 8
    done = np.array([1, 0, 1, 1, 1, 0, 1, 1])
    seg = np.array([4, 9, -1, 2, 7, 1, -1, 5])
    got = [_refill_draws(np.random.default_rng(5), rows, n_new, done, seg, src_batch, entry0, 1, 48, 16, True, d, d)[0]
           for d in ("draws", "plain")]
    for k in got[0]:                                         # both met the same expectation; and it is the same one
        a, b = got[0][k], got[1][k]
        for u, v in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
            assert (u is None and v is None) or np.array_equal(u, v), k
