"""sample_step_kernel on scripted logits (mt3_op_token_steps_sampled) against the numpy restatement mt3_amd/sampling.py,
step by step, on the cases of tests/sampling_script.py: 5 rows x 12 steps; V = 40 (a partial mask word), 300 (no multiple
of 256) and 2048 (the register limit); with and without d_ss row scales; plain sampling, top_k 1 / 5 / 256, top_p 0.3 /
0.9; and masks, prompts, the toy grammar and max_len together.  Before the GPU result is looked at, every pick of the
reference is asserted clear of the margins (sampling_script.MARGIN: 100 times the f32 error of x / T + g); with that the
ids and done flags must be EQUAL.  Exact identities: top_k = 1 is the greedy driver bit for bit, NULL sampling is the
_grammar driver bit for bit, and permuting the rows together with their streams permutes the ids."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib, sampling  # noqa: E402
from tests import grammar_ref as gr  # noqa: E402
from tests import grammar_script as gs  # noqa: E402
from tests import sampling_script as ss  # noqa: E402

STRIDE = 4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _run(case, params="case", streams="case", rows=None, driver="sampled"):
    """the driver on the case's logits (rows: a permutation of its rows); params None: NULL sampling; streams None: NULL
    h_row_stream; driver 'grammar': mt3_op_token_steps_grammar.  Returns ids [B][T], done [T][B], the logits left behind"""
    B, T, V = ss.ROWS, ss.STEPS, case.V
    rows = list(range(B)) if rows is None else list(rows)
    logits = _dev(case.logits[:, rows])
    ss_dev = _dev(case.ss[:, rows]) if case.ss is not None else None
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    done, state = np.full((T, B), -9, np.int32), np.full((T, B), -9, np.int32)
    keep, tables = {}, [None, 0, None, None, STRIDE, None]
    if case.masks is not None:
        words, index = gs.mask_words([case.masks[r] for r in rows], V)
        keep["m"], keep["mi"] = _dev(words), _dev(index)
        tables[:3] = [_p(keep["m"]), len(words), _p(keep["mi"])]
    if case.prompts is not None:
        prows, index = [], []
        for r in rows:
            p = case.prompts[r]
            index.append(len(prows) if p else -1)
            if p:
                prows.append(list(p) + [0] * (STRIDE - len(p)))
        keep["p"], keep["pi"] = _dev(np.array(prows, np.int32)), _dev(np.array(index, np.int32))
        tables[3], tables[5] = _p(keep["p"]), _p(keep["pi"])
    g = _lib.TokenGrammar(*[getattr(case.g, f) for f in gr.FIELDS]) if case.g is not None else None
    params = case.params if isinstance(params, str) else params
    st = params.struct() if params is not None else None
    streams = case.streams[rows] if isinstance(streams, str) else streams
    streams = np.ascontiguousarray(streams, dtype=np.uint64) if streams is not None else None
    torch.cuda.synchronize()
    lib = _lib.load()
    head = (_p(logits), _p(ss_dev), case.n_ss, case.dim, B, V, T, 0, case.max_len, _p(ids), done.ctypes.data, None)
    tail = (C.byref(g) if g is not None else None, state.ctypes.data)
    if driver == "grammar":
        _lib.check(lib.mt3_op_token_steps_grammar(*head, *tables, *tail))
    else:
        _lib.check(lib.mt3_op_token_steps_sampled(*head, *tables, *tail, C.byref(st) if st is not None else None,
                                                  streams.ctypes.data if streams is not None else None))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), done, logits.cpu().numpy()


@pytest.mark.parametrize("case", ss.cases(), ids=lambda c: c.name)
def test_ids_equal_the_restatement_step_by_step(case):
    # the margin condition, on the CPU, before the GPU is asked: no pick is excluded
    assert len(case.margins) >= 20
    for b, t, m in case.margins:
        assert m["pick"] >= ss.PICK_MARGIN and m["boundary"] >= ss.BOUNDARY_MARGIN and m["mass"] >= ss.MASS_MARGIN, (b, t, m)
    ids, done, left = _run(case)
    assert np.array_equal(ids, case.ids), (case.name, np.argwhere(ids != case.ids)[:5])
    assert np.array_equal(done, case.done), case.name
    # the logits handed back stay the model's own: what the greedy driver leaves there (scaled in place with d_ss)
    g_ids, g_done, g_left = _run(case, driver="grammar")
    # (a row that max_len retires is no longer visited, hence no longer scaled: compare where both runs were live)
    live = np.ones((ss.STEPS, ss.ROWS), bool)
    if case.max_len:
        live[1:] = (done[:-1] == 0) & (g_done[:-1] == 0)
    assert np.array_equal(left[live], g_left[live])
    if case.params.top_k != 1:
        assert not np.array_equal(ids, g_ids)                # it samples: the greedy ids are others


@pytest.mark.parametrize("case", [c for c in ss.cases() if c.mode[0] in ("plain", "p90")], ids=lambda c: c.name)
def test_exact_identities(case):
    greedy = _run(case, driver="grammar")
    # top_k = 1 is greedy, bit for bit, ids and done flags, whatever seed and temperature
    for T, seed in ((0.3, 1), (1.7, (1 << 64) - 1)):
        k1 = _run(case, params=sampling.SamplingParams(temperature=T, top_k=1, seed=seed))
        assert np.array_equal(k1[0], greedy[0]) and np.array_equal(k1[1], greedy[1]) and np.array_equal(k1[2], greedy[2])
    # NULL sampling is the _grammar driver
    null = _run(case, params=None)
    assert np.array_equal(null[0], greedy[0]) and np.array_equal(null[1], greedy[1]) and np.array_equal(null[2], greedy[2])
    # the rows permuted together with their streams: the ids permuted; the same call twice: the same bits
    base = _run(case)
    perm = [3, 0, 4, 2, 1]
    moved = _run(case, rows=perm)
    assert np.array_equal(moved[0], base[0][perm]) and np.array_equal(moved[1], base[1][:, perm])
    again = _run(case)
    assert np.array_equal(again[0], base[0]) and np.array_equal(again[1], base[1])


def test_null_streams_are_the_row_indices():
    case = next(c for c in ss.cases() if c.name == "v300_plain")
    by_default = _run(case, streams=None)
    named = _run(case, streams=np.arange(ss.ROWS, dtype=np.uint64))
    assert np.array_equal(by_default[0], named[0])
    assert not np.array_equal(by_default[0], _run(case)[0])  # and the streams matter
    other_seed = sampling.SamplingParams(**{**case.mode[1], "seed": case.params.seed ^ 1})
    assert not np.array_equal(_run(case, params=other_seed)[0], _run(case)[0])
