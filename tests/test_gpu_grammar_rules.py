"""The GRAMMAR instantiations of the token-rule kernels on scripted logits: mt3_op_token_steps_grammar /
mt3_op_beam_search_grammar on every case of tests/grammar_script.py against tests/grammar_ref.py.  Every free decision of
every case is separated by ten times the f32 score bound (beam_script.GAP), so ids, all k decodes, done flags and the
packed grammar state of every slot after every step (h_state: a wrong parent permutation shows there) must equal the
reference exactly; scores are held to beam_script.SCORE_TOL.  With h_grammar == NULL the drivers are the _prompted ones,
bit for bit.

Shapes: three elements / rows, 12 to 16 steps; V = 70 (a ragged last mask word), 2048 (the register path's edge), 2100
(the loop path, token kernel only); k in {1, 2, 8}; with and without d_ss; max_len; a mask intersecting the grammar;
prompts of two kinds (a bare tie; program, pitch, tie, shift)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import beam_script as bs  # noqa: E402
from tests import grammar_ref as gr  # noqa: E402
from tests import grammar_script as gs  # noqa: E402

STRIDE = 4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_CASE = object()


def _tables(case, masks=_CASE):
    """device arrays of the case's prompts and masks (or of `masks`), and the driver arguments that name them"""
    masks = case.masks if masks is _CASE else masks
    keep = {}
    rows, index = [], []
    for p in case.prompts:
        if not p:
            index.append(-1)
            continue
        rows.append(list(p) + [0] * (STRIDE - len(p)))
        index.append(len(rows) - 1)
    if rows:
        keep["prompts"], keep["row_prompt"] = _dev(np.array(rows, np.int32)), _dev(np.array(index, np.int32))
    n_masks = 0
    if masks is not None:
        words, mi = gs.mask_words(masks, case.V)
        keep["masks"], keep["row_mask"], n_masks = _dev(words), _dev(mi), len(words)
    args = (_p(keep.get("masks")), n_masks, _p(keep.get("row_mask")), _p(keep.get("prompts")), STRIDE,
            _p(keep.get("row_prompt")))
    return keep, args


def _struct(g):
    return _lib.TokenGrammar(*[getattr(g, f) for f in gr.FIELDS])


def _beam(case, grammar=True, masks=_CASE, g=None, rc_only=False):
    k, n, T, V, E = case.k, case.elems * case.k, case.num_steps, case.V, case.elems
    logits, ss = _dev(case.logits), (_dev(case.ss) if case.ss is not None else None)
    ids = torch.full((E, T), -7, dtype=torch.int32, device="cuda")
    all_ids = torch.full((E, k, T), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((E, k), float("nan"), device="cuda")
    trace, live = np.full((T, 4, n), -9, np.int32), np.full((T, n), np.nan, np.float32)
    state = np.full((T, n), -9, np.int32)
    forks, ran = C.c_int32(-1), C.c_int32(-1)
    keep, tables = _tables(case, masks)
    g = _struct(g or case.g)
    torch.cuda.synchronize()
    lib = _lib.load()
    head = (_p(logits), _p(ss), case.n_ss, case.dim, E, k, V, T, case.max_len, None, None, 0, _p(ids), _p(all_ids),
            _p(scores), None, trace.ctypes.data, live.ctypes.data, C.byref(forks), C.byref(ran), None)
    if rc_only:
        return lib.mt3_op_beam_search_grammar(*head, *tables, C.byref(g), state.ctypes.data)
    if grammar is None:
        _lib.check(lib.mt3_op_beam_search_prompted(*head, *tables))
    else:
        _lib.check(lib.mt3_op_beam_search_grammar(*head, *tables, C.byref(g) if grammar else None, state.ctypes.data))
    torch.cuda.synchronize()
    return dict(ids=ids.cpu().numpy(), all_ids=all_ids.cpu().numpy(), scores=scores.cpu().numpy(), trace=trace, live=live,
                forks=forks.value, ran=ran.value, state=state)


@pytest.mark.parametrize("case", gs.beam_cases(), ids=lambda c: c.name)
def test_grammar_beam_search(case):
    got, ref = _beam(case), case.ref
    k, E = case.k, case.elems
    assert got["ran"] == ref.steps_run
    assert np.array_equal(got["all_ids"], ref.decodes), case.name
    assert np.array_equal(got["ids"], ref.decodes[:, -1])
    err = np.abs(got["scores"].astype(np.float64) - ref.scores)
    bound = bs.SCORE_TOL[0] + bs.SCORE_TOL[1] * np.abs(ref.scores)
    print("SCORE_ERR %s max_abs %.3e max_over_bound %.3f" % (case.name, err.max(), (err / bound).max()))
    assert (err <= bound).all(), (case.name, err.max())
    for t in range(ref.steps_run):
        want = np.array([gr.as_i32(s) for s in ref.states[t]], np.int32)
        assert np.array_equal(got["state"][t], want), (case.name, t, got["state"][t], want)
        done = got["trace"][t, 2].reshape(E, k)
        assert np.array_equal(done, np.repeat(ref.retired[t].astype(np.int32)[:, None], k, 1)), (case.name, t)
    assert (got["state"][ref.steps_run:] == -9).all()
    for b in range(E):                                   # every decode is well formed
        for d in got["all_ids"][b]:
            assert gr.accepts(case.g, d, case.plen(b)), (case.name, b)
    plain = _beam(case, grammar=False)                   # NULL grammar: the _prompted driver, bit for bit
    prompted = _beam(case, grammar=None)
    for key in ("ids", "all_ids", "trace", "forks", "ran"):
        assert np.array_equal(plain[key], prompted[key]), (case.name, key)
    assert np.array_equal(plain["scores"].view(np.int32), prompted["scores"].view(np.int32))
    assert np.array_equal(plain["live"].view(np.int32), prompted["live"].view(np.int32))
    assert (plain["state"] == -9).all()
    assert not np.array_equal(plain["all_ids"], got["all_ids"])         # the grammar bit


def _token(case, mode, grammar=True, masks=_CASE, g=None, rc_only=False):
    B, T, V = case.elems, case.num_steps, case.V
    logits, ss = _dev(case.logits), (_dev(case.ss) if case.ss is not None else None)
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    done, state = np.full((T, B), -9, np.int32), np.full((T, B), -9, np.int32)
    keep, tables = _tables(case, masks)
    g = _struct(g or case.g)
    torch.cuda.synchronize()
    lib = _lib.load()
    head = (_p(logits), _p(ss), case.n_ss, case.dim, B, V, T, mode, case.max_len, _p(ids), done.ctypes.data, None)
    if rc_only:
        return lib.mt3_op_token_steps_grammar(*head, *tables, C.byref(g), state.ctypes.data)
    if grammar is None:
        _lib.check(lib.mt3_op_token_steps_prompted(*head, *tables))
    else:
        _lib.check(lib.mt3_op_token_steps_grammar(*head, *tables, C.byref(g) if grammar else None, state.ctypes.data))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), done, state, logits.cpu().numpy()


@pytest.mark.parametrize("mode", (0, 1), ids=("greedy", "beam1"))
@pytest.mark.parametrize("case", gs.token_cases(), ids=lambda c: c.name)
def test_grammar_token_steps(case, mode):
    ids, done, state, left = _token(case, mode)
    T = case.num_steps
    if mode == 0:
        scaled = np.stack([case.scaled(t) for t in range(T)])
        want_ids, want_done, want_state = gr.greedy(scaled, case.prompts, case.g, case.masks, case.max_len)
        assert np.array_equal(ids, want_ids) and np.array_equal(done, want_done), case.name
        assert np.array_equal(state, np.vectorize(gr.as_i32)(want_state).astype(np.int32)), case.name
    else:
        ref = case.ref
        assert np.array_equal(ids, ref.decodes[:, 0]), case.name
        for t in range(T):
            want = ref.retired[t] if t < ref.steps_run else np.ones(case.elems, bool)
            assert np.array_equal(done[t], want.astype(np.int32)), (case.name, t)
        for t in range(ref.steps_run):
            assert np.array_equal(state[t], np.array([gr.as_i32(s) for s in ref.states[t]], np.int32)), (case.name, t)
    for b in range(case.elems):
        assert gr.accepts(case.g, ids[b], case.plen(b)), (case.name, b)
    # the logits in memory stay the model's own: what the prompted kernel leaves there (scaled in place with d_ss)
    p_ids, p_done, _, p_left = _token(case, mode, grammar=None)
    assert np.array_equal(left, p_left)
    n_ids, n_done, n_state, n_left = _token(case, mode, grammar=False)     # NULL grammar: the _prompted driver
    assert np.array_equal(n_ids, p_ids) and np.array_equal(n_done, p_done) and np.array_equal(n_left, p_left)
    assert (n_state == -9).all() and not np.array_equal(n_ids, ids)


def _case(cases, name):
    return next(c for c in cases if c.name == name)


def test_drivers_refuse_a_mask_that_leaves_the_grammar_no_room():
    """MT3_ERR_INVALID for a mask whose intersection with the grammar leaves fewer than 2 (token kernel) / 2k (beam kernel)
    ids in the tie-section state; the same masks are accepted without a tie section (with_ties = 0) or with enough ids"""
    lib = _lib.load()
    section = list(range(gs.PITCH0, gs.PITCH0 + 12)) + list(range(gs.PROGRAM0, gs.PROGRAM0 + 8)) + [gs.TIE]
    only_eos = gs._mask(70, section)                                   # the tie section keeps EOS alone: 1 id
    three = gs._mask(70, [i for i in section if i not in (gs.TIE, gs.PITCH0)])      # EOS, tie, one pitch: 3 = 2k - 1 at k = 2
    no_ties = gs.toy_grammar(0)
    tok, b2, b8 = _case(gs.token_cases(), "gt_v70"), _case(gs.beam_cases(), "g_v70_k2"), _case(gs.beam_cases(), "g_v70_k8")
    for mode in (0, 1):
        assert _token(tok, mode, masks=[only_eos, None, None], rc_only=True) == _lib.MT3_ERR_INVALID
        assert b"mt3_op_token_steps_grammar" in lib.mt3_last_error() and b"fewer than" in lib.mt3_last_error()
        assert _token(tok, mode, masks=[None, None, only_eos], rc_only=True) == _lib.MT3_ERR_INVALID   # wherever it is listed
        assert _token(tok, mode, masks=[three, None, None], rc_only=True) == _lib.MT3_OK               # 3 >= 2
        assert _token(tok, mode, masks=[only_eos, None, None], g=no_ties, rc_only=True) == _lib.MT3_OK
    assert _beam(b2, masks=[three, None, None], rc_only=True) == _lib.MT3_ERR_INVALID                  # 3 < 2k = 4
    assert b"mt3_op_beam_search_grammar" in lib.mt3_last_error() and b"fewer than" in lib.mt3_last_error()
    assert _beam(b2, masks=[three, None, None], g=no_ties, rc_only=True) == _lib.MT3_OK
    # the mask of g_v70_mask at k = 8: the tie section holds 12 ids, 2k = 16
    forbid = list(range(gs.PITCH0, gs.PITCH0 + 12, 2)) + list(range(gs.PROGRAM0, gs.PROGRAM0 + 8, 2)) + \
        list(range(gs.SHIFT0 + 1, 23, 2))
    half = gs._mask(70, forbid)
    assert int(gr._rule_vector(b8.g, gr.initial(b8.g), half, 70).sum()) == 12
    assert _beam(b8, masks=[half, None, half], rc_only=True) == _lib.MT3_ERR_INVALID
    assert _beam(b8, masks=[half, None, half], g=no_ties, rc_only=True) == _lib.MT3_OK
    assert _beam(b2, masks=[half, None, half], rc_only=True) == _lib.MT3_OK                            # 12 >= 4
