"""The PROMPT instantiations of the token-rule kernels on scripted logits: mt3_op_token_steps_prompted /
mt3_op_beam_search_prompted against tests/prompt_ref.py.  Every free decision of every case is separated by ten times the
f32 score bound (prompt_ref.PromptCase, as tests/beam_script.py has it), so ids, done flags, the slot -> row map and the
fork sources must equal the reference exactly; scores and live log-probs are held to beam_script.SCORE_TOL, the bound
tests/test_gpu_token_rules.py uses for the same quantities.  No case is skipped.

Shapes: rows 5 / elems 3, 12 steps, vocab 96 (and 2100 for the token kernel's element-loop path), k in {1, 2, 4, 8},
prompt lengths none / 1 / 3 / 11 mixed within one launch, with and without d_ss, max_len inside the longest prompt,
scripted EOS inside a prompt, and masks that forbid a prompt token."""
import copy
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import beam_script as bs  # noqa: E402
from tests import prompt_ref as pr  # noqa: E402

DIM_E = 32
STRIDE = 11


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _prompt_arrays(prompts, stride=STRIDE):
    """the prompts in use as rows [n][stride] (0-padded) and the per-row index (-1: none)"""
    rows, index = [], []
    for p in prompts:
        if not p:
            index.append(-1)
            continue
        rows.append(list(p) + [0] * (stride - len(p)))
        index.append(len(rows) - 1)
    return np.array(rows, np.int32).reshape(-1, stride), np.array(index, np.int32)


def _beam(case, logits_h, prompts, masks=None, row_mask=None, V=None):
    k, n, T, V = case.k, case.elems * case.k, case.num_steps, V or case.V
    g = torch.Generator().manual_seed(len(case.name))
    table, pos = torch.randn(V, DIM_E, generator=g), torch.randn(T + 1, DIM_E, generator=g)
    logits, ss = _dev(logits_h), (_dev(case.ss) if case.ss is not None else None)
    ids = torch.full((case.elems, T), -7, dtype=torch.int32, device="cuda")
    all_ids = torch.full((case.elems, k, T), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((case.elems, k), float("nan"), device="cuda")
    y = torch.full((n, DIM_E), float("nan"), device="cuda")
    trace, live = np.full((T, 4, n), -9, np.int32), np.full((T, n), np.nan, np.float32)
    forks, ran = C.c_int32(-1), C.c_int32(-1)
    rows, index = _prompt_arrays(prompts)
    keep = [_dev(rows), _dev(index), table.cuda(), pos.cuda(), _dev(masks) if masks is not None else None,
            _dev(row_mask) if row_mask is not None else None]
    torch.cuda.synchronize()
    _lib.check(_lib.load().mt3_op_beam_search_prompted(
        _p(logits), _p(ss), case.n_ss, case.dim, case.elems, k, V, T, case.max_len, _p(keep[2]), _p(keep[3]), DIM_E,
        _p(ids), _p(all_ids), _p(scores), _p(y), trace.ctypes.data, live.ctypes.data, C.byref(forks), C.byref(ran), None,
        _p(keep[4]), 0 if masks is None else masks.shape[0], _p(keep[5]), _p(keep[0]), STRIDE, _p(keep[1])))
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), logits_h, equal_nan=True)      # the beam step never writes its logits
    return dict(ids=ids.cpu().numpy(), all_ids=all_ids.cpu().numpy(), scores=scores.cpu().numpy(), trace=trace, live=live,
                forks=forks.value, ran=ran.value, y=y.cpu(), table=table, pos=pos)


def _check_beam(case, got, ref, prompts):
    """ids, scores, and from the per-step trace: done flags, the slot -> row map, the fork sources, the input tokens and
    the live log-probs of every step, the fork count and the next input rows"""
    k, n, E = case.k, case.elems * case.k, case.elems
    assert got["ran"] == ref.steps_run
    assert np.array_equal(got["all_ids"], ref.decodes), case.name
    assert np.array_equal(got["ids"], ref.decodes[:, -1])
    err = np.abs(got["scores"].astype(np.float64) - ref.scores)
    bound = bs.SCORE_TOL[0] + bs.SCORE_TOL[1] * np.abs(ref.scores)
    print("SCORE_ERR %s max_abs %.3e max_over_bound %.3f" % (case.name, err.max(), (err / bound).max()))
    assert (err <= bound).all(), (case.name, err.max())
    row_prev = np.arange(n)
    closed = np.zeros(E, bool)
    forks = 0
    last = np.zeros(E, int)
    for t in range(ref.steps_run):
        slot_row, fork_src, done, cur_tok = (x.astype(np.int64) for x in got["trace"][t])
        for b in range(E):
            sl = slice(b * k, (b + 1) * k)
            if closed[b]:                                                  # a closed element's state is final
                assert np.array_equal(got["trace"][t][:, sl], got["trace"][t - 1][:, sl]), (case.name, t, b)
                assert np.array_equal(got["live"][t][sl], got["live"][t - 1][sl])
                continue
            last[b] = t
            parents = ref.index[t][sl] - b * k
            orow = row_prev[sl]
            free = [orow[j] for j in range(k) if j not in parents]
            claimed, want_row, want_src = set(), [], []
            for p in parents:                                              # the rule of beam_step_kernel, step 3
                if p not in claimed:
                    claimed.add(p)
                    want_row.append(orow[p])
                    want_src.append(-1)
                else:
                    want_row.append(free.pop(0))
                    want_src.append(orow[p])
            assert np.array_equal(slot_row[sl], want_row), (case.name, t, b)
            assert np.array_equal(fork_src[sl], want_src), (case.name, t, b)
            inside = t < len(prompts[b] or [])
            if inside:                                                     # nothing forks, the map does not move
                assert np.array_equal(slot_row[sl], orow) and (fork_src[sl] == -1).all()
                assert (cur_tok[sl] == prompts[b][t]).all()
            now_closed = bool(ref.retired[t][b])
            assert (done[sl] == int(now_closed)).all(), (case.name, t, b)
            assert not (inside and now_closed) or (case.max_len and t + 1 >= case.max_len)
            if not now_closed:
                forks += k - len(set(parents))
            assert np.array_equal(cur_tok[sl], ref.live_seq[t][b, :, t]), (case.name, t, b)
            lp = ref.live_lp[t][b]
            assert (np.abs(got["live"][t][sl] - lp) <= bs.SCORE_TOL[0] + bs.SCORE_TOL[1] * np.abs(lp)).all(), (case.name, t, b)
            if inside:
                assert np.array_equal(got["live"][t][sl], np.array([0.0] + [bs.NEG_INF] * (k - 1), np.float32))
            closed[b] = now_closed
        row_prev = slot_row
    assert got["forks"] == forks, (case.name, got["forks"], forks)
    assert (got["trace"][got["ran"]:] == -9).all()
    for b in range(E):                                                     # y_next = table[cur_tok] + pos[t + 1], exactly
        t = int(last[b])
        for j in range(k):
            tok = int(got["trace"][t, 3, b * k + j])
            assert torch.equal(got["y"][b * k + j], got["table"][tok] + got["pos"][t + 1]), (case.name, b, j)


_BEAM = pr.beam_prompt_cases()


@pytest.mark.parametrize("case", _BEAM, ids=lambda c: c.name)
def test_prompted_beam_search(case):
    got = _beam(case, case.logits, case.prompts)
    _check_beam(case, got, case.ref, case.prompts)
    for b in range(case.elems):                          # every decode that holds a token starts with the prompt
        p = (case.prompts[b] or [])[: case.max_len or None]
        for d in got["all_ids"][b]:
            assert not d.any() or list(d[:len(p)]) == p, (case.name, b)
    if "eos_inside" in case.name:                        # EOS on top of every row at steps 1, 2: no finish inside a prompt
        for b in range(case.elems):
            if case.plen(b) >= 3:
                assert (got["trace"][1:3, 2, b * case.k] == 0).all()
                assert not (got["all_ids"][b][:, 1:3] == bs.EOS).any()
    if "maxlen" in case.name:                            # element 2 is closed inside its prompt: P[:max_len], k times
        want = np.zeros(case.num_steps, np.int32)
        want[:case.max_len] = case.prompts[2][:case.max_len]
        assert (got["all_ids"][2] == want).all() and got["ran"] == case.max_len


def _token(case, logits_h, mode, prompts, masks=None, row_mask=None, V=None):
    B, T, V = case.elems, case.num_steps, V or case.V
    logits, ss = _dev(logits_h), (_dev(case.ss) if case.ss is not None else None)
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    done = np.full((T, B), -9, np.int32)
    rows, index = _prompt_arrays(prompts)
    keep = [_dev(rows), _dev(index), _dev(masks) if masks is not None else None,
            _dev(row_mask) if row_mask is not None else None]
    torch.cuda.synchronize()
    _lib.check(_lib.load().mt3_op_token_steps_prompted(
        _p(logits), _p(ss), case.n_ss, case.dim, B, V, T, mode, case.max_len, _p(ids), done.ctypes.data, None, _p(keep[2]),
        0 if masks is None else masks.shape[0], _p(keep[3]), _p(keep[0]), STRIDE, _p(keep[1])))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), done, logits.cpu().numpy()


def _check_beam1(case, ids, done, ref):
    assert np.array_equal(ids, ref.decodes[:, 0]), case.name
    for t in range(case.num_steps):
        want = ref.retired[t] if t < ref.steps_run else np.ones(case.elems, bool)
        assert np.array_equal(done[t], want.astype(np.int32)), (case.name, t)


_TOKEN = pr.token_prompt_cases()


@pytest.mark.parametrize("mode", (0, 1), ids=("greedy", "beam1"))
@pytest.mark.parametrize("case", _TOKEN, ids=lambda c: c.name)
def test_prompted_token_steps(case, mode):
    ids, done, left = _token(case, case.logits, mode, case.prompts)
    plain = _lib.load().mt3_op_token_steps_scripted
    if mode == 0:
        want_ids, want_done = pr.greedy(case.logits, case.prompts, case.max_len)
        assert np.array_equal(ids, want_ids) and np.array_equal(done, want_done), case.name
    else:
        _check_beam1(case, ids, done, case.ref)
        if case.V <= 2048:                               # at k = 1 the beam kernel's ids are beam-1's, bit for bit
            got = _beam(case, case.logits, case.prompts)
            assert np.array_equal(got["ids"], ids), case.name
    for b in range(case.elems):
        p = (case.prompts[b] or [])[: case.max_len or None]
        assert list(ids[b, :len(p)]) == p
    # the logits in memory stay the model's own: what the unprompted kernel leaves there (scaled in place with d_ss)
    x = _dev(case.logits)
    o = torch.zeros((case.elems, case.num_steps), dtype=torch.int32, device="cuda")
    d = np.zeros((case.num_steps, case.elems), np.int32)
    if not case.max_len:
        _lib.check(plain(_p(x), _p(_dev(case.ss)) if case.ss is not None else None, case.n_ss, case.dim, case.elems, case.V,
                         case.num_steps, mode, 0, _p(o), d.ctypes.data, None))
        torch.cuda.synchronize()
        assert np.array_equal(left, x.cpu().numpy()), case.name
        assert not np.array_equal(ids, o.cpu().numpy()), "the prompts do not bite"


def test_no_prompts_is_the_scripted_driver():
    """d_prompts == NULL, and prompts for no row: the ids of mt3_op_token_steps_scripted / mt3_op_beam_search_scripted"""
    case = next(c for c in bs.beam_cases() if c.name == "four_elems_k3")
    for prompts in ([None] * case.elems,):
        got = _beam(case, case.logits, prompts)
        assert np.array_equal(got["all_ids"], case.ref.decodes) and got["forks"] == case.forks.sum()
    tc = next(c for c in bs.token_cases() if c.name == "tok_v257")
    ids, done, _ = _token(tc, tc.logits, 0, [None] * tc.elems)
    assert np.array_equal(ids, tc.greedy()[0]) and np.array_equal(done, tc.greedy()[1])


# ---------------------------------------------------------------------------------------------- masks and prompts
class MaskedPrompt:
    """A PromptCase z over V_z ids embedded, in increasing id order, into the allowed ids of V = 96 (the construction of
    tests/test_gpu_token_mask_rules.py): X holds 20 + U at the disallowed ids, Xp -inf (what the reference runs on).
    Every element carries the mask; the prompts are drawn in the WIDE id space and each holds a disallowed id."""

    def __init__(self, z, V=96):
        self.z, self.V, self.name = z, V, z.name + "_masked"
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        n_dis = V - z.V
        self.dis = np.sort(2 + rng.permutation(V - 2)[:n_dis])
        self.ok = np.setdiff1d(np.arange(V), self.dis)
        self.masks = np.zeros((1, (V + 31) // 32), np.uint32)
        for i in self.ok:
            self.masks[0, i >> 5] |= np.uint32(1 << (i & 31))
        self.row_mask = np.zeros(z.elems, np.int32)
        T, n = z.num_steps, z.elems * z.k
        self.X, self.Xp = np.empty((T, n, V), np.float32), np.empty((T, n, V), np.float32)
        for A in (self.X, self.Xp):
            A[:, :, self.ok] = z.logits
        self.X[:, :, self.dis] = (20.0 + rng.random((T, n, n_dis))).astype(np.float32)
        self.Xp[:, :, self.dis] = -np.inf
        self.prompts = []
        for b in range(z.elems):
            p = [int(x) for x in rng.integers(2, V, z.plen(b))]
            if p:
                p[-1] = int(self.dis[b % n_dis])                          # forbidden by the element's mask
            self.prompts.append(p or None)
        self.shim = copy.copy(z)
        self.shim.logits, self.shim.V, self.shim._ref, self.shim.prompts = self.Xp, V, None, self.prompts


def test_masks_and_prompts_beam():
    z = pr.PromptCase("pm_k2", 2, 90, 3, pr.T, pr.prompts_for("pm", 90, 3))
    c = MaskedPrompt(z)
    got = _beam(z, c.X, c.prompts, c.masks, c.row_mask, V=c.V)
    _check_beam(z, got, c.shim.ref, c.prompts)
    for b in range(z.elems):
        p = c.prompts[b] or []
        for d in got["all_ids"][b]:
            if d.any():
                assert list(d[:len(p)]) == p                               # the forbidden prompt token is emitted
                assert np.isin(d[len(p):], c.ok).all()                     # the mask holds from t = p


@pytest.mark.parametrize("mode", (0, 1), ids=("greedy", "beam1"))
def test_masks_and_prompts_token(mode):
    z = pr.PromptCase("pmt", 1, 90, 5, pr.T, pr.prompts_for("pmt", 90, 5))
    c = MaskedPrompt(z)
    ids, done, left = _token(z, c.X, mode, c.prompts, c.masks, c.row_mask, V=c.V)
    if mode == 0:
        want_ids, want_done = pr.greedy(c.Xp, c.prompts)
        assert np.array_equal(ids, want_ids) and np.array_equal(done, want_done)
    else:
        _check_beam1(z, ids, done, c.shim.ref)
    assert np.array_equal(left, c.X)                                       # unmasked, unscaled: the model's own
    for b in range(z.elems):
        p = c.prompts[b] or []
        assert list(ids[b, :len(p)]) == p and np.isin(ids[b, len(p):], c.ok).all()
