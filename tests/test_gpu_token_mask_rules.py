"""The masked token-rule kernels on scripted logits: mt3_op_token_steps_masked / mt3_op_beam_search_masked on logits X
with masks M must equal, BIT FOR BIT, the existing scripted drivers on X' = X with the disallowed entries at -inf, and
both must equal the CPU references (tests/beam_script.run_reference, TokenCase.greedy) on X'.

How a case is made.  tests/beam_script.py builds logits Z over a vocabulary of V_z ids whose every decision is separated
by ten times the f32 score bound (or is an exact tie in both arithmetics).  A masked case embeds Z, in increasing id
order, into the ALLOWED ids of a wider vocabulary V = V_z + n_dis (ids 0 and 1 are always allowed, so EOS stays EOS and
the tie rules -- lower id, lower flattened index -- are preserved by the monotone map):
  X'[allowed] = Z, X'[disallowed] = -inf      every decision of X' is a decision of Z: as separated as Z's
  X [disallowed] = 20 + U(0, 1)               above every allowed logit: the unmasked kernels on X pick them, so the
                                              mask bites in every step (asserted)
Rows / elements carry the mask indices [-1, 0, 1, -1, ...] (two elements: [0, 1]); masks 0 and 1 disallow different ids.
An unconstrained row has -1e4 at mask 0's disallowed ids in X and X' alike: exp of it is exactly 0 in f32 and f64, so
its decisions are Z's too.  The CPU references take -inf (numpy / torch log_softmax), so -inf it is, not -1e30.

Cases: every case of token_cases() / beam_cases() that leaves room for disallowed ids below the kernels' vocabulary
limit (the beam cases at V_z = 2047 / 2048 cannot be widened; vocab 2048 is covered by the added shapes), then vocab 70
(a ragged last mask word), 2048 (the register path's edge), 2100 (greedy kernel only: the loop path), k in {1, 2, 8},
with and without d_ss, max_len on."""
import copy
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import beam_script as bs  # noqa: E402

NEG = -np.inf


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Masked:
    """z: the separated case; V: the wide vocabulary; masks uint32 [2][words]; row_mask int32 [elems]; X / Xp f32
    [T][elems * k][V]; shim: z with Xp as its logits (what the CPU references run on)."""

    def __init__(self, z, V):
        assert V > z.V + 1
        self.z, self.V, self.name = z, V, "%s_in_v%d" % (z.name, V)
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        n_dis = V - z.V
        words = (V + 31) // 32
        self.allowed, self.masks = [], np.zeros((2, words), np.uint32)
        for m in range(2):
            dis = 2 + rng.permutation(V - 2)[:n_dis]
            ok = np.setdiff1d(np.arange(V), dis)
            self.allowed.append(ok)
            for i in ok:
                self.masks[m, i >> 5] |= np.uint32(1 << (i & 31))
        e = z.elems
        self.row_mask = np.array(([-1, 0, 1] * e)[:e] if e >= 3 else [0, 1][:e], np.int32)
        T, n = z.num_steps, z.elems * z.k
        self.X = np.empty((T, n, V), np.float32)
        self.Xp = np.empty((T, n, V), np.float32)
        for b in range(e):
            rows = slice(b * z.k, (b + 1) * z.k)
            m = int(self.row_mask[b])
            ok = self.allowed[max(m, 0)]
            dis = np.setdiff1d(np.arange(V), ok)
            for A in (self.X, self.Xp):
                A[:, rows][:, :, ok] = z.logits[:, rows]
            if m < 0:
                self.X[:, rows][:, :, dis] = -1.0e4
                self.Xp[:, rows][:, :, dis] = -1.0e4
            else:
                self.X[:, rows][:, :, dis] = (20.0 + rng.random((T, z.k, n_dis))).astype(np.float32)
                self.Xp[:, rows][:, :, dis] = NEG
        self.shim = copy.copy(z)
        self.shim.logits, self.shim.V, self.shim._ref, self.shim.name = self.Xp, V, None, self.name + "_ref"


def _widen(z, limit):
    return min(z.V + max(3, z.V // 8), limit)


def beam_masked_cases():
    out = [Masked(z, _widen(z, 2048)) for z in bs.beam_cases() if z.V + 2 <= 2048]
    for k in (1, 2, 8):
        out.append(Masked(bs.Case("m70_k%d" % k, k, 50, 3, 12), 70))
        out.append(Masked(bs.Case("m2048_k%d" % k, k, 1800, 3, 8), 2048))
        out.append(Masked(bs.Case("m70_scale_k%d" % k, k, 50, 3, 12, n_ss=32), 70))
    out.append(Masked(bs.Case("m70_maxlen_k2", 2, 50, 3, 16, max_len=9,
                              plan=lambda b, t: "no_eos" if t >= 9 or b == 2 else "rand"), 70))
    return out


def token_masked_cases():
    out = [Masked(z, _widen(z, 1 << 20)) for z in bs.token_cases()]
    for V_z, V in ((50, 70), (1800, 2048), (1850, 2100)):
        out.append(Masked(bs.TokenCase("mt%d" % V, V_z, 3, 12, plan=lambda b, t: "rand" if b < 2 else "no_eos"), V))
        out.append(Masked(bs.TokenCase("mt%d_scale" % V, V_z, 3, 12, n_ss=32), V))
        out.append(Masked(bs.TokenCase("mt%d_maxlen" % V, V_z, 3, 14, max_len=8,
                                       plan=lambda b, t: "no_eos" if t >= 8 or b == 2 else "rand"), V))
    return out


_BEAM, _TOKEN = beam_masked_cases(), token_masked_cases()


# ------------------------------------------------------------------------------------------------------- beam
def _beam(c, logits_h, masked):
    z = c.z
    k, n, T, V = z.k, z.elems * z.k, z.num_steps, c.V
    logits, ss = _dev(logits_h), (_dev(z.ss) if z.ss is not None else None)
    ids = torch.full((z.elems, T), -7, dtype=torch.int32, device="cuda")
    all_ids = torch.full((z.elems, k, T), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((z.elems, k), float("nan"), device="cuda")
    trace, live = np.full((T, 4, n), -9, np.int32), np.full((T, n), np.nan, np.float32)
    forks, ran = C.c_int32(-1), C.c_int32(-1)
    args = [_p(logits), _p(ss), z.n_ss, z.dim, z.elems, k, V, T, z.max_len, None, None, 0, _p(ids), _p(all_ids),
            _p(scores), None, trace.ctypes.data, live.ctypes.data, C.byref(forks), C.byref(ran), None]
    keep = None
    torch.cuda.synchronize()
    if masked:
        keep = (_dev(c.masks), _dev(c.row_mask))
        _lib.check(_lib.load().mt3_op_beam_search_masked(*args, _p(keep[0]), 2, _p(keep[1])))
    else:
        _lib.check(_lib.load().mt3_op_beam_search_scripted(*args))
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), logits_h, equal_nan=True)      # the beam step never writes its logits
    return dict(ids=ids.cpu().numpy(), all_ids=all_ids.cpu().numpy(), scores=scores.cpu().numpy(), trace=trace, live=live,
                forks=forks.value, ran=ran.value)


@pytest.mark.parametrize("c", _BEAM, ids=lambda c: c.name)
def test_masked_beam_search_equals_the_search_on_premasked_logits(c):
    got, want, plain = _beam(c, c.X, True), _beam(c, c.Xp, False), _beam(c, c.X, False)
    for key in ("ids", "all_ids", "trace", "forks", "ran"):
        assert np.array_equal(got[key], want[key]), (c.name, key)
    for key in ("scores", "live"):                      # bit for bit: compared as integers, NaN (rows not run) included
        assert np.array_equal(got[key].view(np.int32), want[key].view(np.int32)), (c.name, key)
    assert not np.array_equal(got["all_ids"], plain["all_ids"]), "the mask does not bite"
    ref = c.shim.ref
    assert got["ran"] == ref.steps_run
    assert np.array_equal(got["all_ids"], ref.decodes), c.name
    assert np.array_equal(got["ids"], ref.decodes[:, -1])
    for t in range(ref.steps_run):
        done = got["trace"][t, 2].reshape(c.z.elems, c.z.k)
        assert np.array_equal(done, np.repeat(ref.retired[t][:, None], c.z.k, 1).astype(np.int32)), (c.name, t)
    err = np.abs(got["scores"].astype(np.float64) - ref.scores)
    bound = bs.SCORE_TOL[0] + bs.SCORE_TOL[1] * np.abs(ref.scores)
    print("SCORE_ERR %s max_abs %.3e max_over_bound %.3f" % (c.name, err.max(), (err / bound).max()))
    assert (err <= bound).all(), (c.name, err.max())
    for b in range(c.z.elems):                          # no decode of a masked element holds a disallowed id
        m = int(c.row_mask[b])
        if m >= 0:
            assert np.isin(got["all_ids"][b], c.allowed[m]).all(), (c.name, b)


# ------------------------------------------------------------------------------------------------------ token
def _token(c, logits_h, mode, masked):
    z = c.z
    B, T, V = z.elems, z.num_steps, c.V
    logits, ss = _dev(logits_h), (_dev(z.ss) if z.ss is not None else None)
    ids = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    done = np.full((T, B), -9, np.int32)
    args = [_p(logits), _p(ss), z.n_ss, z.dim, B, V, T, mode, z.max_len, _p(ids), done.ctypes.data, None]
    torch.cuda.synchronize()
    if masked:
        keep = (_dev(c.masks), _dev(c.row_mask))
        _lib.check(_lib.load().mt3_op_token_steps_masked(*args, _p(keep[0]), 2, _p(keep[1])))
    else:
        _lib.check(_lib.load().mt3_op_token_steps_scripted(*args))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), done, logits.cpu().numpy()


@pytest.mark.parametrize("mode", (0, 1), ids=("greedy", "beam1"))
@pytest.mark.parametrize("c", _TOKEN, ids=lambda c: c.name)
def test_masked_token_steps_equal_the_steps_on_premasked_logits(c, mode):
    ids, done, left = _token(c, c.X, mode, True)
    ids_p, done_p, _ = _token(c, c.Xp, mode, False)
    ids_x, _, left_x = _token(c, c.X, mode, False)
    assert np.array_equal(ids, ids_p) and np.array_equal(done, done_p), c.name
    assert not np.array_equal(ids, ids_x), "the mask does not bite"
    # the logits in memory stay the model's own: what the unmasked kernel leaves there (scaled in place with d_ss)
    assert np.array_equal(left, left_x) and np.isfinite(left).all(), c.name
    if c.z.ss is None:
        assert np.array_equal(left, c.X)
    if mode == 0:
        want_ids, want_done = c.shim.greedy()
        assert np.array_equal(ids, want_ids) and np.array_equal(done, want_done), c.name
    else:
        ref, T = c.shim.ref, c.z.num_steps
        assert np.array_equal(ids, ref.decodes[:, 0]), c.name
        for t in range(T):
            want = ref.retired[t] if t < ref.steps_run else np.ones(c.z.elems, bool)
            assert np.array_equal(done[t], want.astype(np.int32)), (c.name, t)
    for b in range(c.z.elems):
        m = int(c.row_mask[b])
        if m >= 0:
            assert np.isin(ids[b], c.allowed[m]).all(), (c.name, b)


def test_masked_drivers_refuse_bad_masks():
    """read back and checked before a kernel indexes with them: index out of range, no EOS, too few tokens, tail bits"""
    lib = _lib.load()
    V, T = 70, 2
    logits = torch.zeros((T, 2, V), device="cuda")
    ids = torch.zeros((2, T), dtype=torch.int32, device="cuda")
    done = np.zeros((T, 2), np.int32)
    full = np.array([[0xFFFFFFFF, 0xFFFFFFFF, 0x3F]], np.uint32)

    def call(masks, rows):
        m, r = _dev(masks), _dev(np.asarray(rows, np.int32))
        return lib.mt3_op_token_steps_masked(_p(logits), None, 0, 0, 2, V, T, 0, 0, _p(ids), done.ctypes.data, None, _p(m),
                                             int(masks.shape[0]), _p(r))

    assert call(full, [0, -1]) == _lib.MT3_OK
    for masks, rows in ((full, [0, 1]), (full, [-2, 0]), (full & np.uint32(~2 & 0xFFFFFFFF), [0, 0]),
                        (np.array([[2, 0, 0]], np.uint32), [0, 0]), (np.array([[3, 0, 0x40]], np.uint32), [0, 0])):
        assert call(masks, rows) == _lib.MT3_ERR_INVALID
        assert lib.mt3_last_error().startswith(b"mt3_op_token_steps_masked: ")
