"""The slot-moving launches alone, on scripted slot state: the input-row writer (mt3_op_embed_rows), the compaction of
row retirement (mt3_op_slot_compact), the refills of in-flight batching (mt3_op_slot_refill, mt3_op_beam_refill) and the
start of a k-beam streaming job (mt3_op_beam_stream_init) against tests/slot_moves_ref.py.

Everything is compared as raw bits.  Payloads the launches only move are random bit patterns with runs of 0xFF (NaN
patterns compare like any other value); the tables a row is computed from are finite.  Every array is one device
allocation of GUARD slots of random bits, the slots the launch owns, and GUARD more slots; the WHOLE allocation is
compared with what the reference leaves, so a byte written outside the owned slots fails the test, and so does a
written input (tables, staging chunks, histories).  No case is filtered or skipped.  The only inexact check is the
embed rows' y_ss against float64 sums (1e-6 relative, the bound of test_residual_split_exact); the same y_ss is also
compared bit for bit with mt3_op_residual_split and, for the BOS row, with the rational-arithmetic statement of
slot_moves_ref.split_sums_f32.

Shapes are the smallest that cross each kernel's loop seams (128 threads x 4 columns per trip of the row writer, 64
lanes per ballot of the plans, 8 / 16 parts x 256 lanes x 16 bytes per sweep of the cross copy, 256 threads of the beam
element block).  The large cross-copy rows run with up to 40 cache rows per element group only (elems <= 5): the copy's
index arithmetic is per row and 64-bit, and rows 70 x 8 deep would move 150 MB per run for no new path."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import _lib  # noqa: E402
from tests import slot_moves_ref as ref  # noqa: E402

# guard slots on either side of the owned region (8: a position the embed cases clamp, 13 of max_pos 8, would without the
# clamp still read inside the tables' allocations)
GUARD = 8
BF16 = _lib.MT3_BF16


def bits(rng, dtype, shape):
    """random bit patterns with runs of 0xFF"""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    b = rng.integers(0, 256, n, np.uint8)
    starts = rng.integers(0, max(n, 1), 1 + n // 64)
    lens = rng.integers(1, 9, len(starts))
    for i in range(8):
        at = starts[lens > i] + i
        b[at[at < n]] = 0xFF
    return b.view(dtype).reshape(shape)


class Buf:
    """guard | owned | guard in one device allocation; `owned` is an integer-typed (raw bits) or f32 array whose first
    axis indexes slots (slot: the elements of one slot where it does not)"""

    def __init__(self, rng, owned, name, slot=None):
        owned = np.ascontiguousarray(owned)
        self.name, self.shape, self.dtype = name, owned.shape, owned.dtype
        slot = slot or max(int(np.prod(owned.shape[1:])), 1)
        self.g, self.n = GUARD * slot, owned.size
        int_t = np.dtype("u%d" % owned.dtype.itemsize)
        self.host = np.concatenate([bits(rng, int_t, self.g), owned.reshape(-1).view(int_t), bits(rng, int_t, self.g)])
        assert (self.g * int_t.itemsize) % 16 == 0                         # the owned region keeps 16-byte alignment
        self.dev = None

    def owned(self):
        return self.host[self.g:self.g + self.n].view(self.dtype).reshape(self.shape)

    @property
    def ptr(self):
        if self.dev is None:
            self.dev = torch.from_numpy(self.host.copy()).cuda()
        return self.dev.data_ptr() + self.g * self.host.itemsize

    def result(self):
        return self.dev.cpu().numpy()

    def check(self, expect=None, what=""):
        """the whole allocation against the host image with the owned region replaced by `expect` (None: untouched)"""
        want = self.host.copy()
        if expect is not None:
            want[self.g:self.g + self.n] = np.ascontiguousarray(expect).reshape(-1).view(self.host.dtype)
        got = self.result()
        self.dev = None
        if not np.array_equal(got, want):
            at = np.flatnonzero(got != want)
            where = "owned" if self.g <= at[0] < self.g + self.n else "GUARD"
            raise AssertionError("%s %s: %d words differ, first at %d (%s region, owned index %d): got %#x want %#x" % (
                self.name, what, len(at), at[0], where, at[0] - self.g, got[at[0]], want[at[0]]))


def run(bufs, expect, call, what):
    """upload `bufs` (dict name -> Buf | list of Buf | None), call, and compare every allocation with `expect`"""
    flat = [(k, i, b) for k, v in bufs.items() for i, b in enumerate(v if isinstance(v, list) else [v]) if b is not None]
    for _, _, b in flat:
        b.ptr
    torch.cuda.synchronize()
    _lib.check(call())
    torch.cuda.synchronize()
    for k, i, b in flat:
        e = expect.get(k)
        b.check(e[i] if isinstance(e, list) else e, what)


def owned(bufs):
    return {k: ([None if b is None else b.owned() for b in v] if isinstance(v, list) else
                None if v is None else v.owned()) for k, v in bufs.items()}


def ptr(b):
    return b.ptr if b is not None else None


def row_view(bufs, dim, q_n, max_pos=0):
    g = lambda k: ptr(bufs.get(k))
    return _lib.InputRowView(table=g("table"), pos=g("pos"), max_pos=max_pos, dim=dim, y=g("y"), y_ct=g("y_ct"),
                             y_ss=g("y_ss"), ew=g("ew"), pw=g("pw"), q_out=g("q_out"), q_n=q_n)


def state_view(bufs):
    g = lambda k: ptr(bufs.get(k))
    return _lib.SlotStateView(done=g("done"), slot_row=g("slot_row"), slot_seg=g("slot_seg"), step=g("step"),
                              cur_tok=g("cur_tok"), n_done=g("n_done"))


FORMS = [("y",), ("y", "y_ss"), ("y", "y_ct", "y_ss")]               # f32 only; the f32 engine's split; the bf16 path
MAX_POS, VOCAB = 8, 11
_tables = {}


def tables(dim, q_n):
    """finite tables of one (dim, q_n), and the BOS row the reference makes of them"""
    if (dim, q_n) not in _tables:
        rng = np.random.default_rng(dim * 4099 + q_n)
        t = {"table": (rng.standard_normal((VOCAB, dim)) * 3).astype(np.float32),
             "pos": rng.standard_normal((MAX_POS, dim)).astype(np.float32)}
        if q_n:
            t["ew"] = rng.standard_normal((VOCAB, q_n)).astype(np.float32)
            t["pw"] = rng.standard_normal((MAX_POS, q_n)).astype(np.float32)
        t["bos"] = ref.bos_row(t["table"], t["pos"], t.get("ew"), t.get("pw"))
        _tables[(dim, q_n)] = t
    return _tables[(dim, q_n)]


def row_bufs(rng, slots, dim, q_n, form, with_tables=True):
    """the forms `form` (+ q_out with q_n) of `slots` input rows as random payload, and their tables"""
    t = tables(dim, q_n)
    b = {"y": Buf(rng, bits(rng, np.uint32, (slots, dim)), "y")}
    if "y_ct" in form:
        b["y_ct"] = Buf(rng, bits(rng, np.uint16, (slots, dim)), "y_ct")
    if "y_ss" in form:
        b["y_ss"] = Buf(rng, bits(rng, np.uint32, (slots, dim // 16)), "y_ss")
    if q_n:
        b["q_out"] = Buf(rng, bits(rng, np.uint32, (slots, q_n)), "q_out")
    if with_tables:
        for k in ("table", "pos") + (("ew", "pw") if q_n else ()):
            b[k] = Buf(rng, t[k], k)
    return b


# ---------------------------------------------------------------------------------------------------- embed
EMBED_T = np.array([0, 7, 8, 13, 3, 8, 0, 13, 6], np.int32)          # max_pos = 8: 8 and 13 are clamped to 7
EMBED_TOK = np.array([0, 10, 5, 0, 10, 1, 7, 3, 9], np.int32)


def residual_split(y_buf, rows, dim):
    ct = torch.empty(rows, dim, device="cuda", dtype=torch.bfloat16)
    ss = torch.empty(rows, dim // 16, device="cuda")
    _lib.check(_lib.load().mt3_op_residual_split(BF16, y_buf.ptr, ct.data_ptr(), ss.data_ptr(), rows, dim, None))
    torch.cuda.synchronize()
    return ct.view(torch.int16).cpu().numpy().view(np.uint16), ss.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("dim", [16, 512, 528, 768])
def test_embed_rows(dim):
    rng = np.random.default_rng(dim)
    rows = len(EMBED_T)
    for q_n, form in itertools.product([0, 4, 516, 2048], FORMS):
        t = tables(dim, q_n)
        b = row_bufs(rng, rows, dim, q_n, form)
        b["tok"], b["t"] = Buf(rng, EMBED_TOK, "tok"), Buf(rng, EMBED_T, "t")
        want = ref.embed(t["table"], t["pos"], MAX_POS, EMBED_TOK, EMBED_T, t.get("ew"), t.get("pw"))
        what = "dim %d q_n %d %s" % (dim, q_n, "+".join(form))
        for v in b.values():
            v.ptr
        torch.cuda.synchronize()
        _lib.check(_lib.load().mt3_op_embed_rows(C.byref(row_view(b, dim, q_n, MAX_POS)), b["tok"].ptr, b["t"].ptr, rows,
                                                 None))
        torch.cuda.synchronize()
        if "y_ss" in form:
            # the reference states y_ss in float64; its bits are those of mt3_op_residual_split on the same y (the same
            # put_row_piece arithmetic), and with those bits the whole allocation, guards included, is compared below
            ss = b["y_ss"]
            got = ss.result()[ss.g:ss.g + ss.n].reshape(rows, dim // 16)
            rel = np.abs(got.view(np.float32).astype(np.float64) - want["ss64"]) / want["ss64"]
            assert rel.max() < 1e-6, (what, rel.max())
            ct_split, ss_split = residual_split(b["y"], rows, dim)
            assert np.array_equal(ss_split, got), what
            assert np.array_equal(ct_split, want["y_ct"]), what
            want["y_ss"] = got
        for k, v in b.items():
            v.check(want.get(k), what)


# ---------------------------------------------------------------------------------------------------- one writer
def refill_state(rng, rows, batch, done, slot_seg):
    return {"done": Buf(rng, done.astype(np.int32), "done"), "slot_seg": Buf(rng, slot_seg.astype(np.int32), "slot_seg"),
            "slot_row": Buf(rng, rng.permutation(batch)[:rows].astype(np.int32), "slot_row"),
            "step": Buf(rng, bits(rng, np.int32, rows), "step"), "cur_tok": Buf(rng, bits(rng, np.int32, rows), "cur_tok")}


def cross_bufs(rng, src_batch, dst_batch, row_bytes, sc_bytes, scales):
    """2 layers of staging chunks and caches; scale rows for layer 1 only (or none)"""
    b = {"src": [Buf(rng, bits(rng, np.uint8, (2, src_batch, row_bytes)), "src%d" % l, row_bytes) for l in (0, 1)],
         "dst": [Buf(rng, bits(rng, np.uint8, (2, dst_batch, row_bytes)), "dst%d" % l, row_bytes) for l in (0, 1)],
         "src_sc": [None, Buf(rng, bits(rng, np.uint8, (src_batch, sc_bytes)), "src_sc1") if scales else None],
         "dst_sc": [None, Buf(rng, bits(rng, np.uint8, (dst_batch, sc_bytes)), "dst_sc1") if scales else None]}
    return b


def cross_view(c, src_batch, src_entry0, dst_batch, row_bytes, sc_bytes, keep):
    arr = lambda bs: (C.c_void_p * 2)(*[ptr(b) for b in bs])
    a = [arr(c["src"]), arr(c["dst"]), arr(c["src_sc"]), arr(c["dst_sc"])]
    keep.extend(a)
    return _lib.StagedCrossView(n_layers=2, src_batch=src_batch, src_entry0=src_entry0, dst_batch=dst_batch,
                                row_bytes=row_bytes, sc_bytes=sc_bytes, src=a[0], dst=a[1], src_sc=a[2], dst_sc=a[3])


def run_refill(rng, rows, stride, n_new, done, slot_seg, len_vals, dim, q_n, form, beam, cross, what):
    """one mt3_op_slot_refill against the reference; returns the Bufs' expected owned rows"""
    batch, n_segs, first_seg, beam_rows = rows + 7, 2 * rows + 5, rows + 5, rows + 3
    src_batch, entry0, row_bytes, sc_bytes, cbufs = cross
    b = refill_state(rng, rows, batch, done, slot_seg)
    b.update(row_bufs(rng, rows, dim, q_n, form))
    b["n_done"] = Buf(rng, np.array([int((done != 0).sum())], np.int32), "n_done")
    b["ids"] = Buf(rng, bits(rng, np.int32, (batch, stride)), "ids")
    b["out_ids"] = Buf(rng, bits(rng, np.int32, (n_segs, stride)), "out_ids")
    if beam:
        b["f"] = Buf(rng, bits(rng, np.uint32, beam_rows + rows), "f")
        b["len"] = Buf(rng, bits(rng, np.int32, rows), "len")
        b["len_row"] = Buf(rng, len_vals.astype(np.int32), "len_row")
    b.update(cbufs)
    s = owned(b)
    want, plan_ref = ref.refill(s, rows, n_new, first_seg, entry0, tables(dim, q_n)["bos"], beam_rows)
    plan, keep = np.full(rows + 1, -5, np.int32), []

    def call():
        x = cross_view(cbufs, src_batch, entry0, batch, row_bytes, sc_bytes, keep)
        return _lib.load().mt3_op_slot_refill(
            C.byref(state_view(b)), C.byref(row_view(b, dim, q_n, MAX_POS)), ptr(b.get("f")), beam_rows, ptr(b.get("len")),
            ptr(b.get("len_row")), b["ids"].ptr, stride, b["out_ids"].ptr, rows, n_new, first_seg, C.byref(x),
            plan.ctypes.data, None)

    run(b, want, call, what)
    assert np.array_equal(plan, plan_ref), what
    return want


def beam_state(rng, elems, k, L, num_steps, rot):
    """scripted search state of `elems` elements: finished with all k entries, with some entries unfilled, with nothing
    finished (short of / at num_steps), already handed over, and still decoding, in rotation from `rot`"""
    n, stride = elems * k, elems * k + 3
    done, seg, step = np.ones(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    fin_step, fin_beam = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    slot_row = np.zeros(n, np.int32)
    segs = rng.permutation(elems + 3)
    for e in range(elems):
        sl, kind = slice(e * k, (e + 1) * k), (e + rot) % 6
        slot_row[sl] = e * k + rng.permutation(k)
        seg[sl] = -1 if kind == 4 else segs[e]
        ran = num_steps if kind == 3 else int(rng.integers(1, num_steps)) if kind == 2 else int(rng.integers(1, num_steps + 1))
        step[sl] = ran
        filled = k if kind in (0, 4) else int(rng.integers(1, k + 1)) if kind == 1 else 0
        fin_step[e * k:e * k + filled] = rng.integers(0, ran, filled)
        fin_beam[e * k:e * k + filled] = rng.integers(0, k, filled)
        if kind == 5:
            done[sl] = 0
    if elems > 1 and k > 1:                                               # an entry whose EOS is the last position run
        fin_step[np.flatnonzero(fin_step >= 0)[-1]] = step[np.flatnonzero(fin_step >= 0)[-1]] - 1
    hist_tok = rng.integers(0, 2048, (L, stride)).astype(np.int32)
    hist_par = rng.integers(0, k, (L, stride)).astype(np.int32)
    hist_tok[0], hist_par[0] = 2047, k - 1                                 # every walk ends on (2047, k - 1): 14 bits
    b = {"done": Buf(rng, done, "done"), "slot_seg": Buf(rng, seg, "slot_seg"), "slot_row": Buf(rng, slot_row, "slot_row"),
         "step": Buf(rng, step, "step"), "cur_tok": Buf(rng, bits(rng, np.int32, n), "cur_tok"),
         "n_done": Buf(rng, np.array([int(done.sum())], np.int32), "n_done"),
         "live": Buf(rng, bits(rng, np.uint32, n), "live"), "fin_score": Buf(rng, bits(rng, np.uint32, n), "fin_score"),
         "fin_step": Buf(rng, fin_step, "fin_step"), "fin_beam": Buf(rng, fin_beam, "fin_beam"),
         "fork_src": Buf(rng, bits(rng, np.int32, n), "fork_src"),
         "hist_tok": Buf(rng, hist_tok, "hist_tok"), "hist_par": Buf(rng, hist_par, "hist_par")}
    return b


def run_beam_refill(rng, b, elems, k, L, num_steps, n_new, with_all, dim, q_n, form, cross, decodes, what):
    n, n_segs, first_seg = elems * k, 2 * elems + 3, elems + 3
    src_batch, entry0, row_bytes, sc_bytes, cbufs = cross
    dst_batch = n + 5
    b = dict(b)
    b.update(row_bufs(rng, n, dim, q_n, form))
    b["out_ids"] = Buf(rng, bits(rng, np.int32, (n_segs, L)), "out_ids")
    if with_all:
        b["out_all"] = Buf(rng, bits(rng, np.int32, (n_segs, k, L)), "out_all")
        b["out_scores"] = Buf(rng, bits(rng, np.uint32, (n_segs, k)), "out_scores")
    b.update(cbufs)
    s = owned(b)
    want, plan_ref = ref.beam_refill(s, elems, k, L, num_steps, n_new, first_seg, entry0, tables(dim, q_n)["bos"], decodes)
    plan, keep = np.full(elems + 1, -5, np.int32), []

    def call():
        x = cross_view(cbufs, src_batch, entry0, dst_batch, row_bytes, sc_bytes, keep)
        bk = _lib.BeamKView(k=k, elems=elems, vocab=2048, hist_stride=n + 3, live=b["live"].ptr, fin_score=b["fin_score"].ptr,
                            fin_step=b["fin_step"].ptr, fin_beam=b["fin_beam"].ptr, hist_par=b["hist_par"].ptr,
                            hist_tok=b["hist_tok"].ptr, fork_src=b["fork_src"].ptr)
        return _lib.load().mt3_op_beam_refill(
            C.byref(bk), C.byref(state_view(b)), C.byref(row_view(b, dim, q_n, MAX_POS)), L, num_steps, b["out_ids"].ptr,
            ptr(b.get("out_all")), ptr(b.get("out_scores")), n_new, first_seg, C.byref(x), plan.ctypes.data, None)

    run(b, want, call, what)
    assert np.array_equal(plan, plan_ref), what
    return want


@pytest.mark.parametrize("dim,q_n", [(16, 4), (528, 516), (768, 2048)])
def test_one_writer_of_the_bos_row(dim, q_n):
    """embed_kernel (128 threads), a restarted slot of refill_slot_kernel (128 threads) and each of the k slots of a
    restarted element of beam_refill_elem_kernel (256 threads) leave the same bits in all four forms -- and they are the
    bits slot_moves_ref.bos_row states (y_ss in exact rational arithmetic)"""
    rng = np.random.default_rng(dim)
    form, t = FORMS[2], tables(dim, q_n)
    b = row_bufs(rng, 3, dim, q_n, form)
    b["tok"], b["t"] = Buf(rng, np.zeros(3, np.int32), "tok"), Buf(rng, np.zeros(3, np.int32), "t")
    bos = {k: np.broadcast_to(v, (3,) + v.shape) for k, v in t["bos"].items()}
    run(b, bos, lambda: _lib.load().mt3_op_embed_rows(C.byref(row_view(b, dim, q_n, MAX_POS)), b["tok"].ptr, b["t"].ptr, 3,
                                                      None), "embed")
    cross = (6, 1, 16, 16, cross_bufs(rng, 6, 3 + 7, 16, 16, False))
    want = run_refill(rng, 3, 5, 3, np.ones(3), np.full(3, -1), None, dim, q_n, form, False, cross, "refill")
    for k in bos:
        assert np.array_equal(want[k], bos[k]), k          # (of the SCRIPT, not the kernel: all three slots restarted)
    for k_beams in (1, 3, 8):
        n = 2 * k_beams
        st = beam_state(rng, 2, k_beams, 8, 8, 0)
        cross = (6, 1, 16, 16, cross_bufs(rng, 6, n + 5, 16, 16, False))
        want = run_beam_refill(rng, st, 2, k_beams, 8, 8, 2, False, dim, q_n, form, cross, None, "beam k %d" % k_beams)
        for k in bos:
            assert np.array_equal(want[k], np.broadcast_to(t["bos"][k], (n,) + t["bos"][k].shape)), (k, k_beams)


# ---------------------------------------------------------------------------------------------------- compact
def done_pattern(rng, name, rows):
    d = np.zeros(rows, np.int32)
    if name == "all":
        d[:] = 1
    elif name == "last_live":
        d[:-1] = 1
    elif name == "first_done":
        d[0] = 1
    elif name == "alternating":
        d[::2] = 1
    elif name == "random":
        d[:] = rng.random(rows) < 0.5
    return d * rng.integers(1, 1 << 30, rows, dtype=np.int32)              # "done" is any non-zero value


@pytest.mark.parametrize("pattern", ["none", "all", "last_live", "first_done", "alternating", "random"])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130, 200])
def test_slot_compact(rows, pattern):
    rng = np.random.default_rng(rows * 7 + len(pattern))
    beam_rows = rows + 3
    variants = [(dim, q_n, form) for dim in (16, 528) for form in FORMS for q_n in (0, 4, 516)]
    for (dim, q_n, form), beam, seg in itertools.product(variants, (False, True), (False, True)):
        b = row_bufs(rng, rows, dim, q_n, form, with_tables=False)
        b["done"] = Buf(rng, done_pattern(rng, pattern, rows), "done")
        for k in ("slot_row", "step", "cur_tok") + (("slot_seg",) if seg else ()) + (("len",) if beam else ()):
            b[k] = Buf(rng, bits(rng, np.int32, rows), k)
        if beam:
            b["f"] = Buf(rng, bits(rng, np.uint32, beam_rows + rows), "f")
        want, perm_ref = ref.compact(owned(b), rows, beam_rows)
        perm = np.full(rows + 1, -5, np.int32)
        what = "rows %d %s dim %d q_n %d %s beam %d seg %d" % (rows, pattern, dim, q_n, "+".join(form), beam, seg)
        run(b, want, lambda: _lib.load().mt3_op_slot_compact(
            C.byref(state_view(b)), C.byref(row_view(b, dim, q_n)), ptr(b.get("f")), beam_rows, ptr(b.get("len")), rows,
            perm.ctypes.data, None), what)
        assert np.array_equal(perm, perm_ref), what
        if pattern == "none":               # (of the REFERENCE, not the kernel: the identity changes nothing but done -> 0)
            for k in b:
                if k != "done":
                    assert np.array_equal(want[k], b[k].owned()), (what, k)


# ---------------------------------------------------------------------------------------------------- refill
BIG_ROW8 = 8 * 256 * 16 + 16                   # one 16-byte piece past a full sweep of the refill's 8 parts
BIG_ROW16 = 16 * 256 * 16 + 16                 # ... of the beam refill's 16 parts
_cross_cache = {}


def shared_cross(key, src_batch, dst_batch, row_bytes, sc_bytes, scales):
    """the (large) staging chunks and caches of one shape, generated once: their host images never change"""
    k = (key, src_batch, dst_batch, row_bytes, sc_bytes, scales)
    if k not in _cross_cache:
        _cross_cache[k] = cross_bufs(np.random.default_rng(len(_cross_cache)), src_batch, dst_batch, row_bytes, sc_bytes, scales)
    return _cross_cache[k]


@pytest.mark.parametrize("stride", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("rows", [1, 65, 130])
def test_slot_refill(rows, stride):
    rng = np.random.default_rng(rows * 1000 + stride)
    batch, src_batch, entry0 = rows + 7, rows + 3, 2
    crosses = [(16, 16, False), (16, 2064, True), (BIG_ROW8, 16, True), (BIG_ROW8, 2064, False)]
    dones = [np.ones(1), np.zeros(1)] if rows == 1 else [(rng.random(rows) < 0.5).astype(np.int64)]
    run_no = 0
    for done in dones:
        if rows > 1:
            done[:2] = (1, 0)                                              # at least one finished and one live slot
        fin = int(done.sum())
        for n_new, (row_bytes, sc_bytes, scales) in itertools.product(sorted({0, fin // 2, fin, rows}), crosses):
            # segments: distinct; every third finished slot has been handed over already (-1)
            seg = rng.permutation(rows + 5)[:rows]
            handed = np.flatnonzero(done)[run_no % 3::3]
            seg[handed] = -1
            len_vals = np.array([-1, 0, stride - 1, stride])[rng.integers(0, 4, batch)]
            # drawn independently of the loops above, so that no form, size or beam state goes with one cross shape only
            dim, q_n = [(16, 4), (528, 516), (528, 0), (16, 516)][rng.integers(4)]
            form, beam = FORMS[rng.integers(3)], bool(rng.integers(2))
            cross = (src_batch, entry0, row_bytes, sc_bytes,
                     shared_cross("refill", src_batch, batch, row_bytes, sc_bytes, scales))
            what = "rows %d stride %d n_new %d/%d row_bytes %d sc %d/%d dim %d q_n %d %s beam %d" % (
                rows, stride, n_new, fin, row_bytes, sc_bytes, scales, dim, q_n, "+".join(form), beam)
            run_refill(rng, rows, stride, n_new, done, seg, len_vals, dim, q_n, form, beam, cross, what)
            run_no += 1


# ---------------------------------------------------------------------------------------------------- beam refill
BEAM_SHAPES = [(k, e, ln) for k in (1, 2, 3, 8) for e in (1, 5, 70) for ln in [(8, 8), (300, 257)] + ([(2048, 2048)] * (k == 8))]


@pytest.mark.parametrize("k,elems,ln", BEAM_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_beam_refill(k, elems, ln):
    """(2048, 2048) with k = 8 asks for exactly the 64 KB of dynamic LDS the launcher allows"""
    L, num_steps = ln
    rng = np.random.default_rng(k * 100000 + elems * 1000 + L)
    n, src_batch, entry0 = elems * k, elems + 3, 2
    for rot in {1: range(6), 5: (0, 3), 70: (0,)}[elems]:
        st = beam_state(rng, elems, k, L, num_steps, rot)
        s = owned(st)
        fin = np.flatnonzero(s["done"][::k] != 0)
        held = np.array([e for e in fin if s["slot_seg"][e * k] >= 0], np.int64)
        decodes = ref.beam_decodes(s, held, k, L, num_steps) if len(held) else None
        rows_bytes = (16, BIG_ROW16) if elems <= 5 else (16,)
        for n_new, with_all, row_bytes in itertools.product(sorted({0, len(fin) // 2, len(fin), elems}), (True, False),
                                                            rows_bytes):
            # drawn independently of the loops above (see test_slot_refill)
            sc_bytes, scales = (16, 2064)[rng.integers(2)], bool(rng.integers(2))
            dim, q_n = [(16, 4), (528, 516), (528, 0), (16, 516)][rng.integers(4)]
            form = FORMS[rng.integers(3)]
            cross = (src_batch, entry0, row_bytes, sc_bytes,
                     shared_cross("beam", src_batch, n + 5, row_bytes, sc_bytes, scales))
            what = "k %d elems %d L %d steps %d rot %d n_new %d/%d all %d row_bytes %d sc %d/%d dim %d q_n %d %s" % (
                k, elems, L, num_steps, rot, n_new, len(fin), with_all, row_bytes, sc_bytes, scales, dim, q_n, "+".join(form))
            run_beam_refill(rng, st, elems, k, L, num_steps, n_new, with_all, dim, q_n, form, cross, decodes, what)


# ---------------------------------------------------------------------------------------------------- stream init
@pytest.mark.parametrize("groups", [1, 2, 3, 4])
@pytest.mark.parametrize("slots", [1, 255, 256, 257, 600])
def test_beam_stream_init(slots, groups):
    rng = np.random.default_rng(slots * 8 + groups)
    b = {k: Buf(rng, bits(rng, np.int32, slots), k) for k in ("done", "slot_seg", "fork_src", "slot_row")}
    b["n_done"] = Buf(rng, bits(rng, np.int32, groups), "n_done")
    gs = rng.integers(1, 1 << 20, 4).astype(np.int32)
    want = ref.beam_stream_init(owned(b), slots, gs[:groups])
    run(b, want, lambda: _lib.load().mt3_op_beam_stream_init(b["done"].ptr, b["slot_seg"].ptr, b["fork_src"].ptr,
                                                             b["slot_row"].ptr, b["n_done"].ptr, slots, groups,
                                                             gs.ctypes.data, None), "slots %d groups %d" % (slots, groups))
