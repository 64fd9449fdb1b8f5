"""Plain-numpy statement of the launches that move per-slot decode state (mt3_amd/csrc/kernels.h: InputRow, CompactArgs,
RefillArgs, BeamRefillArgs, launch_beam_stream_init), one function per launch, written from the comments there and not
from the kernels.  Every function takes a dict of arrays (the slots a launch owns, payloads as raw-bit integer views),
leaves its arguments alone and returns the dict as the launch must leave it; keys that are absent or None are forms
the launch was not given.  tests/test_gpu_slot_moves.py compares the result bit for bit.

Array names: done, slot_row, slot_seg, step, cur_tok [slots] int32; n_done [1] int32; y [slots][dim] / y_ss
[slots][dim / 16] / q_out [slots][q_n] uint32; y_ct [slots][dim] uint16; f [beam_rows + slots] uint32 (two arrays beam_rows
apart); len [slots], len_row [batch] int32."""
from fractions import Fraction

import numpy as np

NEG_INF = np.float32(-1.0e7)                   # t5x decoding.NEG_INF
ROW_FORMS = ("y", "y_ct", "y_ss", "q_out")


def _copy(s):
    """the arrays a launch may write, copied (the staging chunks src / src_sc are inputs only and shared)"""
    return {k: (v if k.startswith("src") else [None if a is None else a.copy() for a in v] if isinstance(v, list) else
                v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def _has(s, k):
    return s.get(k) is not None


# ---------------------------------------------------------------------------------------------------- input rows
def bf16_rne(x):
    """f32 (finite) -> bf16 bits, round to nearest even"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _f32(fr):
    """the f32 nearest to an exact rational (ties to even)"""
    c = np.float32(float(fr))                  # within one f32 step: float() is correctly rounded to f64
    cand = sorted({c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))})
    err = [abs(Fraction(float(x)) - fr) for x in cand]
    best = [x for x, e in zip(cand, err) if e == min(err)]
    if len(best) > 1:
        best = [x for x in best if not (x.view(np.uint32) & 1)]
    return best[0]


def split_sums_f32(y):
    """y_ss of one f32 row in the order the comments on put_row_piece / put_input_row (decode_ops.hip) and quad_sum
    (device.h) state -- kernels.h only says WHAT y_ss holds, and bit-exact sums need the order -- exactly, in rational
    arithmetic rounded once per f32 operation: each 16-column group by one quad of threads, a thread's four columns x, y, z, w as
    fma(w, w, fma(z, z, fma(y, y, x * x))), the quad's four values t0 .. t3 as (t0 + t1) + (t2 + t3)."""
    v = [Fraction(float(x)) for x in np.asarray(y, np.float32)]
    out = np.zeros(len(v) // 16, np.float32)
    for g in range(len(v) // 16):
        t = []
        for q in range(4):
            x, yy, z, w = v[g * 16 + q * 4: g * 16 + q * 4 + 4]
            a = Fraction(float(_f32(x * x)))
            for c in (yy, z, w):
                a = Fraction(float(_f32(c * c + a)))
            t.append(a)
        lo, hi = Fraction(float(_f32(t[0] + t[1]))), Fraction(float(_f32(t[2] + t[3])))
        out[g] = _f32(lo + hi)
    return out


def embed(table, pos, max_pos, tok, t, ew=None, pw=None):
    """rows table[tok] + pos[min(t, max_pos - 1)] (one f32 add: exact), their bf16 copy, the float64 sums of squares of
    every 16-column group, and q = ew[tok] + pw[min(t, max_pos - 1)]"""
    tt = np.minimum(np.asarray(t), max_pos - 1)
    y = table[tok] + pos[tt]
    assert y.dtype == np.float32
    r = {"y": y.view(np.uint32), "y_ct": bf16_rne(y),
         "ss64": (y.astype(np.float64) ** 2).reshape(len(tt), -1, 16).sum(-1) if y.shape[1] % 16 == 0 else None}
    if ew is not None:
        r["q_out"] = (ew[tok] + pw[tt]).view(np.uint32)
    return r


def bos_row(table, pos, ew=None, pw=None):
    """the row of a restarted slot in its four forms: token 0 at position 0"""
    r = embed(table, pos, len(pos), np.zeros(1, np.int64), np.zeros(1, np.int64), ew, pw)
    out = {"y": r["y"][0], "y_ct": r["y_ct"][0], "y_ss": split_sums_f32(r["y"][0].view(np.float32)).view(np.uint32)}
    if ew is not None:
        out["q_out"] = r["q_out"][0]
    return out


def _put_bos(s, slot, bos):
    for k in ROW_FORMS:
        if _has(s, k):
            s[k][slot] = bos[k]


# ---------------------------------------------------------------------------------------------------- compaction
def compact(s, rows, beam_rows=0):
    """row retirement: the state of the i-th live slot lands in slot i; returns (state, perm [rows + 1])"""
    o = _copy(s)
    live = np.flatnonzero(s["done"][:rows] == 0)
    n = len(live)
    for k in ROW_FORMS + ("slot_row", "step", "cur_tok", "slot_seg", "len"):
        if _has(s, k):
            o[k][:n] = s[k][live]
    if _has(s, "f"):
        o["f"][:n] = s["f"][live]
        o["f"][beam_rows:beam_rows + n] = s["f"][beam_rows + live]
    o["done"][:n] = 0
    o["done"][n:rows] = 1
    if _has(s, "slot_seg"):
        o["slot_seg"][n:rows] = -1
    perm = np.full(rows + 1, -1, np.int32)
    perm[:n] = live
    perm[rows] = n
    return o, perm


# ---------------------------------------------------------------------------------------------------- refill
def _cross(o, s, entry, cache_rows):
    """staged entry `entry` of every layer -> each of cache_rows (K rows, V rows and, where staged, scale rows)"""
    for l in range(len(s["src"])):
        for r in cache_rows:
            o["dst"][l][:, r] = s["src"][l][:, entry]
            if s["src_sc"][l] is not None:
                o["dst_sc"][l][r] = s["src_sc"][l][entry]


def refill(s, rows, n_new, first_seg, src_entry0, bos, beam_rows=0):
    """in-flight batching, greedy and beam-1 (f / len / len_row present).  ids [batch][stride], out_ids [segs][stride];
    src / dst: per layer uint8 [2][batch][row_bytes]; src_sc / dst_sc: per layer uint8 [batch][sc_bytes] or None.
    Returns (state, plan [rows + 1])."""
    o = _copy(s)
    fin = np.flatnonzero(s["done"][:rows] != 0)
    beam = _has(s, "f")
    for i, slot in enumerate(fin):
        row, seg = s["slot_row"][slot], s["slot_seg"][slot]
        if seg >= 0:
            out = s["ids"][row].copy()
            n = s["len_row"][row] if beam else -1
            if n >= 0:                                     # the finished hypothesis: prefix, EOS, padding
                out[n:] = 0
                out[n:n + 1] = 1
            o["out_ids"][seg] = out
        if i >= n_new:
            o["slot_seg"][slot] = -1
            continue
        o["ids"][row] = 0
        o["slot_seg"][slot] = first_seg + i
        o["step"][slot] = o["cur_tok"][slot] = o["done"][slot] = 0
        if beam:
            o["f"][slot] = o["f"][beam_rows + slot] = 0     # +0.0f
            o["len"][slot] = o["len_row"][row] = -1
        _put_bos(o, slot, bos)
        _cross(o, s, src_entry0 + i, [row])
    o["n_done"][0] = s["n_done"][0] - min(n_new, len(fin))
    plan = np.full(rows + 1, -1, np.int32)
    plan[:len(fin)] = fin
    plan[rows] = len(fin)
    return o, plan


def beam_decodes(s, elems, k, L, num_steps):
    """what beam_finalize_kernel states, for the elements `elems` at once: decodes [len(elems)][k][L] in increasing order
    of score and scores [len(elems)][k] (raw bits).  Result i is state entry k - 1 - i: with anything finished
    (fin_step[s0] >= 0) the finished entries (EOS at fin_step, the prefix of beam fin_beam walked back from the step
    before; an unfilled entry: an all-zero row, its stored score), else the live beams over the min(step, num_steps) steps
    the element ran."""
    elems = np.asarray(elems, np.int64)
    s0 = elems * k
    dec = np.zeros((len(elems), k, L), np.int32)
    scores = np.zeros((len(elems), k), np.uint32)
    any_fin = s["fin_step"][s0] >= 0
    ran = np.minimum(s["step"][s0], num_steps)
    ar = np.arange(len(elems))
    for i in range(k):
        e = k - 1 - i
        scores[:, i] = np.where(any_fin, s["fin_score"][s0 + e], s["live"][s0 + e])
        eos = np.where(any_fin, s["fin_step"][s0 + e], -1)
        m = eos >= 0
        dec[ar[m], i, eos[m]] = 1
        u0 = np.where(any_fin, eos - 1, ran - 1)           # first history row of the walk (-2: nothing to walk)
        j = np.where(any_fin, s["fin_beam"][s0 + e], e)
        for u in range(int(u0.max(initial=-1)), -1, -1):
            m = u <= u0
            col = s0[m] + j[m]
            dec[ar[m], i, u] = s["hist_tok"][u, col]
            j[m] = s["hist_par"][u, col]
    return dec, scores


def beam_refill(s, elems, k, L, num_steps, n_new, first_seg, src_entry0, bos, decodes=None):
    """in-flight batching of the k-beam search over `elems` elements of k slots.  live / fin_score [slots] uint32;
    fin_step, fin_beam, fork_src [slots]; hist_tok / hist_par [L][stride]; out_ids [segs][L]; out_all [segs][k][L] and
    out_scores [segs][k] uint32 (optional).  decodes: beam_decodes() of the finished elements that hold a segment, in
    ascending order, where the caller has them already.  Returns (state, plan [elems + 1])."""
    o = _copy(s)
    fin = np.flatnonzero(s["done"][:elems * k:k] != 0)
    held = np.array([b for b in fin if s["slot_seg"][b * k] >= 0], np.int64)
    if len(held):
        dec, scores = decodes if decodes is not None else beam_decodes(s, held, k, L, num_steps)
        segs = s["slot_seg"][held * k]
        o["out_ids"][segs] = dec[:, k - 1]
        if _has(s, "out_all"):
            o["out_all"][segs] = dec
        if _has(s, "out_scores"):
            o["out_scores"][segs] = scores
    for i, b in enumerate(fin):
        sl = slice(b * k, (b + 1) * k)
        if i >= n_new:
            o["slot_seg"][sl] = -1
            continue
        o["slot_seg"][sl] = first_seg + i
        o["live"][sl] = NEG_INF.view(np.uint32)
        o["live"][b * k] = 0
        o["fin_score"][sl] = NEG_INF.view(np.uint32)
        o["fin_step"][sl] = o["fin_beam"][sl] = o["fork_src"][sl] = -1
        o["step"][sl] = o["cur_tok"][sl] = o["done"][sl] = 0
        for slot in range(b * k, (b + 1) * k):
            _put_bos(o, slot, bos)
        _cross(o, s, src_entry0 + i, list(s["slot_row"][sl]))
    o["n_done"][0] = s["n_done"][0] - k * min(n_new, len(fin))
    plan = np.full(elems + 1, -1, np.int32)
    plan[:len(fin)] = fin
    plan[elems] = len(fin)
    return o, plan


def beam_stream_init(s, slots, group_slots):
    """start of a k-beam streaming job: every slot finished, without a segment, on its own cache row, no fork pending;
    n_done[g] = the slots of group g"""
    o = _copy(s)
    o["done"][:slots] = 1
    o["slot_seg"][:slots] = -1
    o["fork_src"][:slots] = -1
    o["slot_row"][:slots] = np.arange(slots)
    o["n_done"][:len(group_slots)] = group_slots
    return o
