"""Temperature sampling with top-k / top-p as the engine draws it (mt3_engine_set_sampling; the rule: include/mt3_hip.h),
restated in numpy.  This is the CPU statement the tests hold the kernel to -- it is not a fallback: nothing in the package
decodes with it.

  philox_bits(seed, stream, t, id)   word 0 of Philox4x32-10, key (seed lo, seed hi), counter (stream lo, stream hi, t, id)
  gumbel(bits)                       u = ((bits >> 9) + 0.5) * 2^-23 (exact in f32), g = -log(-log(u)) in float64
  pick(logits, t, stream, params)    one free pick, in float64 after the f32-exact u, with its decision margins
                                     (seed=: the segment's own key where a per-segment seed table is set)

The kernel computes z = x / temperature, z + g and the softmax masses in f32; `pick` computes them in float64 and reports
how far every decision it took was from going the other way, so that a caller can compare ids only where the margin is
far above f32 rounding."""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

from . import _lib

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    """mt3_sampling: temperature > 0 and finite; top_k in 0 .. 256 (0: off); 0 <= top_p < 1 (0: off); not both on"""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 0.0
    seed: int = 0

    def check(self):
        t, p = np.float32(self.temperature), np.float32(self.top_p)
        if not (t > 0 and np.isfinite(t)):
            raise ValueError("temperature must be positive and finite, got %r" % (self.temperature,))
        if not 0 <= int(self.top_k) <= _lib.SAMPLING_MAX_TOP_K:
            raise ValueError("top_k must be in 0 .. %d, got %r" % (_lib.SAMPLING_MAX_TOP_K, self.top_k))
        if not (0 <= p < 1):
            raise ValueError("top_p must be in [0, 1), got %r" % (self.top_p,))
        if self.top_k > 0 and p > 0:
            raise ValueError("top_k and top_p must not both be on")
        if not 0 <= int(self.seed) < 1 << 64:
            raise ValueError("seed must fit 64 bits, got %r" % (self.seed,))
        return self

    def struct(self) -> "_lib.Sampling":
        return _lib.Sampling(float(self.temperature), int(self.top_k), float(self.top_p), int(self.seed))


def philox_bits(seed, stream, t, id):
    """uint32 word 0 of Philox4x32-10 for (broadcast) arrays of seeds, streams (both taken modulo 2^64), positions and
    token ids (both taken modulo 2^32)"""
    def u64(a):
        a = np.asarray(a)
        if a.dtype == object or a.dtype.kind not in "iu":
            return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in np.asarray(a, dtype=object).reshape(-1)],
                            dtype=np.uint64).reshape(a.shape)
        return a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)

    seed, stream, t, id = np.broadcast_arrays(u64(seed), u64(stream), u64(t), u64(id))
    k0, k1 = seed & _LO, seed >> _S32
    c0, c1, c2, c3 = stream & _LO, stream >> _S32, t & _LO, id & _LO
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0.astype(np.uint32)


def uniform(bits):
    """u = ((bits >> 9) + 0.5) * 2^-23 as float64: the value the f32 expression has exactly, never 0 or 1"""
    return ((np.asarray(bits, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(bits):
    """g = -log(-log(u)) in float64"""
    return -np.log(-np.log(uniform(bits)))


def pick(logits, t: int, stream: int, params: SamplingParams, allowed: Optional[np.ndarray] = None,
         seed: Optional[int] = None):
    """One free pick from a row of logits (as the token kernel reads them: after the row scale) at position t of the
    segment with noise stream `stream`; allowed: bool [vocab], what the mask and the grammar leave (None: everything);
    seed: the segment's own Philox key (mt3_engine_set_sampling_seeds; None: params.seed).
    Returns (token id, margins):
      'pick'      gap between the best and the second best z + g of the kept set (inf: one candidate kept)
      'boundary'  top_k: gap in z between the last kept candidate and the first one left out (inf: nothing left out, or
                  the two tie exactly in x, where the lower id decides on both sides)
      'mass'      top_p: distance of p from the nearer of the two cumulative masses around the cut (before and after the
                  last kept candidate)
      'kept'      the kept ids, best first
    A caller compares against the f32 kernel only where these are far above f32 rounding."""
    x32 = np.asarray(logits, dtype=np.float32).reshape(-1)
    x = x32.astype(np.float64)
    ok = x > -np.inf                                       # (NaN: no candidate either)
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool).reshape(-1)
    ids = np.nonzero(ok)[0]
    margins = {"pick": np.inf, "boundary": np.inf, "mass": np.inf, "kept": ids}
    if ids.size == 0:
        return 1, margins                                  # no candidate at all: the kernel ends the row with EOS
    T = float(np.float32(params.temperature))
    z = x[ids] / T
    order = np.argsort(-x[ids], kind="stable")             # larger first, lower id on ties (ids ascend)
    ids, z = ids[order], z[order]
    keep = ids.size
    if params.top_k > 0:
        keep = min(int(params.top_k), ids.size)
        if keep < ids.size and x32[ids[keep - 1]] != x32[ids[keep]]:
            margins["boundary"] = float(z[keep - 1] - z[keep])
    elif np.float32(params.top_p) > 0:
        p = float(np.float32(params.top_p))
        e = np.exp(z - z[0])
        cum = np.cumsum(e) / e.sum()
        keep = min(int(np.searchsorted(cum, p, side="left")) + 1, ids.size)       # the first prefix with mass >= p
        near = [abs(cum[keep - 1] - p)] + ([abs(p - cum[keep - 2])] if keep > 1 else [])
        margins["mass"] = float(min(near))
    ids, z = ids[:keep], z[:keep]
    margins["kept"] = ids
    s = z + gumbel(philox_bits(params.seed if seed is None else seed, stream, t, ids))
    best = np.lexsort((ids, -s))                           # larger first, lower id on ties
    if keep > 1:
        margins["pick"] = float(s[best[0]] - s[best[1]])
    return int(ids[best[0]]), margins
