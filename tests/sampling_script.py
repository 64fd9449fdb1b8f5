"""Scripted cases for sample_step_kernel (mt3_op_token_steps_sampled) and their CPU reference: the greedy driver's loop of
tests/grammar_ref.py with `mt3_amd.sampling.pick` at every free position.

The rows are drawn so that the restatement's own decisions are clear of f32 rounding: every logit is a multiple of 1/64
(two logits tie exactly or differ by 1/64 or more, so a top-k boundary is a tie the ids decide or a gap far above 1e-3 at
every scale and temperature used here), and a head of a few ids holds almost all of the softmax mass (so a top-p cut falls
between masses of a few percent).  What is left to chance -- the top-two gap of z + g, the distance of p from the masses
around the cut -- is settled by the DRAW: a case takes the first draw of its logits and seed, counting up from the one its
name gives, for which every pick of the reference meets MARGIN; the GPU is not asked.  MARGIN: the f32 error of x / T + g at |z| <= 50 is about
1e-5 (an ulp of 50 is 4e-6, the two logf add as much), the margins are 100 times that; a mass is a ratio of sums of up
to 2048 f32 exponentials, good to about 1e-6, the margin is 1e-4."""
import functools
import zlib

import numpy as np

from mt3_amd import sampling
from tests import grammar_ref as gr
from tests import grammar_script as gs

EOS = 1
PICK_MARGIN, BOUNDARY_MARGIN, MASS_MARGIN = 1e-3, 1e-3, 1e-4
MAX_DRAWS = 50
ROWS, STEPS = 5, 12


def reference(scaled, streams, params, prompts=None, g=None, masks=None, max_len=0):
    """ids [rows][T], done [T][rows] and the margins of every free pick, (row, t, margins), of the sampled greedy loop on
    the scaled logits [T][rows][V] (float64 or f32)"""
    T, B, V = scaled.shape
    ids, done, margins = np.zeros((B, T), np.int32), np.zeros((T, B), np.int32), []
    for b in range(B):
        P = list(prompts[b]) if prompts is not None and prompts[b] is not None else []
        mask = masks[b] if masks is not None else None
        state, over = (gr.initial(g) if g is not None else 0), False
        for t in range(T):
            if not over:
                if t < len(P):
                    tok = P[t]
                else:
                    tok, m = sampling.pick(scaled[t, b], t, int(streams[b]), params, gr._rule_vector(g, state, mask, V))
                    margins.append((b, t, m))
                ids[b, t] = tok
                if g is not None:
                    state = gr.advance(g, state, tok)
                over = (t >= len(P) and tok == EOS) or bool(max_len and t + 1 >= max_len)
            done[t, b] = over
    return ids, done, margins


def clear(margins):
    """every decision of every pick is at least its margin away from going the other way"""
    return all(m["pick"] >= PICK_MARGIN and m["boundary"] >= BOUNDARY_MARGIN and m["mass"] >= MASS_MARGIN
               for _, _, m in margins)


class Case:
    """5 rows x 12 steps of scripted logits at vocabulary V; mode: (name, dict of SamplingParams fields without the seed);
    scale: with d_ss row scales; tables: masks, a prompt, the toy grammar (V >= 70) and max_len together"""

    def __init__(self, V, mode, scale, tables):
        self.V, self.mode, self.scale, self.tables = V, mode, scale, tables
        self.name = "v%d_%s%s%s" % (V, mode[0], "_scale" if scale else "", "_tables" if tables else "")
        for self.draw in range(MAX_DRAWS):
            self._draw(np.random.default_rng(zlib.crc32(self.name.encode()) + self.draw))
            self.ids, self.done, self.margins = reference(self.scaled(), self.streams, self.params, self.prompts, self.g,
                                                          self.masks, self.max_len)
            if clear(self.margins):
                return
        raise AssertionError("%s: no draw in %d with every pick clear of the margins" % (self.name, MAX_DRAWS))

    def _draw(self, rng):
        V, scale, tables = self.V, self.scale, self.tables
        self.params = sampling.SamplingParams(seed=int(rng.integers(0, 1 << 63)), **self.mode[1])
        T, B = STEPS, ROWS
        x = np.round((rng.normal(0, 1.0, (T, B, V)) - 8.0) * 64) / 64
        for t in range(T):
            for b in range(B):
                head = rng.choice(V, int(rng.integers(3, min(30, V // 2))), replace=False)
                x[t, b, head] = 6.0 + np.round(rng.uniform(0, 3, head.size) * 64) / 64
                if rng.random() < 0.15:
                    x[t, b, EOS] = 7.5                   # now and then EOS is a likely pick: rows finish
                x[t, b, rng.choice(V, 4, replace=False)] = x[t, b].max()       # exact ties at the top, the ids decide
        self.logits = x.astype(np.float32)
        assert np.array_equal(self.logits.astype(np.float64), x)
        self.n_ss, self.dim, self.ss = 0, 0, None
        if scale:
            self.n_ss, self.dim = 32, 512
            self.ss = (rng.uniform(0.5, 2.0, (T, B, 1)) * self.dim * rng.dirichlet(np.ones(self.n_ss), (T, B))
                       ).astype(np.float32)
        # streams: not the row index, and past 2^32
        self.streams = (rng.integers(0, 1 << 62, B, dtype=np.uint64) | np.uint64(1 << 40)).astype(np.uint64)
        self.prompts, self.masks, self.g, self.max_len = None, None, None, 0
        if tables:
            self.max_len = 9
            if V >= 70:
                self.g = gs.toy_grammar(1)
                forbid = list(range(gs.PITCH0, gs.PITCH0 + 12, 2)) + list(range(gs.SHIFT0 + 1, 23, 2))
                self.prompts = [gs.PROMPT_SECTION, None, gs.PROMPT_TIE, None, None]
            else:
                forbid = list(range(2, V, 3))
                self.prompts = [[5, 9, 2], None, [7], None, None]
            m = gs._mask(V, forbid)
            self.masks = [m, None, m, m, None]

    def scaled(self):
        """the logits as the token rule reads them, float64 [T][rows][V]"""
        x = self.logits.astype(np.float64)
        if self.ss is None:
            return x
        return x * ((self.ss.astype(np.float64).sum(-1) / self.dim + 1e-6) ** -0.5)[..., None]


MODES = (("plain", dict(temperature=0.8)), ("k1", dict(temperature=1.3, top_k=1)), ("k5", dict(temperature=0.7, top_k=5)),
         ("k256", dict(temperature=1.5, top_k=256)), ("p30", dict(temperature=1.0, top_p=0.3)),
         ("p90", dict(temperature=1.2, top_p=0.9)))


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for V in (40, 300, 2048):
        for mode in MODES:
            for scale in (False, True):
                out.append(Case(V, mode, scale, False))
        for mode in (MODES[0], MODES[2], MODES[5]):
            out.append(Case(V, mode, V == 300, True))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)
