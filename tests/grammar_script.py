"""Scripted cases for the GRAMMAR instantiations of the token-rule kernels (mt3_op_token_steps_grammar,
mt3_op_beam_search_grammar), drawn step by step against a float64 mirror exactly as tests/beam_script.py does it: the same
GAP, the same MAX_TRIES, hitting the cap is an assertion.  The difference: the mirror applies each beam's own allowed
vector (the grammar in the state of the beam's slot, the element's mask) before the log-softmax.

The vocabulary is a toy grammar laid out in the first ids (whatever V >= 70): shifts at ids 3 .. 22 with max_steps 15,
pitches 23 .. 34, velocities 35 .. 36, tie 37, programs 38 .. 45, drums 46 .. 50, the rest extra ids.  Every row is drawn
so that ids its beam's state disallows sit ABOVE the allowed ones (20 + U(0, 1), the device of
tests/test_gpu_token_mask_rules.py), so the grammar bites: the unconstrained reference on the same logits breaks the
grammar in every case, on at least half of its rows (tests/test_grammar_ref.py asserts both, on the CPU)."""
import functools
import zlib

import numpy as np
import torch

from tests import beam_script as bs
from tests import grammar_ref as gr
from tests import prompt_ref as pr
from tests.beam_search_ref import EOS

TIE, PITCH0, PROGRAM0, SHIFT0 = 37, 23, 38, 3


def toy_grammar(with_ties=1):
    return gr.grammar(shift_first=SHIFT0, shift_count=20, max_steps=15, tie_id=TIE, program_first=PROGRAM0, program_count=8,
                      pitch_first=PITCH0, pitch_count=12, with_ties=with_ties)


# the two prompts of the issue: a bare `tie`, and a program, pitch, `tie` section followed by a shift
PROMPT_TIE = [TIE]
PROMPT_SECTION = [PROGRAM0 + 2, PITCH0 + 5, TIE, SHIFT0 + 4]


class _Mirror(bs._Mirror):
    """beam_script._Mirror that also keeps the grammar state of each live beam's slot"""

    def __init__(self, k, num_steps, g):
        super().__init__(k, num_steps)
        self.g, self.state = g, [gr.initial(g)] * k

    def ruled(self, rows64, mask):
        x = np.array(rows64, np.float64)
        for j in range(self.k):
            x[j, ~gr._rule_vector(self.g, self.state[j], mask, x.shape[1])] = -np.inf
        return x

    def look(self, rows64, t, mask=None):
        x = self.ruled(rows64, mask)
        r = super().look(x, t)
        # the tokens and parents of the new live beams, as the mirror's own selection orders them
        lp = torch.log_softmax(torch.as_tensor(x), -1).numpy()
        V = lp.shape[-1]
        flat = (self.live[:, None] + lp).reshape(-1)
        nl = []
        for e in np.argsort(-flat, kind="stable")[:2 * self.k]:
            beam, token = divmod(int(e), V)
            if token != EOS and len(nl) < self.k:
                nl.append((beam, token))
        r["state"] = [gr.advance(self.g, self.state[b], tok) for b, tok in nl]
        r["gaps"] = [(d, s) for d, s in r["gaps"] if np.isfinite(d)]       # (-inf candidates past the allowed set)
        return r

    def take(self, r):
        super().take(r)
        self.state = r["state"]

    def force(self, tok):
        self.state = [gr.advance(self.g, s, tok) for s in self.state]


class GrammarCase(pr.PromptCase):
    """A prompt_ref.PromptCase under the toy grammar (and, with `masks`, one bool [V] mask or None per element)."""

    def __init__(self, name, k, V, elems, num_steps, prompts=None, masks=None, with_ties=1, **kw):
        self.g = toy_grammar(with_ties)
        self.masks = masks
        self._ref_g = None
        super().__init__(name, k, V, elems, num_steps, prompts or [None] * elems, **kw)

    def _build(self):
        k, V, T, n = self.k, self.V, self.num_steps, self.elems * self.k
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        self.logits = np.zeros((T, n, V), np.float32)
        self.ss = None
        if self.n_ss:
            self.ss = (rng.uniform(0.25, 4.0, (T, n, 1)) * self.dim * rng.dirichlet(np.ones(self.n_ss), (T, n))
                       ).astype(np.float32)
        mirrors = [_Mirror(k, T, self.g) for _ in range(self.elems)]
        self.max_tries, self.gaps = 0, []
        self.forks = np.zeros(self.elems, int)
        self.retired_at = np.full(self.elems, -1)
        for t in range(T):
            for b, m in enumerate(mirrors):
                rows = slice(b * k, (b + 1) * k)
                style = self.plan(b, t)
                mask = self.masks[b] if self.masks is not None else None
                inside = t < self.plen(b)
                idle = m.retired or bool(self.max_len and t >= self.max_len) or inside
                for tries in range(1, bs.MAX_TRIES + 1):
                    z = np.stack([bs._row(rng, V, k, style) for _ in range(k)])
                    for j in range(k):                 # what beam j's state (or the mask) disallows sits above the rest
                        bad = ~gr._rule_vector(self.g, m.state[j], mask, V)
                        z[j, bad] = 20.0 + rng.random(int(bad.sum()))
                    if self.ss is not None:            # the kernel multiplies by rs: store the rows divided by it
                        z = z / ((self.ss[t, rows].astype(np.float64).sum(-1) / self.dim + 1e-6) ** -0.5)[:, None]
                    self.logits[t, rows] = z.astype(np.float32)
                    if idle:
                        break                          # nobody decides anything on these rows
                    r = m.look(self.scaled(t)[rows], t, mask)
                    if bs.separated(r["gaps"], False):
                        break
                else:
                    raise AssertionError("%s: step %d of element %d not separated in %d draws" % (self.name, t, b, tries))
                if inside and not (m.retired or (self.max_len and t >= self.max_len)):
                    m.force(self.prompts[b][t])
                if idle:
                    continue
                self.max_tries = max(self.max_tries, tries)
                self.gaps += [(d, s, False) for d, s in r["gaps"]]
                m.take(r)
                if m.retired:
                    self.retired_at[b] = t
                elif not (self.max_len and t + 1 >= self.max_len):
                    self.forks[b] += r["forks"]        # a closed element's forks are never copied
        self.n_fin = np.array([len(m.fin) for m in mirrors])
        self.mirror_fin = [list(m.fin) for m in mirrors]

    @property
    def ref(self):
        """the reference WITH the grammar (and the masks) on these logits"""
        if self._ref_g is None:
            self._ref_g = gr.run_reference(self, self.g, self.masks)
        return self._ref_g

    @property
    def plain_ref(self):
        """the unconstrained reference (prompts only) on the same logits"""
        if self._ref is None:
            self._ref = pr.run_reference(self)
        return self._ref

    def broken_rows(self):
        """per element: the unconstrained reference's best decode is NOT accepted by the grammar"""
        best = self.plain_ref.decodes[:, -1]
        return np.array([not gr.accepts(self.g, best[b], self.plen(b)) for b in range(self.elems)])


def _mask(V, forbid):
    m = np.ones(V, bool)
    m[list(forbid)] = False
    return m


def _prompts(kind):
    return {"none": [None, None, None], "tie": [PROMPT_TIE, None, PROMPT_TIE],
            "section": [PROMPT_SECTION, PROMPT_TIE, None]}[kind]


@functools.lru_cache(maxsize=None)
def beam_cases():
    out = []
    for k in (1, 2, 8):
        out.append(GrammarCase("g_v70_k%d" % k, k, 70, 3, 14, _prompts("tie")))
        out.append(GrammarCase("g_v70_section_k%d" % k, k, 70, 3, 14, _prompts("section")))
        out.append(GrammarCase("g_v70_scale_k%d" % k, k, 70, 3, 12, _prompts("none"), n_ss=32))
        out.append(GrammarCase("g_v70_maxlen_k%d" % k, k, 70, 3, 16, _prompts("tie"), max_len=9,
                               plan=lambda b, t: "no_eos" if t >= 9 else "rand"))
        # a mask that intersects the grammar: half the pitches, half the programs and the odd shifts go
        forbid = list(range(PITCH0, PITCH0 + 12, 2)) + list(range(PROGRAM0, PROGRAM0 + 8, 2)) + list(range(SHIFT0 + 1, 23, 2))
        if k < 8:                                      # (the tie section then holds 12 ids: not enough for 2k = 16)
            out.append(GrammarCase("g_v70_mask_k%d" % k, k, 70, 3, 14, _prompts("tie"),
                                   masks=[_mask(70, forbid), None, _mask(70, forbid)]))
        out.append(GrammarCase("g_v2048_k%d" % k, k, 2048, 3, 12, _prompts("section")))
    out.append(GrammarCase("g_v70_noties_k2", 2, 70, 3, 12, _prompts("none"), with_ties=0))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def token_cases():
    out = []
    for V in (70, 2048, 2100):                         # 2100: the token kernel's element-loop path
        out.append(GrammarCase("gt_v%d" % V, 1, V, 3, 14, _prompts("tie")))
        out.append(GrammarCase("gt_v%d_section" % V, 1, V, 3, 14, _prompts("section")))
    out.append(GrammarCase("gt_scale", 1, 70, 3, 12, _prompts("none"), n_ss=32))
    out.append(GrammarCase("gt_scale_v2100", 1, 2100, 3, 12, _prompts("tie"), n_ss=32))
    out.append(GrammarCase("gt_maxlen", 1, 70, 3, 16, _prompts("section"), max_len=9,
                           plan=lambda b, t: "no_eos" if t >= 9 else "rand"))
    forbid = list(range(PITCH0, PITCH0 + 12, 2)) + list(range(SHIFT0 + 1, 23, 2))
    for V in (70, 2100):
        out.append(GrammarCase("gt_mask_v%d" % V, 1, V, 3, 14, _prompts("tie"),
                               masks=[_mask(V, forbid), None, _mask(V, forbid)]))
    out.append(GrammarCase("gt_noties", 1, 70, 3, 12, _prompts("none"), with_ties=0))
    return tuple(out)


def mask_words(masks, V):
    """bool masks [n][V] (None entries: unconstrained) -> (uint32 [m][ceil(V / 32)], int32 index per element, -1: none)"""
    rows, index = [], []
    for m in masks:
        if m is None:
            index.append(-1)
            continue
        w = np.zeros((V + 31) // 32, np.uint32)
        for i in np.nonzero(m)[0]:
            w[i >> 5] |= np.uint32(1 << (int(i) & 31))
        rows.append(w)
        index.append(len(rows) - 1)
    return np.stack(rows), np.array(index, np.int32)

