"""CPU reference of PROMPTED decoding (mt3_engine_set_prompts; the rule: include/mt3_hip.h) over scripted logits: what
tests/beam_search_ref.beam_search and tests/beam_script.Case do, with a forced token prefix per element.  [from memory:
t5x is not at hand, as for the beam search itself]

The rule on top of beam_search_ref's.  Element b has a prompt P_b (a sequence of ids in [2, V), or None); step t of the
element is inside the prompt when t < len(P_b):
- all k live beams take P_b[t]; the k live log-probs stay as they are (prompt tokens are not scored: [0, NEG_INF, ...]
  until the first free step, which therefore expands beam 0 only, as step 0 does without a prompt);
- no candidate enters the finished set, nothing forks (every beam is its own parent), the retirement test is skipped;
- from t = len(P_b) the rule is beam_search_ref's, an EOS candidate at step t scoring logp / bp(t + 1) with the ABSOLUTE
  length t + 1 and logp the sum over the free tokens only.
Greedy: ids[t] = P_b[t] inside the prompt, never finished there; then the first arg-max, 0 after EOS (`greedy`).

`PromptCase` extends beam_script.Case: the same rows and the same float64 mirror, but an element decides nothing inside
its prompt, so its rows there are drawn once and its mirror stays at the start state; every decision from the first free
step on is separated by GAP or is an exact tie, as in beam_script."""
import zlib

import numpy as np
import torch

from tests import beam_script as bs
from tests.beam_search_ref import EOS, NEG_INF, brevity_penalty


def beam_search(step, reorder, batch, k, num_steps, prompts=None, alpha=0.6, eos_id=EOS, on_step=None):
    """beam_search_ref.beam_search with `prompts`: a list of `batch` id sequences (None / empty: no prompt).  Same
    arguments, same results (decodes [batch, k, num_steps] in increasing order of score, scores, steps_run).  With
    on_step the finished set is reported too: on_step(t, live_lp, live_seq, index, retired, fin_score, fin_valid)."""
    prompts = [list(p) if p is not None else [] for p in (prompts or [None] * batch)]
    n = batch * k
    live_lp = np.full((batch, k), NEG_INF)
    live_lp[:, 0] = 0.0
    live_seq = np.zeros((batch, k, num_steps), np.int32)
    fin_score = np.full((batch, k), NEG_INF)
    fin_valid = np.zeros((batch, k), bool)
    fin_seq = np.zeros((batch, k, num_steps), np.int32)
    retired = np.zeros(batch, bool)
    tok = torch.zeros(n, dtype=torch.int64)
    bp_max = brevity_penalty(num_steps + 1, alpha)
    ran = 0
    for t in range(num_steps):
        if retired.all():
            break
        ran += 1
        logits = torch.as_tensor(step(tok, t))
        lp = torch.log_softmax(logits.double(), -1).numpy()
        V = lp.shape[-1]
        index = np.arange(n)
        new_tok = tok.numpy().copy()
        bp_t = brevity_penalty(t + 1, alpha)
        for b in range(batch):
            if retired[b]:
                continue
            if t < len(prompts[b]):                     # inside the prompt: the token is given, nothing else moves
                live_seq[b, :, t] = prompts[b][t]
                new_tok[b * k:(b + 1) * k] = prompts[b][t]
                continue
            flat = (live_lp[b][:, None] + lp[b * k:(b + 1) * k]).reshape(-1)
            top = np.argsort(-flat, kind="stable")[:2 * k]
            nf_score, nf_valid, nf_seq = [], [], []
            nl = []
            for e in top:
                beam, token = divmod(int(e), V)
                if token == eos_id:
                    seq = live_seq[b, beam].copy()
                    seq[t] = eos_id
                    nf_score.append(flat[e] / bp_t)
                    nf_valid.append(True)
                    nf_seq.append(seq)
                else:
                    nf_score.append(NEG_INF)
                    nf_valid.append(False)
                    nf_seq.append(np.zeros(num_steps, np.int32))
                    if len(nl) < k:
                        nl.append((flat[e], beam, token))
            scores = np.concatenate([fin_score[b], nf_score])
            valid = np.concatenate([fin_valid[b], nf_valid])
            seqs = np.concatenate([fin_seq[b], np.stack(nf_seq)])
            keep = np.argsort(-scores, kind="stable")[:k]
            fin_score[b], fin_valid[b], fin_seq[b] = scores[keep], valid[keep], seqs[keep]
            fin_seq[b][~fin_valid[b]] = 0
            old_seq = live_seq[b].copy()
            for j, (sc, beam, token) in enumerate(nl):
                live_lp[b, j] = sc
                live_seq[b, j] = old_seq[beam]
                live_seq[b, j, t] = token
                index[b * k + j] = b * k + beam
                new_tok[b * k + j] = token
            if fin_valid[b, k - 1] and fin_score[b, k - 1] > live_lp[b, 0] / bp_max:
                retired[b] = True
        if on_step is not None:
            on_step(t, live_lp, live_seq, index, retired, fin_score, fin_valid)
        reorder(torch.from_numpy(index))
        tok = torch.from_numpy(new_tok)
    decodes = np.zeros((batch, k, num_steps), np.int32)
    out_scores = np.zeros((batch, k))
    for b in range(batch):
        if fin_valid[b].any():
            decodes[b], out_scores[b] = fin_seq[b][::-1], fin_score[b][::-1]
        else:
            decodes[b], out_scores[b] = live_seq[b][::-1], live_lp[b][::-1]
    return decodes, out_scores, ran


def run_reference(case, logits=None):
    """beam_script.run_reference for a PromptCase (or a plain Case: no prompts), optionally on other logits of the same
    shape than the case's own.  With max_len the rows from step max_len on keep EOS out (as in beam_script), so the
    finished sets are those of step max_len - 1; an element still inside its prompt at max_len has nothing finished."""
    k, T = case.k, case.num_steps
    r = bs.Ref()
    r.live_lp, r.live_seq, r.index, r.retired, r.fin_score, r.fin_valid = [], [], [], [], [], []

    def on_step(t, live_lp, live_seq, index, retired, fin_score, fin_valid):
        for dst, src in ((r.live_lp, live_lp), (r.live_seq, live_seq), (r.index, index), (r.retired, retired),
                         (r.fin_score, fin_score), (r.fin_valid, fin_valid)):
            dst.append(src.copy())

    def scaled(t):
        if logits is None:
            return case.scaled(t)
        x = logits[t].astype(np.float64)
        if case.ss is not None:
            x = x * ((case.ss[t].astype(np.float64).sum(-1) / case.dim + 1e-6) ** -0.5)[:, None]
        return x

    decodes, scores, ran = beam_search(lambda tok, t: scaled(t), lambda index: None, case.elems, k, T,
                                       prompts=getattr(case, "prompts", None), on_step=on_step)
    M = case.max_len
    if M and M < T:
        ran = min(ran, M)
        for b in range(case.elems):
            if not r.fin_valid[M - 1][b].any():        # nothing finished: the live beams as step M - 1 left them
                decodes[b] = r.live_seq[M - 1][b][::-1]
                decodes[b][:, M:] = 0
                scores[b] = r.live_lp[M - 1][b][::-1]
        for x in (r.live_lp, r.live_seq, r.index, r.retired, r.fin_score, r.fin_valid):
            del x[M:]
        r.retired[M - 1][:] = True                     # closed
    r.decodes, r.scores, r.steps_run = decodes, scores, ran
    return r


def greedy(logits, prompts, max_len=0):
    """ids [rows][T] and done [T][rows] of prompted greedy decoding over logits [T][rows][V]: P[t] inside the prompt (no
    finish there but by max_len), then the first arg-max, 0 after EOS, closed at max_len."""
    T, B = logits.shape[0], logits.shape[1]
    ids, done = np.zeros((B, T), np.int32), np.zeros((T, B), np.int32)
    for b in range(B):
        P = list(prompts[b]) if prompts[b] is not None else []
        over = False
        for t in range(T):
            if not over:
                ids[b, t] = P[t] if t < len(P) else int(np.argmax(logits[t, b]))
                over = (t >= len(P) and ids[b, t] == EOS) or bool(max_len and t + 1 >= max_len)
            done[t, b] = over
    return ids, done


class PromptCase(bs.Case):
    """A beam_script.Case whose element b is prompted with prompts[b] (a list of ids in [2, V), or None).  Inside its
    prompt an element decides nothing: its rows are drawn once (whatever the plan's style: `eos_best` there is the
    "scripted logits would emit EOS inside the prompt" case) and its mirror stays at the start state."""

    def __init__(self, name, k, V, elems, num_steps, prompts, **kw):
        self.prompts = [list(p) if p is not None else None for p in prompts]
        assert len(self.prompts) == elems
        super().__init__(name, k, V, elems, num_steps, **kw)

    def plen(self, b):
        return len(self.prompts[b]) if self.prompts[b] is not None else 0

    def _build(self):
        k, V, T, n = self.k, self.V, self.num_steps, self.elems * self.k
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        self.logits = np.zeros((T, n, V), np.float32)
        self.ss = None
        if self.n_ss:
            self.ss = (rng.uniform(0.25, 4.0, (T, n, 1)) * self.dim * rng.dirichlet(np.ones(self.n_ss), (T, n))
                       ).astype(np.float32)
        mirrors = [bs._Mirror(k, T) for _ in range(self.elems)]
        self.max_tries, self.gaps = 0, []
        self.forks = np.zeros(self.elems, int)
        self.retired_at = np.full(self.elems, -1)
        for t in range(T):
            for b, m in enumerate(mirrors):
                rows = slice(b * k, (b + 1) * k)
                style = self.plan(b, t)
                idle = m.retired or bool(self.max_len and t >= self.max_len) or t < self.plen(b)
                for tries in range(1, bs.MAX_TRIES + 1):
                    z = np.stack([bs._row(rng, V, k, style) for _ in range(k)])
                    if self.ss is not None:            # the kernel multiplies by rs: store the rows divided by it
                        z = z / ((self.ss[t, rows].astype(np.float64).sum(-1) / self.dim + 1e-6) ** -0.5)[:, None]
                    self.logits[t, rows] = z.astype(np.float32)
                    if idle:
                        break                          # nobody decides anything on these rows
                    r = m.look(self.scaled(t)[rows], t)
                    if bs.separated(r["gaps"], False):
                        break
                else:
                    raise AssertionError("%s: step %d of element %d not separated in %d draws" % (self.name, t, b, tries))
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
        if self._ref is None:
            self._ref = run_reference(self)
        return self._ref


# the shapes the issue names: rows 5 / elems 3, 12 steps, vocab 96, prompt lengths none / 1 / 3 / 11 mixed in one launch
T = 12


def _prompt(rng, V, n):
    return [int(x) for x in rng.integers(2, V, n)]


def prompts_for(name, V, count):
    """prompts of lengths [None, 1, 3, 11, 3][:count] (count 3: [3, None, 11]) with random ids in [2, V)"""
    rng = np.random.default_rng(zlib.crc32(("prompts " + name).encode()))
    lens = [3, 0, 11] if count == 3 else [0, 1, 3, 11, 3][:count]
    return [_prompt(rng, V, n) if n else None for n in lens]


def _eos_inside(b, t):
    """EOS is the best token of every row, by a wide margin, at steps 1 and 2: inside the prompts of 3 and 11 tokens (no
    finish there), a real finish for a row without a prompt or with one token"""
    return "eos_best" if t in (1, 2) else "rand"


def beam_prompt_cases():
    out = []
    for k in (1, 2, 4, 8):
        out.append(PromptCase("p_k%d" % k, k, 96, 3, T, prompts_for("b%d" % k, 96, 3)))
        out.append(PromptCase("p_scale_k%d" % k, k, 96, 3, T, prompts_for("bs%d" % k, 96, 3), n_ss=32))
        out.append(PromptCase("p_eos_inside_k%d" % k, k, 96, 3, T, prompts_for("be%d" % k, 96, 3), plan=_eos_inside))
        # max_len 9 lies inside the 11-token prompt of element 2 and after the others'
        out.append(PromptCase("p_maxlen_k%d" % k, k, 96, 3, T, prompts_for("bm%d" % k, 96, 3), max_len=9,
                              plan=lambda b, t: "no_eos" if t >= 9 else "rand"))
    return out


def token_prompt_cases():
    out = []
    for V in (96, 2100):                               # 2100: the greedy kernel's element-loop path
        out.append(PromptCase("pt_v%d" % V, 1, V, 5, T, prompts_for("t%d" % V, V, 5)))
    out.append(PromptCase("pt_scale", 1, 96, 5, T, prompts_for("ts", 96, 5), n_ss=32))
    out.append(PromptCase("pt_eos_inside", 1, 96, 5, T, prompts_for("te", 96, 5), plan=_eos_inside))
    out.append(PromptCase("pt_maxlen", 1, 96, 5, T, prompts_for("tm", 96, 5), max_len=9,
                          plan=lambda b, t: "no_eos" if t >= 9 else "rand"))
    return out
