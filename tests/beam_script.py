"""Scripted logits for the token-rule kernels (mt3_op_beam_search_scripted, mt3_op_token_steps_scripted) and what
tests/beam_search_ref.beam_search makes of them.  No GPU is needed to build or to validate a case
(tests/test_beam_script.py); tests/test_gpu_token_rules.py runs every case through the kernels.

A case is a tensor of logits [num_steps][elems * k][V] (f32; row b*k + j of step t is what live beam j of element b sees
at step t), optionally with the partial sums of a LogitScale.  Random cases are drawn step by step, element by element,
against a float64 mirror of the reference's scores (`_Mirror`; test_beam_script.py asserts that it IS the reference's
state): a draw is accepted only if every decision of the step is SEPARATED, i.e. each of these gaps is >= GAP(s):
  - consecutive scores among the best 2k + 1 candidates and among the best k + 1 real finished entries,
  - |k-th finished - live[0] / bp(num_steps + 1)| once the k-th entry exists.
GAP(s) = 1e-4 + 1e-5 |s| is ten times the f32-vs-f64 score bound of tests/test_gpu_beam_search.py: an f32 running sum of
<= 24 log-probs with |s| <~ 60 plus the fast exp / log of the log-sum-exp stays under about 5e-5, so the kernel's f32
ordering cannot differ from the reference's.  A rejected draw is redrawn from the same generator (deterministic), at
most MAX_TRIES times -- hitting the cap is an assertion, not a skip.

Hand-built TIE cases hold exact ties -- exact in f32 and f64 alike, because they come only from equal logits inside a
row and from identical rows under equal parents: their gaps are 0 (decided by the documented rule: lower token id inside
a beam, lower beam across beams) or >= GAP.  An old finished entry that exactly equals a new one cannot be made exact in
both arithmetics (the old score was divided by another brevity penalty) and is left out."""
import functools
import zlib

import numpy as np
import torch

from tests.beam_search_ref import EOS, NEG_INF, beam_search, brevity_penalty

MAX_TRIES = 300
SCORE_TOL = (1e-5, 1e-6)              # |kernel - reference| <= a + b |s|: the bound of tests/test_gpu_beam_search.py


def GAP(s):
    return 1e-4 + 1e-5 * abs(s)


# ---------------------------------------------------------------------------------------------------- rows
def _row(rng, V, k, style):
    """One row of logits (float64, before the f32 cast): a ladder of 4k top values with spacing 0.05 (1 + U) shuffled
    over the vocabulary, a Gaussian tail at -6; style decides where EOS sits."""
    n = min(4 * k, V)
    ladder = -np.concatenate([[0.0], np.cumsum(0.05 * (1.0 + rng.random(n - 1)))])
    row = -6.0 + rng.standard_normal(V)
    ids = rng.permutation(V)[:n]
    row[ids] = ladder
    if style == "rand":                               # EOS lifted into the ladder in 35 % of the rows
        if rng.random() < 0.35 and EOS not in ids:
            j = ids[rng.integers(n)]
            row[EOS], row[j] = row[j], row[EOS]
    elif style == "no_eos":
        row[EOS] = -30.0
    elif style == "eos_top":                          # EOS is the row's best token, by a ladder step
        j = ids[0]
        row[EOS], row[j] = row[j], row[EOS]
    elif style == "eos_best":                         # ... by a wide margin: every beam's EOS beats every other candidate
        row[EOS] = 10.0
    elif style == "extreme":                          # +-80 and -1e4 in one row: exp underflows, nothing overflows
        a, b, c = rng.permutation(V)[:3]
        # (the low one jittered: 0 + (-80 - 80) and (-80 - 80) + 0 would tie exactly in the next step)
        row[a], row[b], row[c] = 80.0, -80.0 - rng.random(), -1.0e4
    else:
        raise ValueError(style)
    return row


def _tie_row(rng, V, k):
    """Case (a): the top 2k logits are all equal, EOS among them; what is left lies at least 0.5 below."""
    ids = [EOS] + [int(i) for i in rng.permutation(np.delete(np.arange(V), EOS))[:2 * k - 1]]
    row = -0.5 - np.concatenate([[0.0], np.cumsum(0.05 * (1.0 + rng.random(V - 1)))])[rng.permutation(V)]
    row[ids] = 0.0
    return row


# ---------------------------------------------------------------------------------------------------- mirror
class _Mirror:
    """The reference's scores of ONE element in float64, computed with the reference's own expressions: live log-probs,
    the real finished scores (best first) and the retirement flag.  `look` evaluates a step without taking it."""

    def __init__(self, k, num_steps):
        self.k, self.bp_max = k, brevity_penalty(num_steps + 1)
        self.live = np.full(k, NEG_INF)
        self.live[0] = 0.0
        self.fin = []
        self.retired = False

    def look(self, logits64, t):
        k = self.k
        lp = torch.log_softmax(torch.as_tensor(logits64).double(), -1).numpy()
        V = lp.shape[-1]
        flat = (self.live[:, None] + lp).reshape(-1)
        order = np.argsort(-flat, kind="stable")[:2 * k + 1]
        sc = flat[order]
        gaps = [(a - b, max(abs(a), abs(b))) for a, b in zip(sc[:-1], sc[1:])]
        bp_t = brevity_penalty(t + 1)
        new_fin, new_live, parents = [], [], []
        for e in order[:2 * k]:
            beam, token = divmod(int(e), V)
            if token == EOS:
                new_fin.append(flat[e] / bp_t)
            elif len(new_live) < k:
                new_live.append(flat[e])
                parents.append(beam)
        merged = sorted(self.fin + new_fin, reverse=True)
        top = merged[:k + 1]
        gaps += [(a - b, max(abs(a), abs(b))) for a, b in zip(top[:-1], top[1:])]
        fin = merged[:k]
        retired = False
        if len(fin) == k:
            bound = new_live[0] / self.bp_max
            gaps.append((abs(fin[-1] - bound), max(abs(fin[-1]), abs(bound))))
            retired = fin[-1] > bound
        return dict(gaps=gaps, live=np.array(new_live), fin=fin, retired=retired, n_eos=len(new_fin),
                    forks=k - len(set(parents)))

    def take(self, r):
        self.live, self.fin, self.retired = r["live"], r["fin"], r["retired"]


def separated(gaps, tie):
    return all(d >= GAP(s) or (tie and d == 0.0) for d, s in gaps)


# ---------------------------------------------------------------------------------------------------- cases
class Case:
    """name, k, V, elems, num_steps, max_len (0: off), logits f32 [T][elems*k][V], ss f32 [T][elems*k][n_ss] or None,
    dim, tie (holds exact ties); after `build`: max_tries, gaps [(diff, |s|, step is a tie step)], per-element totals
    n_eos / forks / n_fin / retired_at, mirror_live [T][elems][k], and `ref` (lazily) the reference's results."""

    def __init__(self, name, k, V, elems, num_steps, plan=None, n_ss=0, max_len=0, tie=False):
        self.name, self.k, self.V, self.elems, self.num_steps = name, k, V, elems, num_steps
        self.n_ss, self.dim, self.max_len, self.tie = n_ss, 16 * n_ss if n_ss else 0, max_len, tie
        self.plan = plan or (lambda b, t: "rand")
        self._ref = None
        self._build()

    def scaled(self, t):
        """What the reference's step function returns for step t: float64, the LogitScale applied."""
        x = self.logits[t].astype(np.float64)
        if self.ss is not None:
            x = x * ((self.ss[t].astype(np.float64).sum(-1) / self.dim + 1e-6) ** -0.5)[:, None]
        return x

    def _build(self):
        k, V, T, n = self.k, self.V, self.num_steps, self.elems * self.k
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        self.logits = np.zeros((T, n, V), np.float32)
        self.ss = None
        if self.n_ss:                                  # mean square of the "residual row" in [0.25, 4]
            self.ss = (rng.uniform(0.25, 4.0, (T, n, 1)) * self.dim * rng.dirichlet(np.ones(self.n_ss), (T, n))
                       ).astype(np.float32)
        mirrors = [_Mirror(k, T) for _ in range(self.elems)]
        self.max_tries, self.gaps = 0, []
        self.n_eos, self.forks = np.zeros(self.elems, int), np.zeros(self.elems, int)
        self.retired_at = np.full(self.elems, -1)
        self.step_eos = np.zeros((T, self.elems), int)
        self.mirror_live = np.full((T, self.elems, k), np.nan)
        for t in range(T):
            for b, m in enumerate(mirrors):
                rows = slice(b * k, (b + 1) * k)
                style = self.plan(b, t)
                tie_step = style in ("tie_a", "same", "same_eos") or isinstance(style, tuple)
                for tries in range(1, MAX_TRIES + 1):
                    if isinstance(style, tuple):       # ("peaks", ids): the row's maximum at each of ids
                        z = np.stack([_peak_row(rng, V, style[1]) for _ in range(k)])
                    elif style == "tie_a":
                        z = np.stack([_tie_row(rng, V, k)] + [_row(rng, V, k, "rand") for _ in range(k - 1)])
                    elif tie_step:                     # k identical rows
                        z = np.repeat(_row(rng, V, k, "eos_top" if style == "same_eos" else "no_eos")[None], k, 0)
                    else:
                        z = np.stack([_row(rng, V, k, style) for _ in range(k)])
                    if self.ss is not None:            # the kernel multiplies by rs: store the rows divided by it
                        z = z / ((self.ss[t, rows].astype(np.float64).sum(-1) / self.dim + 1e-6) ** -0.5)[:, None]
                    self.logits[t, rows] = z.astype(np.float32)
                    if m.retired or (self.max_len and t >= self.max_len):
                        break                          # nobody decides anything on these rows
                    r = m.look(self.scaled(t)[rows], t)
                    if separated(r["gaps"], self.tie):         # (equal finished entries stay equal in later steps)
                        break
                else:
                    raise AssertionError("%s: step %d of element %d not separated in %d draws" % (self.name, t, b, MAX_TRIES))
                if m.retired or (self.max_len and t >= self.max_len):
                    continue
                self.max_tries = max(self.max_tries, tries)
                self.gaps += [(d, s, tie_step) for d, s in r["gaps"]]
                m.take(r)
                self.n_eos[b] += r["n_eos"]
                self.step_eos[t, b] = r["n_eos"]
                self.mirror_live[t, b] = m.live
                if m.retired:
                    self.retired_at[b] = t
                elif not (self.max_len and t + 1 >= self.max_len):
                    self.forks[b] += r["forks"]        # a closed element's forks are never copied
        self.n_fin = np.array([len(m.fin) for m in mirrors])
        self.mirror_fin = [list(m.fin) for m in mirrors]

    @property
    def ref(self):
        """The reference on these logits, run once: decodes / scores / steps_run and the state after every step."""
        if self._ref is None:
            self._ref = run_reference(self)
        return self._ref


class Ref:
    pass


def run_reference(case):
    """beam_search over the case's logits.  With max_len the kernels close every element after max_len steps; the
    reference has no such switch, so the case's rows from step max_len on keep EOS out of every top 2k (style no_eos):
    the reference's finished sets are then those of step max_len - 1, and the live beams of that step come from on_step."""
    k, T = case.k, case.num_steps
    r = Ref()
    r.live_lp, r.live_seq, r.index, r.retired = [], [], [], []

    def on_step(t, live_lp, live_seq, index, retired):
        r.live_lp.append(live_lp.copy())
        r.live_seq.append(live_seq.copy())
        r.index.append(index.copy())
        r.retired.append(retired.copy())

    decodes, scores, ran = beam_search(lambda tok, t: case.scaled(t), lambda index: None, case.elems, k, T, on_step=on_step)
    M = case.max_len
    if M and M < T:
        ran = min(ran, M)
        for b in range(case.elems):
            if case.n_fin[b] == 0:                     # nothing finished: the live beams as step M - 1 left them
                decodes[b] = r.live_seq[M - 1][b][::-1]
                decodes[b][:, M:] = 0
                scores[b] = r.live_lp[M - 1][b][::-1]
        for x in (r.live_lp, r.live_seq, r.index, r.retired):
            del x[M:]
        r.retired[M - 1][:] = True                     # closed
    r.decodes, r.scores, r.steps_run = decodes, scores, ran
    return r


V_EDGES = (63, 64, 65, 255, 256, 257, 1536, 1664, 2047, 2048)


def _early(b, t):
    """Element 0 sees EOS on top of every row from step 2 on and retires; element 1 takes a random walk; the last
    element never sees EOS among its candidates and returns its live beams."""
    return ("eos_best" if t >= 2 else "rand", "rand", "no_eos")[min(b, 2)]


@functools.lru_cache(maxsize=None)
def beam_cases():
    cases = []
    for k in range(1, 9):                              # the smallest vocabularies of every width
        cases.append(Case("v2k_k%d" % k, k, 2 * k, 3, 24 if k > 5 else 16))
        cases.append(Case("v2k1_k%d" % k, k, 2 * k + 1, 2, 16))
        cases.append(Case("retire_k%d" % k, k, 4 * k + 3, 3, 14, plan=_early))
    for i, V in enumerate(V_EDGES):                    # the lane-mapping edges, two widths each; every width twice or more
        for k in (i % 8 + 1, (i + 3) % 8 + 1, 8 if V in (64, 2047, 2048) else 0):
            if k:
                cases.append(Case("edge_v%d_k%d" % (V, k), k, V, 2, 12))
    cases.append(Case("table_v130_k7", 7, 130, 3, 24))
    cases.append(Case("table_v1536_k5", 5, 1536, 3, 16))
    cases.append(Case("table_v12_k6", 6, 12, 3, 24))
    cases.append(Case("four_elems_k3", 3, 65, 4, 12))
    for n_ss, k, V in ((1, 3, 64), (32, 8, 1536), (64, 5, 257), (32, 1, 2048), (64, 8, 16)):
        cases.append(Case("scale%d_v%d_k%d" % (n_ss, V, k), k, V, 2, 12, n_ss=n_ss))
    cases.append(Case("scale32_retire_k4", 4, 130, 3, 14, plan=_early, n_ss=32))
    # max_len < num_steps: from step max_len on the rows keep EOS out (run_reference)
    for k, V in ((1, 64), (4, 130), (8, 257)):
        cases.append(Case("maxlen_k%d" % k, k, V, 3, 16, max_len=9,
                          plan=lambda b, t: "no_eos" if t >= 9 or b == 2 else "rand"))
    # exact ties.  (a) step 0: 2k equal top logits, EOS among them; (b) then k identical rows: k-fold ties at every rank
    for k in (1, 2, 3, 5, 8):
        cases.append(Case("tie_ab_k%d" % k, k, 6 * k + 1, 2, 12, tie=True,
                          plan=lambda b, t: ("tie_a", "same")[t] if t < 2 else "rand"))
    cases.append(Case("tie_a_v2k_k4", 4, 8, 2, 12, tie=True, plan=lambda b, t: "tie_a" if t == 0 else "rand"))
    # (c) equal live scores, identical rows whose best token is EOS: k equal new finished scores in one step
    for k in (2, 3, 8):
        cases.append(Case("tie_c_k%d" % k, k, 4 * k + 1, 2, 12, tie=True,
                          plan=lambda b, t: ("tie_a", "same_eos")[t] if t < 2 else "rand"))
    # (d) V = 2k, EOS the best token of every beam: the merged top 2k holds exactly k candidates that do not end in EOS
    for k in (2, 4, 8):
        cases.append(Case("eos_all_k%d" % k, k, 2 * k, 2, 12, plan=lambda b, t: "eos_best" if t in (1, 2) else "rand"))
    # (e) +-80 and -1e4 in one row
    cases.append(Case("extreme_k2", 2, 4, 2, 12, plan=lambda b, t: "extreme"))
    cases.append(Case("extreme_k3", 3, 7, 2, 12, plan=lambda b, t: "extreme" if t % 2 == 0 else "rand"))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


# ------------------------------------------------------------------------------------------- token steps (k = 1)
TOKEN_V = (2, 255, 256, 257, 1536, 2048, 2049, 2176, 4100)


def _peak_row(rng, V, ids):
    """A row whose maximum is attained at every one of `ids`; everything else lies at least 0.5 below."""
    row = -0.5 - np.concatenate([[0.0], np.cumsum(0.05 * (1.0 + rng.random(V - 1)))])[rng.permutation(V)]
    row[list(ids)] = 0.0
    return row


def _peaks(V):
    """Equal maxima at 0 / 255 / 256, at 2047 / 2048, at EOS and a neighbour ... wherever V has those indices."""
    groups = [g for g in ((0, 255, 256), (255, 256), (2047, 2048), (EOS, 0), (EOS, 5), (V - 2, V - 1), (2048, 4099))
              if max(g) < V]
    return lambda b, t: ("peaks", groups[(t + b) % len(groups)])


class TokenCase(Case):
    """A k = 1 case of any vocabulary (mt3_op_token_steps_scripted takes any), one row per element."""

    def __init__(self, name, V, rows, num_steps, **kw):
        super().__init__(name, 1, V, rows, num_steps, **kw)

    def greedy(self):
        """ids [rows][T] and done [T][rows] of greedy decoding: the first arg-max, 0 after EOS, closed at max_len."""
        T, B = self.num_steps, self.elems
        ids, done = np.zeros((B, T), np.int32), np.zeros((T, B), np.int32)
        for b in range(B):
            over = False
            for t in range(T):
                if not over:
                    ids[b, t] = int(np.argmax(self.logits[t, b]))          # np.argmax: the first maximum
                    over = ids[b, t] == EOS or bool(self.max_len and t + 1 >= self.max_len)
                done[t, b] = over
        return ids, done


@functools.lru_cache(maxsize=None)
def token_cases():
    cases = []
    for V in TOKEN_V:
        cases.append(TokenCase("tok_v%d" % V, V, 4, 12, plan=lambda b, t: "rand" if b < 3 else "no_eos"))
        if V >= 6:
            cases.append(TokenCase("tok_tie_v%d" % V, V, 4, 8, plan=_peaks(V), tie=True))
    for n_ss, V in ((1, 257), (32, 1536), (64, 2049), (32, 4100)):
        cases.append(TokenCase("tok_scale%d_v%d" % (n_ss, V), V, 3, 12, n_ss=n_ss))
    for V in (256, 2176):
        cases.append(TokenCase("tok_maxlen_v%d" % V, V, 3, 14, max_len=8,
                               plan=lambda b, t: "no_eos" if t >= 8 or b == 2 else "rand"))
    return tuple(cases)
