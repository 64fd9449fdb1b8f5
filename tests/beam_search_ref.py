"""CPU reference of k-beam search: t5x decoding.beam_search(alpha=0.6) with num_decodes = k, the rule
include/mt3_hip.h states for mt3_engine_decode_beams.  [from memory] -- t5x is not at hand here, as for the beam-1
emulation of SURVEY.md A.5; the engine and this reference implement the SAME written rule:

- start: the k live beams of an element have log-probs [0, NEG_INF, ...]; the k finished scores are NEG_INF (unfilled);
- candidates: log_softmax (float64 here) of each live beam's logits plus the beam's log-prob; the top 2k of the k*V
  candidates, ties to the lower flattened index beam*V + token (a stable sort, as lax.top_k);
- finished set: an EOS candidate scores logp / bp(t+1), bp(n) = ((5+n)/6)^alpha; the old k entries and the 2k new
  ones (non-EOS candidates count as NEG_INF) are merged and the k best kept, the lower index on ties;
- live set: the k best candidates that do not end in EOS;
- retirement: an element whose k-th best finished score beats its best live log-prob / bp(num_steps + 1) is final;
  the search stops when every element is final or after num_steps;
- result: an element with no finished entry returns its live beams and their log-probs, one with at least one its
  finished set (unfilled entries: NEG_INF and all-zero ids); the k decodes in increasing order of score.
"""
import numpy as np
import torch

NEG_INF = -1.0e7
EOS = 1


def brevity_penalty(n, alpha=0.6):
    return ((5.0 + n) / 6.0) ** alpha


def beam_search(step, reorder, batch, k, num_steps, alpha=0.6, eos_id=EOS, on_step=None):
    """step(tok [batch*k] int64 tensor, t) -> logits [batch*k, V]; reorder(index [batch*k]) makes row j of every
    per-row state (the self-attention cache) a copy of row index[j].  Returns (decodes [batch, k, num_steps] int32,
    scores [batch, k] float64, steps_run), decodes in increasing order of score.  on_step(t, live_lp, live_seq, index,
    retired), if given, sees the state each step leaves (the arrays are the search's own: copy what is kept)."""
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
            on_step(t, live_lp, live_seq, index, retired)
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


@torch.no_grad()
def oracle_beam_search(orc, encoded, k, num_steps, alpha=0.6):
    """beam_search over oracle.network.Oracle's cached decode step: the cache holds batch*k rows, beam j of element b
    in row b*k + j, reordered with index_select after every step."""
    cache = orc._init_cache(encoded.repeat_interleave(k, 0))

    def step(tok, t):
        return orc._step(cache, tok, t)

    def reorder(index):
        for c in cache:
            c["k"] = [x.index_select(0, index) for x in c["k"]]
            c["v"] = [x.index_select(0, index) for x in c["v"]]

    return beam_search(step, reorder, encoded.shape[0], k, num_steps, alpha)
