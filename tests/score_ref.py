"""CPU reference of teacher-forced scoring (t5x score_batch on Transformer.decode(decode=False), mt3/network.py:303-361)
recomposed from the oracle's pieces, with t5x's decoder masks [from memory: t5x is not at hand]:
make_decoder_mask(decoder_target_tokens) = causal AND key target > 0 AND query target > 0 (network.py:333-340); the
encoder-decoder mask only masks queries whose target is 0.  The log-softmax / gather / weights run in float64."""
from __future__ import annotations

import numpy as np
import torch

from oracle import network as ON


def shift_right(targets: np.ndarray) -> np.ndarray:
    t = np.asarray(targets, np.int64)
    out = np.zeros_like(t)
    out[:, 1:] = t[:, :-1]
    return out


@torch.no_grad()
def teacher_forced_logits(orc: ON.Oracle, encoded: torch.Tensor, targets, decoder_inputs=None, masked: bool = True):
    """logits [B, L, V] of the full-sequence decoder pass.  masked=False: the plain causal pass (Oracle.decode_logits)."""
    p, cfg = orc.p, orc.cfg
    tgt = torch.as_tensor(np.asarray(targets, np.int64))
    din = torch.as_tensor(shift_right(targets) if decoder_inputs is None else np.asarray(decoder_inputs, np.int64))
    B, L = tgt.shape
    y = p["decoder/token_embedder/embedding"][din] + orc.pe[:L]
    visible = torch.ones((L, L), dtype=torch.bool).tril()[None].repeat(B, 1, 1)
    cross_visible = torch.ones((B, L, encoded.shape[1]), dtype=torch.bool)
    if masked:
        valid = tgt > 0
        visible &= valid[:, None, :] & valid[:, :, None]
        cross_visible &= valid[:, :, None]
    neg = torch.tensor(-1e10, dtype=orc.dtype)
    zero = torch.tensor(0.0, dtype=orc.dtype)
    self_bias = torch.where(visible, zero, neg)[:, None]
    cross_bias = torch.where(cross_visible, zero, neg)[:, None]
    enc = encoded.to(orc.dtype)
    for i in range(cfg.num_decoder_layers):
        Lp = f"decoder/layers_{i}"
        h = ON.rms_norm(y, p[Lp + "/pre_self_attention_layer_norm/scale"])
        y = y + orc._mha(Lp + "/self_attention", h, h, self_bias)
        h = ON.rms_norm(y, p[Lp + "/pre_cross_attention_layer_norm/scale"])
        y = y + orc._mha(Lp + "/encoder_decoder_attention", h, enc, cross_bias)
        h = ON.rms_norm(y, p[Lp + "/pre_mlp_layer_norm/scale"])
        y = y + orc._mlp(Lp + "/mlp", h)
    y = ON.rms_norm(y, p["decoder/decoder_norm/scale"])
    return y @ p["decoder/logits_dense/kernel"]


def scores_from_logits(logits, targets, weights=None):
    """(token_scores [B, L], sequence_scores [B]) in float64; positions whose target is 0 score 0."""
    lg = torch.as_tensor(np.asarray(logits)).double()
    tgt = torch.as_tensor(np.asarray(targets, np.int64))
    lp = torch.log_softmax(lg, -1).gather(-1, tgt[..., None])[..., 0]
    w = torch.ones_like(lp) if weights is None else torch.as_tensor(np.asarray(weights, np.float64))
    tok = torch.where(tgt > 0, lp * w, torch.zeros_like(lp))
    return tok.numpy(), tok.sum(-1).numpy()
