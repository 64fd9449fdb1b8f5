"""Feature conversion of the model wrapper (mirror of mt3/models.py:24-118,
`ContinuousInputsEncDecFeatureConverter` with pack=False): every example's continuous
`inputs` [n, depth] are trimmed / zero-padded to `task_feature_lengths['inputs']` rows and the
decoder gets all-zero token rows of `task_feature_lengths['targets']` (at inference the targets are
the dummy empty array of preprocessors.add_dummy_targets).  The zero rows are added AFTER the
log-mel (0.0, not log(1e-5))."""
from __future__ import annotations

from typing import Any, Dict, Mapping, Sequence

import numpy as np


def convert_features(examples: Sequence[Mapping[str, np.ndarray]], task_feature_lengths: Mapping[str, int]
                     ) -> Dict[str, np.ndarray]:
    T, L = task_feature_lengths["inputs"], task_feature_lengths["targets"]
    depth = examples[0]["inputs"].shape[-1] if examples else 0
    enc = np.zeros((len(examples), T, depth), np.float32)
    tgt = np.zeros((len(examples), L), np.int32)
    for i, ex in enumerate(examples):
        x = np.asarray(ex["inputs"], np.float32)[:T]
        enc[i, : x.shape[0]] = x
        t = np.asarray(ex.get("targets", np.zeros((0,), np.int32)), np.int32)[:L]
        tgt[i, : t.shape[0]] = t
    dec_in = np.zeros_like(tgt)
    dec_in[:, 1:] = tgt[:, :-1]                            # seqio autoregressive_inputs: shift right, BOS = 0
    return {"encoder_input_tokens": enc, "decoder_target_tokens": tgt, "decoder_input_tokens": dec_in,
            "decoder_loss_weights": (tgt > 0).astype(np.int32)}


SCORE_KEYS = ("encoder_input_tokens", "decoder_target_tokens", "decoder_input_tokens", "decoder_loss_weights")


def score_batch(model, batch: Mapping[str, Any], return_intermediates: bool = False):
    """t5x EncoderDecoderModel.score_batch, which mt3/models.py:121-152 inherits [from memory]: the sum over length of
    log_softmax(logits)[target] * decoder_loss_weights, logits = Transformer.decode(decode=False) on the teacher-forced
    `decoder_input_tokens`.  `model`: a network.Transformer; `batch`: the dict convert_features returns (all four keys
    are used).  Segments are encoded and scored in chunks of the engine's max_batch.  Returns float32 [B] sequence
    scores, with return_intermediates also {"decoder": {"token_scores": (float32 [B, L],)}}."""
    import torch
    missing = [k for k in SCORE_KEYS if k not in batch]
    if missing:
        raise ValueError("score_batch needs the converter's keys; missing: %s" % ", ".join(missing))
    x = torch.as_tensor(np.asarray(batch["encoder_input_tokens"], np.float32))
    tgt = np.asarray(batch["decoder_target_tokens"], np.int32)
    din = np.asarray(batch["decoder_input_tokens"], np.int32)
    w = np.asarray(batch["decoder_loss_weights"], np.float32)
    if not (tgt.ndim == 2 and tgt.shape == din.shape == w.shape and x.shape[0] == tgt.shape[0]):
        raise ValueError("score_batch: decoder arrays must be [B, L] and match the encoder batch")
    scores, tokens = [], []
    step = model.max_batch
    for s in range(0, tgt.shape[0], step):
        e = min(s + step, tgt.shape[0])
        model.encode(x[s:e].cuda())
        seq, tok = model.score(tgt[s:e], din[s:e], w[s:e], return_token_scores=True)
        scores.append(seq.cpu().numpy())
        tokens.append(tok.cpu().numpy())
    seq = np.concatenate(scores) if scores else np.zeros((0,), np.float32)
    if return_intermediates:
        tok = np.concatenate(tokens) if tokens else np.zeros(tgt.shape, np.float32)
        return seq, {"decoder": {"token_scores": (tok,)}}
    return seq
