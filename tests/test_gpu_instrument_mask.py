"""Allowed instruments end to end on the trained fixture: `InferenceModel(..., programs=[p], drums=False)` returns only
non-drum notes of program p, and one in-flight job holds files with different instruments.

The fixture was trained on program 0 alone and never emits another program of its own accord, so the test gives a second
program, 33, a voice.  Its input embedding becomes program 0's (what follows a program token does not depend on which of
the two was taken) and its output column becomes program 0's plus EPS times the column of another token j, so that
logit[33] = logit[program 0] + EPS * logit[j] at every step.  j is chosen from the fixture's own teacher-forced logits of
the test audio: the token whose logit is positive at some of the steps that emit program 0 and negative at others, with
the widest margin, and which lifts program 33 above the decoded token at no other step.  Both programs then appear in
the UNCONSTRAINED transcription -- asserted before anything else, or the test proves nothing."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import checkpoints, inference, synthetic  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")


def _fields(ns):
    return [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum) for n in ns.notes]


EPS = 0.05


def _program_tokens():
    from mt3_amd import event_codec, vocabularies
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    return tuple(3 + codec.encode_event(event_codec.Event("program", p)) for p in (0, 33))


def _second_voice_token(m, audio):
    """the token j of the module docstring, from the unmodified fixture's greedy decode of `audio`"""
    t0, t33 = _program_tokens()
    _, x = m._examples(audio, 16000)
    ids = m._predict_ids({"encoder_input_tokens": x})
    h = ids.cpu().numpy()
    n = int(max(np.flatnonzero(r == 1)[0] if (r == 1).any() else len(r) - 1 for r in h)) + 1
    m.model.encode(x)
    _, logits = m.model.decode_forced(ids, num_steps=n)
    lg = logits.cpu().numpy().astype(np.float64)                   # [n, B, V]
    live = np.array([[not (h[b, :t] == 1).any() for b in range(h.shape[0])] for t in range(n)])
    at = live & (h[:, :n].T == t0)                                 # the steps that emit program 0
    assert at.sum() >= 2, "fewer than two program tokens in the decode"
    L, top = lg[at], lg.max(-1)                                    # L [points, V]
    margin = np.where((L > 0).any(0) & (L < 0).any(0), np.abs(L).min(0), -1.0)
    other = live & ~at
    lifted = lg[..., t0][..., None] + EPS * lg                      # what logit[33] would be, per candidate j
    margin[(lifted[other] > top[other][:, None] - 0.5).any(0)] = -1.0
    margin[[t0, t33]] = -1.0
    j = int(np.argmax(margin))
    assert EPS * margin[j] > 1e-3, "no token separates the program steps of this audio"
    return j


def _two_voices(trained, j):
    t0, t33 = _program_tokens()
    params = {k: np.array(v) for k, v in trained.items()}
    out, emb = params["decoder/logits_dense/kernel"], params["decoder/token_embedder/embedding"]
    out[:, t33] = out[:, t0] + EPS * out[:, j]
    emb[t33] = emb[t0]
    return params


@pytest.mark.skipif(not os.path.exists(CKPT), reason="the trained fixture is absent")
def test_allowed_instruments():
    a = synthetic.synth_music(3 * 2.048 - 0.3, seed=13, device="cpu")[1]
    b = synthetic.synth_music(2 * 2.048 - 0.3, seed=7, device="cpu")[1]
    trained = checkpoints.load_compact_npz(CKPT)
    m = inference.InferenceModel(trained, "mt3", dtype="float32", decoding="greedy")
    j = _second_voice_token(m, a)
    m = None
    m = inference.InferenceModel(_two_voices(trained, j), "mt3", dtype="float32", decoding="greedy")
    plain = m(a)
    programs = sorted({n.program for n in plain.notes if not n.is_drum},
                      key=lambda p: -sum(n.program == p and not n.is_drum for n in plain.notes))
    print("SECOND_VOICE token %d programs %s" % (j, programs))
    assert len(programs) >= 2, "the unconstrained model must emit two programs here, or the test proves nothing"
    p, q = programs[0], programs[1]
    only_p = m(a, programs=[p], drums=False)
    assert only_p.notes and all(n.program == p and not n.is_drum for n in only_p.notes)
    assert _fields(only_p) != _fields(plain)
    assert m.model.status(inference.network._lib.STATUS_TOKEN_MASKS) == 0       # cleared after the call
    assert _fields(m(a)) == _fields(plain)
    only_q = m(b, programs=[q], drums=False)
    assert all(n.program == q and not n.is_drum for n in only_q.notes)
    both = m.transcribe_many([a, b], programs=[[p], [q]], drums=False)
    assert _fields(both[0]) == _fields(only_p) and _fields(both[1]) == _fields(only_q)
    with pytest.raises(ValueError):
        m(a, programs=[128])
    assert m.model.status(inference.network._lib.STATUS_TOKEN_MASKS) == 0
