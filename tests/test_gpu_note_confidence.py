"""Note confidences end to end on the trained fixture: InferenceModel.transcribe_scored / transcribe_wav_scored return
the notes of __call__ plus, per note, the teacher-forced log-probability of the token that started it, of the token that
ended it, and the margin of the onset token to the model's best token -- and the command line writes them as JSON."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from mt3_amd import audio_io, checkpoints, inference, midi_io, synthetic, transcribe  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")


def _fields(ns):
    return [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum, n.instrument) for n in ns.notes]


@pytest.fixture(scope="module")
def wav():
    return synthetic.synth_music(3 * 2.048 + 0.5, seed=13, device="cpu")[1]


@pytest.fixture(scope="module")
def trained():
    return checkpoints.load_compact_npz(CKPT)


def _id_rows(m, audio):
    """the decoded id rows of `audio`, each up to and including its EOS: InferenceModel.score's targets"""
    _, x = m._examples(audio, 16000)
    rows = []
    for row in m._predict_ids({"encoder_input_tokens": x}).cpu().numpy():
        eos = np.flatnonzero(row == 1)
        rows.append(row[: int(eos[0]) + 1] if eos.size else row)
    return rows


@pytest.mark.parametrize("decoding", ["beam1", "greedy"])
def test_scored_transcription(wav, trained, decoding):
    m = inference.InferenceModel(trained, "mt3", dtype="float32", decoding=decoding)
    plain = m(wav)
    ns, sc = m.transcribe_scored(wav)
    n = len(ns.notes)
    assert n >= 5 and _fields(ns) == _fields(plain) and ns.total_time == plain.total_time
    assert set(sc) == {"onset_logprob", "end_logprob", "onset_margin", "note_tokens"}
    for k in ("onset_logprob", "end_logprob", "onset_margin"):
        assert sc[k].shape == (n,) and sc[k].dtype == np.float64
    tr = sc["note_tokens"]
    assert tr.shape == (n, 2, 2) and tr.dtype == np.int64 and np.all(tr[:, 0] >= 0)
    assert np.all(np.isfinite(sc["onset_logprob"])) and np.all(sc["onset_logprob"] <= 0)
    assert np.all(sc["onset_margin"] <= 0)
    assert np.array_equal(np.isnan(sc["end_logprob"]), tr[:, 1, 0] < 0)
    assert np.all(sc["end_logprob"][tr[:, 1, 0] >= 0] <= 0)

    # the same numbers through InferenceModel.score on the decoded rows, bit for bit after the float64 widening
    rows = _id_rows(m, wav)
    _, tok = m.score(wav, rows, return_token_scores=True)
    for j in range(n):
        (s0, p0), (s1, p1) = tr[j].tolist()
        assert sc["onset_logprob"][j] == tok[s0][p0], (j, s0, p0)
        if s1 >= 0:
            assert sc["end_logprob"][j] == tok[s1][p1], (j, s1, p1)

    if decoding == "greedy":
        # a greedy decode picks the arg-max of its step; wherever the teacher-forced prefill agrees with that pick, the
        # margin is exactly 0.  (The prefill and the cached step round differently, so a near-tie may flip: counted.)
        x_rows = np.zeros((len(rows), max(len(r) for r in rows)), np.int32)
        for i, r in enumerate(rows):
            x_rows[i, : len(r)] = r
        _, x = m._examples(wav, 16000)
        _, top_id, _ = m.model.score_segments(x, x_rows, return_top1=True)
        top_id = top_id.cpu().numpy()
        agree = np.array([top_id[s, p] == x_rows[s, p] for s, p in tr[:, 0].tolist()])
        print("greedy: the prefill's arg-max is the decoded onset token for %d of %d notes" % (agree.sum(), n))
        assert agree.sum() >= n // 2
        assert np.all(sc["onset_margin"][agree] == 0)


def test_wav_form_and_command_line(wav, trained, tmp_path):
    path = tmp_path / "tune.wav"
    path.write_bytes(audio_io.samples_to_wav_data(np.asarray(wav), 16000))
    m = inference.InferenceModel(trained, "mt3", dtype="float32")
    plain = m.transcribe_wav(str(path))
    ns, sc = m.transcribe_wav_scored(str(path))
    assert _fields(ns) == _fields(plain) and len(sc["onset_logprob"]) == len(ns.notes)

    # the command line: NAME.confidence.json beside NAME.mid, one record per note of the written MIDI
    del m
    assert transcribe.main(["--checkpoint", CKPT, "--confidences", str(path)]) == 0
    records = json.load(open(tmp_path / "tune.confidence.json"))
    midi = midi_io.midi_bytes_to_note_sequence((tmp_path / "tune.mid").read_bytes())
    assert len(records) == len(ns.notes) == len(midi.notes) >= 5
    for r, note, lp, mg, end in zip(records, ns.notes, sc["onset_logprob"], sc["onset_margin"], sc["end_logprob"]):
        assert (r["start_time"], r["end_time"], r["pitch"], r["velocity"]) == \
            (note.start_time, note.end_time, note.pitch, note.velocity)
        assert r["onset_logprob"] == lp and r["onset_margin"] == mg
        assert (r["end_logprob"] is None) if np.isnan(end) else (r["end_logprob"] == end)
