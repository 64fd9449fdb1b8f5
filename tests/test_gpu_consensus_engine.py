"""`InferenceModel.consensus` and `python -m mt3_amd.transcribe --consensus N` on the trained fixture: the consensus of the
model's own samples is `consensus.consensus` of `sample`'s output and the numpy reference's, the model is left as it was,
and the command writes a .mid and a .votes.json that hold the same notes."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mt3_amd import audio_io, checkpoints, consensus, inference, midi_io, synthetic, transcribe  # noqa: E402
from tests import consensus_ref as ref  # noqa: E402

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt3_synthetic_ckpt.npz")
TICK = 60.0 / (120.0 * 220)              # one MIDI tick of the writer in seconds: 220 per quarter at 120 per minute


@pytest.fixture(scope="module")
def audio():
    return synthetic.synth_music(2 * 2.048 - 0.1, seed=17, device="cpu")[1]          # two segments


@pytest.fixture(scope="module")
def model():
    return inference.InferenceModel(checkpoints.load_compact_npz(CKPT), "mt3", dtype="float32", temperature=1.0, seed=3)


def test_consensus_is_sample_then_vote(model, audio):
    was = (model.decoding, model.sampling)
    ns, record, samples = model.consensus(audio, num_samples=3, return_votes=True)
    assert (model.decoding, model.sampling) == was and model.decoding == "beam1"
    again = model.sample(audio, 3)
    assert samples == again and len(samples) == 3 and sum(len(s.notes) for s in samples) > 0
    ref.assert_same([record], consensus.consensus([again]))
    ref.assert_same([record], consensus.consensus_reference([again]))
    assert ns == record.notes and model.consensus(audio, num_samples=3) == ns
    assert record.n_voters == 3 and record.min_votes == 2 and len(record.votes) == len(ns.notes)
    assert all(2 <= v <= 3 for v in record.votes)
    assert [len(v) for v in record.note_votes] == [len(s.notes) for s in samples]
    assert all(1 <= v <= 3 for nv in record.note_votes for v in nv)
    loose = model.consensus(audio, num_samples=3, min_votes=1, return_votes=True)[1]
    assert all(1 <= v <= 3 for v in loose.votes) and len(loose.votes) >= len(record.votes)


def test_one_sample_is_its_own_consensus(model, audio):
    ns, record, samples = model.consensus(audio, num_samples=1, min_votes=1, return_votes=True)
    ref.assert_same([record], consensus.consensus_reference([[samples[0]]]))
    assert samples == model.sample(audio, 1) and list(record.votes) == [1] * len(ns.notes)


def test_a_beam_model_is_refused_in_samples_words(audio):
    m = inference.InferenceModel("random:0", "mt3", decoding="beam", num_beams=2,
                                 config=inference.network.T5Config(num_encoder_layers=1, num_decoder_layers=1))
    with pytest.raises(ValueError, match=r"sample\(\) draws on the greedy path"):
        m.consensus(audio, num_samples=2)
    with pytest.raises(ValueError, match="num_samples must be at least 1"):
        m.consensus(audio, num_samples=0)


def test_the_command_writes_the_notes_and_their_votes(audio, tmp_path):
    wav = tmp_path / "tune.wav"
    wav.write_bytes(audio_io.samples_to_wav_data(np.asarray(audio, np.float32), 16000))
    out = tmp_path / "out"
    os.makedirs(out)
    assert transcribe.main(["--checkpoint", CKPT, "--consensus", "3", "--consensus-min-votes", "2", "--seed", "3",
                            "-o", str(out / "tune.mid"), str(wav)]) == 0
    assert sorted(os.listdir(out)) == ["tune.mid", "tune.votes.json"]
    with open(out / "tune.votes.json") as f:
        votes = json.load(f)
    with open(out / "tune.mid", "rb") as f:
        ns = midi_io.midi_bytes_to_note_sequence(f.read())
    assert votes["n_voters"] == 3 and votes["min_votes"] == 2 and len(votes["notes"]) == len(ns.notes) > 0
    assert all(2 <= n["votes"] <= 3 and n["members"] >= n["votes"] for n in votes["notes"])
    # the same notes: the .mid holds them on its tick grid (a time moves by half a tick at most, and an end is at least
    # one tick after its start), the JSON as they are
    for field in ("start_time", "end_time"):
        a = sorted((n["pitch"], n["program"], n["is_drum"], n[field]) for n in votes["notes"])
        b = sorted((n.pitch, n.program, bool(n.is_drum), getattr(n, field)) for n in ns.notes)
        assert [x[:3] for x in a] == [x[:3] for x in b]
        assert max(abs(x[3] - y[3]) for x, y in zip(a, b)) <= 1.5 * TICK + 1e-9
    assert transcribe.main(["--checkpoint", CKPT, "--consensus", "2", "--decoding", "beam", "-o", str(out / "b.mid"),
                            str(wav)]) == 1
    assert sorted(os.listdir(out)) == ["tune.mid", "tune.votes.json"]
