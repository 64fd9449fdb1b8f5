"""The job-level note scores against the single-pair host functions: the quotients are of the same integers, so every
value is compared with ==.  Then `transcription_metrics`' keys and per-track values, and `--score-against`."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mt3_amd import audio_io, metrics, midi_io, synthetic, transcribe  # noqa: E402
from mt3_amd.note_sequences import Note, NoteSequence, TrackSpec, extract_track  # noqa: E402
from tests import note_matching_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz")
GRANULARITIES = ("flat", "midi_class", "full")


def _pair(rng, n):
    """a reference with three programs (two of one MIDI class) and drums, and an estimate made from it: notes dropped,
    times jittered, programs and pitches sometimes changed, notes added, some of zero length"""
    programs = np.array([0, 1, 33])
    ref, est = [], []
    on = np.sort(rng.uniform(0.0, 0.05 * n, n))
    for t in on:
        drum = rng.random() < 0.2
        note = Note(float(t), float(t + rng.uniform(0.05, 0.5)), int(rng.integers(36, 48) if drum else rng.integers(60, 66)),
                    int(rng.integers(20, 127)), 0 if drum else int(rng.choice(programs)), bool(drum), 9 if drum else 0)
        ref.append(note)
        if rng.random() < 0.15:
            continue
        start = max(0.0, note.start_time + rng.normal(0.0, 0.03))
        end = max(start, note.end_time + rng.normal(0.0, 0.05)) if rng.random() > 0.05 else start      # some zero-length
        est.append(Note(float(start), float(end), note.pitch + int(rng.random() < 0.1), note.velocity,
                        note.program if drum or rng.random() > 0.1 else int(rng.choice(programs)), note.is_drum,
                        note.instrument))
    for t in rng.uniform(0.0, 0.05 * n, n // 6):
        est.append(Note(float(t), float(t + 0.2), int(rng.integers(60, 66)), 80, int(rng.choice(programs))))
    order = rng.permutation(len(est))
    return NoteSequence(notes=ref, total_time=float(on[-1] + 1.0)), NoteSequence(notes=[est[i] for i in order])


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.default_rng(11)
    out = [_pair(rng, n) for n in (120, 300, 40, 200)]
    # sides of ONLY zero-length notes: dropped before n_ref and n_est are counted, so everything scores zero
    zeros = NoteSequence(notes=[Note(a, b, p, 100, program) for a, b, p in cases.zero_length_sequences() for program in (0, 33)])
    out.append((zeros, out[2][1]))
    out.append((out[3][0], zeros))
    drums_only = NoteSequence(notes=[n for n in out[0][0].notes if n.is_drum])
    out.append((drums_only, out[0][1]))                    # a reference without a non-drum note
    out.append((out[1][0], NoteSequence()))                # an empty estimate
    assert len(out) == 8
    return out


def test_transcription_scores_many(pairs):
    for unit in ("note_number", "hz"):
        got = metrics.transcription_scores_many(pairs, pitch_unit=unit)
        want = [metrics.transcription_scores(r, e, pitch_unit=unit) for r, e in pairs]
        assert got == want
        assert 0.0 < want[0]["Onset + offset F1"] < want[0]["Onset F1"] < 1.0
        assert set(got[4].values()) == {0.0} == set(got[5].values())          # only zero-length notes on a side


def test_program_aware_note_scores_many(pairs):
    for g in GRANULARITIES:
        got = metrics.program_aware_note_scores_many(pairs, granularity_type=g)
        want = [metrics.program_aware_note_scores(r, e, granularity_type=g) for r, e in pairs]
        assert got == want
        assert 0.0 < want[0]["Drum onset F1 (%s)" % g] and 0.0 < want[0]["Nondrum onset + offset + program F1 (%s)" % g] < 1.0


def _host_sweep(ref_ns, est_ns, tolerances):
    ri, rp, _ = metrics.sequence_to_valued_intervals(ref_ns, drums=False)
    ei, ep, _ = metrics.sequence_to_valued_intervals(est_ns, drums=False)
    out = {}
    for tol in tolerances:
        p, r, f = metrics.precision_recall_f1_overlap(ri, rp, ei, ep, onset_tolerance=tol, offset_min_tolerance=tol)
        out["Onset + offset precision (%s)" % tol], out["Onset + offset recall (%s)" % tol] = p, r
        out["Onset + offset F1 (%s)" % tol] = f
    return out


def test_note_onset_tolerance_sweep_many(pairs):
    tolerances = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)
    got = metrics.note_onset_tolerance_sweep_many(pairs)
    assert got == [_host_sweep(r, e, tolerances) for r, e in pairs]
    assert list(got[0])[:3] == ["Onset + offset precision (0.01)", "Onset + offset recall (0.01)", "Onset + offset F1 (0.01)"]
    f1 = [got[0]["Onset + offset F1 (%s)" % t] for t in tolerances]
    assert f1 == sorted(f1) and f1[0] < f1[-1]             # a wider tolerance never matches fewer
    assert metrics.note_onset_tolerance_sweep_many(pairs[:2], tolerances=(0.03,)) == [_host_sweep(r, e, (0.03,))
                                                                                      for r, e in pairs[:2]]


def test_transcription_metrics(pairs):
    specs = [TrackSpec("Piano", 0), TrackSpec("Bass", 33), TrackSpec("Drums", 0, True)]
    got = metrics.transcription_metrics(pairs, track_specs=specs)
    names = ["Onset precision", "Onset recall", "Onset F1"]
    offs = ["Onset + offset precision", "Onset + offset recall", "Onset + offset F1"]
    frame = ["Frame Precision", "Frame Recall", "Frame F1"]
    want_keys = names + offs + frame
    for track in ("Piano", "Bass"):
        want_keys += [track + "/" + k for k in names + offs + frame]
    want_keys += ["Drums/" + k for k in names + frame]     # a drum track has no offsets
    for g in GRANULARITIES:
        for name in ("Onset + offset + program", "Drum onset", "Nondrum onset + offset + program"):
            want_keys += ["%s %s (%s)" % (name, what, g) for what in ("precision", "recall", "F1")]
    for tol in (0.01, 0.02, 0.05, 0.1, 0.2, 0.5):
        want_keys += ["Onset + offset %s (%s)" % (what, tol) for what in ("precision", "recall", "F1")]
    assert sorted(got["scores"]) == sorted(want_keys) == sorted(got["mean"])
    assert not any("velocity" in k for k in got["scores"])
    scores = got["scores"]
    assert all(len(v) == len(pairs) for v in scores.values())
    for k, (ref_ns, est_ns) in enumerate(pairs):
        whole = metrics.transcription_scores(ref_ns, est_ns)
        assert {key: scores[key][k] for key in whole} == whole
        for spec in specs[:2]:
            track = metrics.transcription_scores(extract_track(ref_ns, spec.program, False),
                                                 extract_track(est_ns, spec.program, False))
            assert {key: scores[spec.name + "/" + key][k] for key in track} == track
        for spec in specs:                                 # the frame rows: each track with the reference's all(is_drum) flag
            tracks = [extract_track(ns, spec.program, spec.is_drum) for ns in (ref_ns, est_ns)]
            want = metrics.frame_scores(*tracks, is_drum=all(n.is_drum for n in tracks[0].notes))
            assert {key: scores[spec.name + "/" + key][k] for key in want} == want
        drum_ref, drum_est = extract_track(ref_ns, 0, True), extract_track(est_ns, 0, True)
        ri, rp, _ = metrics.sequence_to_valued_intervals(drum_ref)
        ei, ep, _ = metrics.sequence_to_valued_intervals(drum_est)
        p, r, f = metrics.precision_recall_f1_overlap(ri, rp, ei, ep, offset_ratio=None)
        assert (scores["Drums/Onset precision"][k], scores["Drums/Onset recall"][k], scores["Drums/Onset F1"][k]) == (p, r, f)
        for g in GRANULARITIES:
            aware = metrics.program_aware_note_scores(ref_ns, est_ns, granularity_type=g)
            assert {key: scores[key][k] for key in aware} == aware
        drumless = [NoteSequence(notes=[n for n in ns.notes if not n.is_drum], total_time=ns.total_time)
                    for ns in (ref_ns, est_ns)]
        frames = metrics.frame_scores(*drumless, is_drum=not drumless[0].notes)      # the reference's all([...]) of no notes
        assert {key: scores[key][k] for key in frames} == frames
    for key, values in scores.items():
        assert got["mean"][key] == float(np.mean(values))
    assert metrics.transcription_metrics([]) == {"scores": {}, "mean": {}}


def test_matched_notes_lists_the_pairs(pairs):
    ref_ns, est_ns = pairs[0]
    got = metrics.matched_notes(ref_ns, est_ns)
    assert got.dtype == np.int64 and got.shape[1] == 2
    assert len(got) / len([n for n in ref_ns.notes if not n.is_drum]) == metrics.transcription_scores(ref_ns, est_ns)[
        "Onset + offset recall"]
    assert len(set(got[:, 0].tolist())) == len(got) == len(set(got[:, 1].tolist()))
    for i, j in got:
        r, e = ref_ns.notes[i], est_ns.notes[j]
        assert not r.is_drum and not e.is_drum and e.end_time != e.start_time
        assert metrics.match_notes([[r.start_time, r.end_time]], [r.pitch], [[e.start_time, e.end_time]], [e.pitch]) == 1


def test_a_pitch_of_zero_is_refused(pairs):
    bad = NoteSequence(notes=[Note(0.0, 1.0, 0, 100)])
    good = NoteSequence(notes=[Note(0.0, 1.0, 60, 100)])
    for pair in ((bad, good), (good, bad), (bad, NoteSequence())):
        with pytest.raises(ValueError):
            metrics.transcription_scores_many([pairs[0], pair])
        with pytest.raises(ValueError):
            metrics.transcription_metrics([pair])
        with pytest.raises(ValueError):
            metrics.transcription_scores(*pair)            # as the host path does


def test_score_against_on_the_command_line(tmp_path):
    _, y = synthetic.synth_music(2.048 + 0.7, seed=21, device="cpu")
    wav = tmp_path / "tune.wav"
    wav.write_bytes(audio_io.samples_to_wav_data(np.asarray(y, np.float32), 16000))
    refs, out = tmp_path / "refs", tmp_path / "out"
    assert transcribe.main(["--checkpoint", CKPT, "-o", str(refs / "tune.mid"), str(wav)]) == 0
    assert transcribe.main(["--checkpoint", CKPT, "--score-against", str(refs), "-o", str(out / "tune.mid"), str(wav)]) == 0
    assert sorted(os.listdir(out)) == ["scores.json", "tune.mid"]
    with open(refs / "tune.mid", "rb") as f:
        ref_ns = midi_io.midi_bytes_to_note_sequence(f.read())
    assert len([n for n in ref_ns.notes if not n.is_drum]) >= 5
    with open(out / "scores.json") as f:
        scores = json.load(f)
    assert list(scores) == ["files", "mean"] and list(scores["files"]) == ["tune"]
    assert scores["files"]["tune"] == scores["mean"]       # one file: the mean is the file
    has_drums = any(n.is_drum for n in ref_ns.notes)
    for key, value in scores["mean"].items():
        if key.startswith("Frame"):
            assert 0.0 <= value <= 1.0                     # the MIDI file's tick grid can move a frame edge
        elif key.startswith("Drum onset") and not has_drums:
            assert value == 0.0
        else:
            assert value == 1.0, key
