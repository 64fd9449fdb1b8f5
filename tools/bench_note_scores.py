"""Times the job-level note scores (one device matching call per job) against a loop over the single-pair host functions,
for the same pairs on the same machine.

    python tools/bench_note_scores.py [--pairs 256] [--seconds 600] [--runs 5] [--out FILE.json]

The job: `--pairs` pieces of `synthetic.random_music(seconds, seed=i)` (600 s: about 3,100 notes each) as references.  Each
estimate is made by this file's own `estimate_of`, after the recipe of the tests' dense cases: 15 % of the reference's
notes dropped, onsets and offsets jittered (normal, sd 0.03 s), and 15 % extra notes added, these with `random_music`'s
pitch range (36 .. 96) and durations (0.12 .. 1.6 s).
Both sides of every comparison run on ALL pairs, alternating (device, host, device, host, ...): one warm-up of each, then
`--runs` timed runs of each; median and min - max.  The whole host loop takes seconds, so a run is well above scheduler
noise.  For `transcription_scores_many` the device path is also split into the conversion of the note objects to arrays,
the host packing (`note_matching.pack`) and the device call with its copy back (`note_matching.match` on the packed job)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mt3_amd import metrics, note_matching, synthetic  # noqa: E402
from mt3_amd.note_sequences import Note, NoteSequence  # noqa: E402

GRANULARITIES = ("flat", "midi_class", "full")


def estimate_of(ref_ns, rng):
    notes = []
    for n in ref_ns.notes:
        if rng.random() < 0.15:
            continue
        start = max(0.0, n.start_time + rng.normal(0.0, 0.03))
        notes.append(Note(float(start), float(max(start + 0.01, n.end_time + rng.normal(0.0, 0.03))), n.pitch, n.velocity))
    for t in rng.uniform(0.0, ref_ns.total_time, int(round(0.15 * len(ref_ns.notes)))):
        notes.append(Note(float(t), float(t + rng.uniform(0.12, 1.6)), int(rng.integers(36, 97)), 100))
    return NoteSequence(notes=notes, total_time=ref_ns.total_time)


def _once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _stats(samples):
    return {"median_s": float(np.median(samples)), "min_s": float(min(samples)), "max_s": float(max(samples)),
            "runs": len(samples)}


def timed(fn, runs):
    fn()
    return _stats([_once(fn) for _ in range(runs)])


def timed_alternating(device, host, runs):
    """one warm-up of each, then device and host in turn, `runs` times; the per-run ratio host / device beside them"""
    device()
    host()
    d, h = [], []
    for _ in range(runs):
        d.append(_once(device))
        h.append(_once(host))
    ratio = [b / a for a, b in zip(d, h)]
    return {"device": _stats(d), "host_loop": _stats(h),
            "host_over_device": {"median": float(np.median(ratio)), "min": float(min(ratio)), "max": float(max(ratio))}}


def host_sweep(ref_ns, est_ns):
    ri, rp, _ = metrics.sequence_to_valued_intervals(ref_ns, drums=False)
    ei, ep, _ = metrics.sequence_to_valued_intervals(est_ns, drums=False)
    return [metrics.precision_recall_f1_overlap(ri, rp, ei, ep, onset_tolerance=t, offset_min_tolerance=t)
            for t in metrics.SWEEP_TOLERANCES]


def host_metrics(pairs):
    for r, e in pairs:
        metrics.transcription_scores(r, e)
        for g in GRANULARITIES:
            metrics.program_aware_note_scores(r, e, g)
        host_sweep(r, e)
        metrics.frame_scores(r, e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    refs = [synthetic.random_music(args.seconds, seed=i) for i in range(args.pairs)]
    pairs = [(r, estimate_of(r, rng)) for r in refs]
    few = pairs[:4]
    result = {"pairs": len(pairs), "seconds": args.seconds,
              "ref_notes": int(sum(len(r.notes) for r, _ in pairs)), "est_notes": int(sum(len(e.notes) for _, e in pairs))}

    assert metrics.transcription_scores_many(few) == [metrics.transcription_scores(r, e) for r, e in few]
    rows = {
        "transcription_scores": (lambda p: metrics.transcription_scores_many(p),
                                 lambda p: [metrics.transcription_scores(r, e) for r, e in p]),
        "program_aware_note_scores": (lambda p: metrics.program_aware_note_scores_many(p, "full"),
                                      lambda p: [metrics.program_aware_note_scores(r, e, "full") for r, e in p]),
        "transcription_metrics": (lambda p: metrics.transcription_metrics(p), host_metrics),
    }
    for name, (device, host) in rows.items():
        result[name] = timed_alternating(lambda: device(pairs), lambda: host(pairs), args.runs)
        print(name, json.dumps(result[name]), flush=True)

    # transcription_scores_many, split: the host's packing, and the device call with its copy back
    job = metrics._MatchJob()
    for r, e in pairs:
        metrics._plan_transcription(job, metrics._valued(r, False), metrics._valued(e, False))
    packed = note_matching.pack(job.problems)
    result["split_transcription_scores"] = {
        "problems": len(job.problems),
        "valued_intervals": timed(lambda: [(metrics._valued(r, False), metrics._valued(e, False)) for r, e in pairs], args.runs),
        "pack": timed(lambda: note_matching.pack(job.problems), args.runs),
        "device_call_and_copy": timed(lambda: note_matching.match(job.problems, packed=packed), args.runs)}
    print("split", json.dumps(result["split_transcription_scores"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
