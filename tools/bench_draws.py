#!/usr/bin/env python3
"""What n sampled transcriptions cost as ONE engine job (`InferenceModel.sample` / `consensus`:
mt3_engine_transcribe_draws, every segment encoded once) against the way the same notes were made before: n `__call__`s of
the model with seeds seed .. seed + n - 1, each its own frontend pass, encoder passes and decode.  The trained fixture,
float32; `synth_music(--short)` (16.384 s: 9 segments, the framing always pads) and a piece of --long seconds.  Wall clock
around each call, the median of --runs runs after one warm-up (the warm-up also sizes the engine: both ways then run on
the same slots).
Writes one JSON record (and prints it); per piece:

  segments, draws            the job: segments of the piece, segments * n
  sample_ms, loop_ms         `sample(audio, n)` as one job / the loop of n calls; ratio = loop_ms / sample_ms
  consensus_ms               `consensus(audio, n)`: sample_ms plus the vote
  encoder_passes_*           encoder passes of each way (job: transcribe_stats; loop: the first pass into the caches plus
                             the staging passes of every call)
  slots                      decode slots of the job
  same_notes                 the two ways give the same n NoteSequences
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz"))
    ap.add_argument("--short", type=float, default=16.384)
    ap.add_argument("--long", type=float, default=120.0)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_draws.json"))
    args = ap.parse_args()
    import torch
    from mt3_amd import checkpoints, inference, synthetic

    n = args.samples
    model = inference.InferenceModel(checkpoints.load_compact_npz(args.checkpoint), "mt3", dtype="float32",
                                     decoding="sample", temperature=args.temperature, seed=0)
    notes = lambda ns: [(x.start_time, x.end_time, x.pitch, x.velocity, x.program, x.is_drum) for x in ns.notes]  # noqa: E731

    def timed(fn):
        ts = []
        for _ in range(args.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts[1:]), 2), out

    passes = [0]

    def loop(audio):
        """the n samples as they were made before the one job: n calls, seeds seed .. seed + n - 1"""
        was, out, passes[0] = model.sampling, [], 0
        try:
            for j in range(n):
                model.sampling = dataclasses.replace(was, seed=(was.seed + j) % (1 << 64))
                out.append(model(audio))
                passes[0] += 1 + model.model.transcribe_stats["encoder_chunks"]
        finally:
            model.sampling = was
        return out

    rec = {"tool": "bench_draws", "samples": n, "runs": args.runs, "temperature": args.temperature, "dtype": "float32",
           "pieces": {}}
    for name, seconds in (("short", args.short), ("long", args.long)):
        audio = synthetic.synth_music(seconds, seed=23, device="cpu")[1]
        sample_ms, samples = timed(lambda: model.sample(audio, n))
        st = dict(model.model.transcribe_stats)
        consensus_ms, _ = timed(lambda: model.consensus(audio, n))
        loop_ms, looped = timed(lambda: loop(audio))
        row = {"seconds": seconds, "segments": model.rows_per_engine_call[0], "draws": st["slots"] + st["refills"],
               "slots": st["slots"], "sample_ms": sample_ms, "consensus_ms": consensus_ms, "loop_ms": loop_ms,
               "ratio": round(loop_ms / sample_ms, 3), "encoder_passes_job": st["encoder_chunks"],
               "encoder_passes_loop": passes[0], "same_notes": [notes(a) for a in samples] == [notes(b) for b in looped]}
        rec["pieces"][name] = row
        print(name, row, file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
