#!/usr/bin/env python3
"""Does voting help on the trained fixture?  For `synth_music(--seconds)` with each of --seeds, float32: onset F1 and
onset + offset F1 (`metrics.transcription_scores`) against the rendered notes of
  default      the model's default decode (beam1)
  samples      each of --samples draws at --temperature: mean, lowest and highest
  consensus    their consensus at the majority default, at min_votes 2 and at min_votes = --samples
Writes one JSON record (and prints it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz"))
    ap.add_argument("--seconds", type=float, default=16.384)
    ap.add_argument("--seeds", default="23,31,47")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_f1.json"))
    args = ap.parse_args()
    import numpy as np
    from mt3_amd import checkpoints, consensus, inference, metrics, synthetic

    model = inference.InferenceModel(checkpoints.load_compact_npz(args.checkpoint), "mt3", dtype="float32",
                                     temperature=args.temperature, seed=0)
    keys = ("Onset F1", "Onset + offset F1")
    rec = {"tool": "consensus_f1", "seconds": args.seconds, "samples": args.samples, "temperature": args.temperature,
           "pieces": {}}
    for seed in [int(s) for s in args.seeds.split(",")]:
        truth, audio = synthetic.synth_music(args.seconds, seed=seed, device="cpu")
        score = lambda ns: [round(float(metrics.transcription_scores(truth, ns)[k]), 4) for k in keys]     # noqa: E731
        samples = model.sample(audio, args.samples)
        each = np.array([score(s) for s in samples])
        row = {"truth_notes": len(truth.notes), "default": score(model(audio)),
               "samples_mean": [round(float(v), 4) for v in each.mean(axis=0)],
               "samples_min": each.min(axis=0).tolist(), "samples_max": each.max(axis=0).tolist()}
        for name, q in (("consensus_majority", None), ("consensus_min_votes_2", 2),
                        ("consensus_min_votes_%d" % args.samples, args.samples)):
            result = consensus.consensus([samples], min_votes=q)[0]
            row[name] = score(result.notes)
            row[name + "_notes"] = len(result.notes.notes)
        rec["pieces"][str(seed)] = row
        print(seed, row, file=sys.stderr, flush=True)
    names = [k for k in next(iter(rec["pieces"].values())) if not k.endswith("_notes")]
    rec["mean"] = {k: [round(float(np.mean([p[k][j] for p in rec["pieces"].values()])), 4) for j in range(2)] for k in names}
    rec["columns"] = list(keys)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
