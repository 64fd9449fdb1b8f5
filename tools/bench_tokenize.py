"""Times the target tokenizer: the host recipe against pack + upload + mt3_op_tokenize_notes.

Workload: `--files` pieces of synthetic.random_music(`--seconds`, seed=i), once as they are and once under 21 shifts.
Legs, each between device synchronisations, `--runs` alternating runs after one warm-up of each, median (min - max):
  (a) reference   tokenize.target_rows_reference looped over the files -- the only way before mt3_op_tokenize_notes
                  (timed on `--reference-files` files and, under shifts, on 3 of the 21 shifts, then scaled to the whole
                  job: the JSON states both)
  (b) pack        tokenize.plan: events, tables and rule on the host
  (c) device      upload + mt3_op_tokenize_notes (tokenize.run)
Writes profiles/bench_tokenize.json.  Recorded, not asserted."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reference-files", type=int, default=0, help="files the reference leg loops over (0: all); its time "
                    "is scaled to --files")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_tokenize.json"))
    args = ap.parse_args(argv)
    import torch
    from mt3_amd import note_sequences, synthetic, tokenize, vocabularies
    from tests import tokenize_cases
    spec = note_sequences.NoteEncodingWithTiesSpec
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    pieces = [synthetic.random_music(args.seconds, seed=i) for i in range(args.files)]
    frames = [int(args.seconds * 125) + 1] * args.files
    n_ref = args.reference_files or args.files
    result = {"files": args.files, "seconds": args.seconds, "runs": args.runs, "reference_files": n_ref, "reference_shifts_timed": 3,
              "notes": sum(len(p.notes) for p in pieces), "device": torch.cuda.get_device_name(0)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for label, shifts in (("plain", None), ("shifts21", [round(0.01 * (k - 10), 2) for k in range(21)])):
        def reference():
            for ns, f in zip(pieces[:n_ref], frames):
                for s in (shifts[::10] if shifts else [None]):
                    tokenize.target_rows_reference(ns if s is None else tokenize_cases.shifted(ns, s), f, codec, spec)

        def pack():
            return tokenize.plan(pieces, frames, codec, spec, shifts=shifts)

        legs = {"reference": reference, "pack": pack, "device": None}
        job = pack()
        legs["device"] = lambda: tokenize.run(job)
        times = {k: [] for k in legs}
        for k, fn in legs.items():                           # one warm-up of each
            timed(fn)
        for _ in range(args.runs):                           # alternating
            for k, fn in legs.items():
                times[k].append(timed(fn)[0] * (args.files / n_ref * (7.0 if shifts else 1.0) if k == "reference" else 1.0))
        result[label] = {"rows": int(len(job.rows)), "events": int(job.packed.events.shape[1]),
                         **{k: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v)} for k, v in times.items()}}
        print(label, json.dumps(result[label]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
