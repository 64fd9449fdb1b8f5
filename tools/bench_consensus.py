#!/usr/bin/env python3
"""Cost of voting (mt3_amd.consensus) on one job: --files pieces of `random_music(--seconds)`, --voters transcriptions of
each made by moving every onset by up to 0.02 s, dropping one note in ten and adding a tenth of stray ones (fixed seed;
NOTE_DTYPE record arrays, so that the job is not millions of Python objects).  Writes one JSON record (and prints it):

  pack_ms        `consensus.pack`: the checks, the keys and the per-file sort on the host
  device_ms      `consensus.run`: the one upload, the mt3_op_note_consensus launches and the one copy back, wall clock
                 between device synchronisations
  reference_ms   `consensus.reference_columns` on the same packed job: the rule in numpy -- what device_ms is measured
                 against; `same_bits`: the two agree on every kept note and every note's votes
  results_ms     `consensus._results`: the columns -> NoteSequences (shared by both)
  one_file_*     the same for a job of the first file alone: one workgroup, bound by latency
Times are the median of --runs runs after one warm-up.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def voters_of(piece, n_voters, rng, np, dtype):
    start = np.array([n.start_time for n in piece.notes])
    end = np.array([n.end_time for n in piece.notes])
    pitch = np.array([n.pitch for n in piece.notes])
    out = []
    for _ in range(n_voters):
        keep = rng.uniform(size=len(start)) >= 0.1
        stray = len(start) // 10
        s = np.concatenate([np.maximum(start[keep] + rng.uniform(-0.02, 0.02, int(keep.sum())), 0.0),
                            rng.uniform(0.0, max(piece.total_time - 0.2, 0.1), stray)])
        e = np.concatenate([end[keep], np.zeros(stray)])
        e = np.maximum(e, s + 0.1)
        rec = np.zeros(len(s), dtype)
        rec["start_time"], rec["end_time"] = s, e
        rec["pitch"] = np.concatenate([pitch[keep], rng.integers(36, 97, stray)])
        rec["velocity"] = 100
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--voters", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_consensus.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from mt3_amd import consensus, metrics_utils, synthetic

    rng = np.random.default_rng(7)
    groups = [voters_of(synthetic.random_music(args.seconds, seed=100 + i), args.voters, rng, np, metrics_utils.NOTE_DTYPE)
              for i in range(args.files)]

    def timed(fn, sync=False):
        ts = []
        for i in range(args.runs + 1):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            if sync:
                torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts[1:]), 3), out

    rec = {"tool": "bench_consensus", "files": args.files, "seconds": args.seconds, "voters": args.voters, "runs": args.runs}
    for prefix, job in (("", groups), ("one_file_", groups[:1])):
        pack_ms, packed = timed(lambda: consensus.pack(job))
        device_ms, got = timed(lambda: consensus.run(packed), sync=True)
        reference_ms, want = timed(lambda: consensus.reference_columns(packed))
        results_ms, results = timed(lambda: consensus._results(packed, *got))
        same = bool(np.array_equal(got[-1], want[-1]) and np.array_equal(got[6], want[6]))
        for f, n in zip(packed.files, want[-1]):
            a = int(f["first"])
            same = same and all(np.array_equal(g[a: a + n].view(np.uint8), w[a: a + n].view(np.uint8))
                                for g, w in zip(got[:6], want[:6]))
        rec.update({prefix + "notes": packed.n_notes, prefix + "consensus_notes": int(want[-1].sum()),
                    prefix + "pack_ms": pack_ms, prefix + "device_ms": device_ms, prefix + "reference_ms": reference_ms,
                    prefix + "results_ms": results_ms, prefix + "same_bits": same})
        print(prefix or "job", {k: v for k, v in rec.items() if k.startswith(prefix or "pack")}, file=sys.stderr, flush=True)
    rec["reference_over_device"] = round(rec["reference_ms"] / rec["device_ms"], 3)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
