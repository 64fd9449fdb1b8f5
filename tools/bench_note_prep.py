#!/usr/bin/env python
"""Cost of applying the sustain pedal (mt3_amd.note_prep) on one job: --files piano-like pieces of --seconds, about --notes
notes and --pedal controller-64 events each (a continuous-valued pedal going down and up every few seconds).  One JSON
line, also written to --out.  Medians of --runs after a warm-up, wall clock between device synchronisations.

  columns_ms     `note_prep.columns`: the checks and the NoteSequence -> numpy extraction, per file (host)
  pack_ms        `note_prep.pack`: the keys and the per-file sorts (host)
  device_ms      `note_prep.launch`: the one upload and the mt3_op_prepare_notes launches
  copy_back_ms   `note_prep.fetch`: the one copy back
  host_rule_ms   `note_sequences.apply_sustain_control_changes` over the same files: the event rule, what the device legs
                 are measured against (one run)
  same_bits      the device's survivors and ends equal the host rule's, file by file
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def piano_like(np, NS, rng, n_notes, n_pedal, seconds):
    ns = NS.NoteSequence()
    start = np.sort(rng.uniform(0, seconds - 1.0, n_notes))
    for s, d, p, v in zip(start, rng.uniform(0.05, 1.0, n_notes), rng.integers(21, 109, n_notes),
                          rng.integers(1, 128, n_notes)):
        ns.notes.append(NS.Note(float(s), float(s + d), int(p), int(v)))
    ns.total_time = max(n.end_time for n in ns.notes)
    t = np.sort(rng.uniform(0, seconds, n_pedal))
    value = np.clip(64 + 80 * np.sin(t * 1.7) + rng.integers(-8, 9, n_pedal), 0, 127).astype(int)
    ns.control_changes = [NS.ControlChange(float(a), 64, int(b)) for a, b in zip(t, value)]
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--notes", type=int, default=3000)
    ap.add_argument("--pedal", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_note_prep.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from mt3_amd import note_prep, note_sequences as NS

    rng = np.random.default_rng(9)
    job = [piano_like(np, NS, rng, args.notes, args.pedal, args.seconds) for _ in range(args.files)]

    def timed(fn, sync=False, runs=args.runs):
        ts = []
        for i in range(runs + 1):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            if sync:
                torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ts[1:]), 3), out

    columns_ms, files = timed(lambda: [note_prep.columns(ns, f) for f, ns in enumerate(job)])
    pack_ms, packed = timed(lambda: note_prep.pack(files, note_prep.SUSTAIN))
    device_ms, out = timed(lambda: note_prep.launch(packed), sync=True)
    copy_back_ms, (end, src, counts, total) = timed(lambda: note_prep.fetch(packed, out), sync=True)
    t0 = time.perf_counter()
    want = [NS.apply_sustain_control_changes(ns) for ns in job]
    host_rule_ms = round((time.perf_counter() - t0) * 1e3, 3)
    same = True
    for ns, w, f, n, t in zip(job, want, packed.files, counts, total):
        a = int(f["first"])
        w_end = np.array([x.end_time for x in w.notes])
        same = same and n == len(w.notes) and np.array_equal(end[a: a + n].view(np.uint64), w_end.view(np.uint64)) \
            and float(t) == w.total_time
    rec = {"tool": "bench_note_prep", "files": args.files, "seconds": args.seconds, "runs": args.runs,
           "notes": packed.n_notes, "pedal_events": packed.n_pedal, "survivors": int(counts.sum()),
           "upload_bytes": int(len(packed.notes) + len(packed.pedal)), "copy_back_bytes": int(out.numel()),
           "columns_ms": columns_ms, "pack_ms": pack_ms, "device_ms": device_ms, "copy_back_ms": copy_back_ms,
           "host_rule_ms": host_rule_ms, "same_bits": bool(same)}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
