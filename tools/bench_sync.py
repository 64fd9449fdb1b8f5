#!/usr/bin/env python3
"""Cost of the three synchronisation launches (mt3_op_logmel_chroma, mt3_op_note_chroma, mt3_op_sync_paths), each timed
on its own, for jobs of --files x --seconds (default: 1, 32 and 256 files of 16 s, 120 s and 600 s; a combination whose
log-mel or workspace would not fit --max-gib of device memory is recorded as skipped).  Inputs: random float32 log-mel
(the cost does not depend on the values), `random_music(seconds)` as the score, --distinct different pieces repeated.
Timing: every buffer is allocated once, outside the timed region; a hipEvent pair (torch.cuda.Event) brackets a window
of back-to-back calls of ONE C entry point on the current stream (as many as fill about --window-ms), after --warmup
untimed calls; the per-launch median, minimum and maximum over --runs windows.  The path op's time is that of its slowest file: one workgroup per file.
Writes profiles/bench_sync.json (and prints it).  Not called by bench.py.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(launch, warmup, runs, inner):
    """hipEvent pairs around `inner` back-to-back launches; the per-launch time of each of `runs` windows"""
    import torch
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": runs, "launches_per_run": inner}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--seconds", type=float, nargs="+", default=[16.0, 120.0, 600.0])
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--pool", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=20.0, help="launches are repeated inside a timed window until it "
                    "is about this long (from an untimed first estimate)")
    ap.add_argument("--max-gib", type=float, default=64.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_sync.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from mt3_amd import _lib, note_arrays, sync, synthetic

    lib = _lib.load()
    n_mel, fps = 512, 125.0 / args.pool
    bins = np.random.default_rng(0).integers(-1, 12, n_mel).astype(np.int8)
    weights = np.array(sync.DEFAULT_WEIGHTS, np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    records = []
    for seconds in args.seconds:
        pieces = [synthetic.random_music(seconds, seed=300 + i) for i in range(args.distinct)]
        for n_files in args.files:
            rows = int(seconds * 125.0)
            packed = sync.pack([pieces[i % args.distinct] for i in range(n_files)], [rows] * n_files, [rows] * n_files,
                               args.pool, fps)
            files = packed.files
            words = int(files["work0"][-1]) + sync.workspace_words(files["n"][-1], files["m"][-1])
            total_a, total_s = int(files["n"].sum()), int(files["m"].sum())
            total_path = int(files["path0"][-1]) + sync.path_capacity(files["n"][-1], files["m"][-1])
            need = 4.0 * (n_files * rows * n_mel + words) / 2 ** 30
            rec = {"files": n_files, "seconds": seconds, "pool": args.pool, "feature_frames": int(files["n"][0]),
                   "score_frames": [int(m) for m in files["m"][: args.distinct]], "notes": packed.n_notes,
                   "cells": int((files["n"].astype(np.int64) * files["m"]).sum()), "device_gib": need}
            if need > args.max_gib:
                rec["skipped"] = "needs %.1f GiB of device memory" % need
                records.append(rec)
                continue
            # everything a launch touches is allocated once, outside the timed windows
            logmel = torch.randn((n_files * rows, n_mel), device="cuda")
            table = note_arrays.to_device(files.view(np.uint8).copy())
            n = packed.n_notes
            cols = [torch.from_numpy(packed.notes[4 * n * k: 4 * n * (k + 1)].view("<i4").copy()).cuda() for k in range(3)]
            bins_dev = torch.from_numpy(bins).cuda()
            a = torch.zeros((total_a, 12), device="cuda", dtype=torch.uint8)
            s = torch.zeros((total_s, 12), device="cuda", dtype=torch.uint8)
            scratch = torch.empty(12 * total_s, device="cuda", dtype=torch.int32)
            work = torch.empty(words, device="cuda", dtype=torch.int32)
            path = torch.empty((2, total_path), device="cuda", dtype=torch.int32)
            counts = torch.zeros((2, n_files), device="cuda", dtype=torch.int32)
            h, d = files.ctypes.data, table.data_ptr()
            launches = {
                "logmel_chroma": lambda: _lib.check(lib.mt3_op_logmel_chroma(
                    logmel.data_ptr(), n_files * rows, n_mel, h, d, n_files, bins_dev.data_ptr(), args.pool,
                    sync.DEFAULT_RANGE, sync.DEFAULT_FLOOR, a.data_ptr(), total_a, stream)),
                "note_chroma": lambda: _lib.check(lib.mt3_op_note_chroma(
                    cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), n, h, d, n_files, weights.ctypes.data,
                    len(weights), scratch.data_ptr(), s.data_ptr(), total_s, stream)),
                "sync_paths": lambda: _lib.check(lib.mt3_op_sync_paths(
                    a.data_ptr(), total_a, s.data_ptr(), total_s, h, d, n_files, work.data_ptr(), 4 * words,
                    path[0].data_ptr(), path[1].data_ptr(), total_path, counts[0].data_ptr(), counts[1].data_ptr(), stream)),
            }
            for name in ("logmel_chroma", "note_chroma", "sync_paths"):       # in the job's order: the paths read a and s
                first = timed(launches[name], 1, 1, 1)["median_ms"]
                inner = int(min(1000, max(1, round(args.window_ms / max(first, 1e-3)))))
                rec[name] = timed(launches[name], args.warmup, args.runs, inner)
            rec["sync_paths"]["cells_per_second"] = rec["cells"] / (rec["sync_paths"]["median_ms"] * 1e-3)
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del logmel, a, s, scratch, work, path
            torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0),
           "timing": "hipEvent pairs around back-to-back launches of one C entry point on preallocated buffers (windows of "
                     "about --window-ms; note_chroma is its memset and three kernels); per-launch median, minimum and "
                     "maximum over the windows after warm-up",
           "records": records}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
