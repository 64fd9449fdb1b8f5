#!/usr/bin/env python3
"""Cost of aligning known notes to audio (InferenceModel.align_notes_many's device legs) on one job: --files pieces of
`random_music(--seconds)` (--distinct different ones, repeated), K = --shifts candidate shifts, random weights at the MT3
shape, random log-mel (the encoder's cost does not depend on its input).  Writes one JSON record (and prints it):

  table_replicated_ms   the (segment, shift) table as `score_notes_many` gets it: `score_segments` on the log-mel
                        replicated once per shift -- K encoder passes per segment
  table_shared_ms       the same table by `score_candidates`: one encoder pass per segment; `saving` = the ratio
  encoder_passes_*      MT3_STATUS_SCORE_ENCODER_PASSES of either call
  same_bits             float32: the two tables are torch.equal
  paths_ms              `alignment.best_paths` over the job's table (upload of the file table, the launches, the wait)
  warp_ms               `alignment.warp_notes` of all files on the host
Times are wall clock between device synchronisations, the median of --runs alternating runs after a warm-up of each.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--shifts", type=int, default=21)
    ap.add_argument("--step", type=float, default=0.02)
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_align.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from mt3_amd import _lib, alignment, network, note_sequences, synthetic, tokenize, vocabularies

    K, T, L = args.shifts, 256, 1024
    grid = (np.arange(K) - K // 2).astype(np.float64) * args.step
    seconds = T / 125.0
    codec = vocabularies.build_codec(vocabularies.VocabularyConfig(num_velocity_bins=1))
    pieces = [synthetic.random_music(args.seconds, seed=100 + i) for i in range(args.distinct)]
    files = [pieces[i % args.distinct] for i in range(args.files)]
    n_frames = [int(args.seconds * 16000) // 128 + 1] * args.files
    rows = tokenize.target_rows(files, n_frames, codec, note_sequences.NoteEncodingWithTiesSpec, shifts=list(grid),
                                stride=L, segment_frames=T)
    table = rows.rows_of_file
    counts = [int(table[i, 0, 1]) for i in range(args.files)]
    total = sum(counts)
    order = np.concatenate([(table[i, :, 0][None, :] + np.arange(counts[i])[:, None]).reshape(-1)
                            for i in range(args.files)])
    seg0 = np.concatenate([[0], np.cumsum(counts)])
    source = np.concatenate([seg0[i] + np.arange(counts[i]) for i in range(args.files) for _ in range(K)])
    width = max(int(rows.lengths.max()), 1)
    order_dev = torch.from_numpy(order).cuda()
    ids_files = rows.ids[:, :width].contiguous()              # (file, shift, segment): score_notes_many's order
    ids_table = ids_files.index_select(0, order_dev)          # (file, segment, shift)
    del rows

    cfg = network.T5Config(dtype=args.dtype)
    eng = network.Transformer(cfg, input_length=T, max_decode_length=L, max_batch=args.slots)
    eng.load_params(network.init_random_params(cfg, seed=0))
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((total, T, cfg.input_depth), device="cuda", generator=g) * 2.0 - 4.0
    source_dev = torch.from_numpy(source).cuda()

    def replicated():
        # the log-mel is replicated in slices of one shift of one file at a time inside score_notes_many's index_select;
        # here per 4,096 rows, so that the bench does not hold K copies of the job's log-mel
        out = []
        for at in range(0, len(source), 4096):
            out.append(eng.score_segments(x.index_select(0, source_dev[at: at + 4096]), ids_files[at: at + 4096]))
        return torch.cat(out).index_select(0, order_dev).view(total, K)

    def shared():
        return eng.score_candidates(x, ids_table, K).view(total, K)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rec = {"tool": "bench_align", "files": args.files, "seconds": args.seconds, "shifts": K, "dtype": args.dtype,
           "slots": args.slots, "segments": total, "rows": total * K, "row_width": width, "runs": args.runs}
    _, a = timed(shared)                                      # warm-up: workspace, planes
    rec["encoder_passes_shared"] = eng.status(_lib.STATUS_SCORE_ENCODER_PASSES)
    rec["prefill_pieces_shared"] = eng.status(_lib.STATUS_SCORE_CHUNKS)
    eng.score_segments(x[:8], ids_table[:8])                  # warm-up of the other entry
    ts, tr = [], []
    for _ in range(args.runs):
        t, b = timed(replicated)
        tr.append(t)
        t, a = timed(shared)
        ts.append(t)
        print("replicated %.1f ms, shared %.1f ms" % (tr[-1], ts[-1]), file=sys.stderr, flush=True)
    rec["encoder_passes_replicated"] = -(-4096 // args.slots) * (len(source) // 4096) + -(-(len(source) % 4096) // args.slots)
    rec["table_replicated_ms"], rec["table_replicated_ms_all"] = round(statistics.median(tr), 1), [round(t, 1) for t in tr]
    rec["table_shared_ms"], rec["table_shared_ms_all"] = round(statistics.median(ts), 1), [round(t, 1) for t in ts]
    rec["saving"] = round(statistics.median(tr) / statistics.median(ts), 3)
    rec["same_bits"] = bool(torch.equal(a, b))

    scores = a.contiguous()
    alignment.best_paths(scores, counts, grid, alignment.DEFAULT_SMOOTHNESS)
    tp = [timed(lambda: alignment.best_paths(scores, counts, grid, alignment.DEFAULT_SMOOTHNESS)) for _ in range(max(args.runs, 5))]
    rec["paths_ms"], rec["paths_ms_all"] = round(statistics.median(t for t, _ in tp), 3), [round(t, 3) for t, _ in tp]
    path = tp[-1][1][0].cpu().numpy()
    t0 = time.perf_counter()
    first = 0
    for ns, n in zip(files, counts):
        alignment.warp_notes(ns, grid[path[first: first + n]], seconds)
        first += n
    rec["warp_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    rec["notes"] = sum(len(ns.notes) for ns in files)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
