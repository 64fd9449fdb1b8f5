#!/usr/bin/env python3
"""Cost of k-beam search (mt3_engine_decode_beams) at 256 decode slots: f32 and bf16, k = 1 / 2 / 4 (B = 256 / 128 / 64
segments), full `--steps` (no early exit), synthetic music through the trained fixture's weights
(tests/golden/mt3_synthetic_ckpt.npz).  Prints one JSON line:

  ms_per_step             wall time of the decode call / steps run (one warm-up call first; graphs captured by then)
  steps_run               steps the call ran
  forks_per_step          cache-row copies (MT3_STATUS_LAST_DECODE_FORKS) / steps run
  fork_copy_bytes_per_step  forks_per_step x the bytes one fork WRITES at the mean depth of the decode (steps / 2 positions
                          of K and V, every layer and head; it reads as many) -- an estimate: the copy depth of each fork
                          is not recorded
  audio_s_per_s           segments x 2.048 s / (encode + beam decode) of the best decode

--refill: in-flight batching of the beam search (mt3_engine_transcribe_beams, `Transformer.transcribe(num_beams=k)`)
against the batch-synchronous loop it replaces -- chunks of slots // k segments through encode(num_beams=k) +
decode_beams(k, early_exit=True) -- on `--segments` segments of synthetic music with natural EOS, k = 2 / 4, f32 and bf16,
both in the same process, `--repeats` timed runs each, alternating.  Every (dtype, k) configuration runs in a child
process of its own under `--step-timeout` seconds; the first one that fails ends the tool.  The result (audio-s/s of both
with their spread, the ratio of the medians, steps run, forks, starved polls) goes to `--out` and to stdout.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEG_SECONDS = 2.048
SEG = 32768


def refill_step(args, dtype, k):
    """one (dtype, k) configuration of --refill, in this process; prints one JSON line"""
    import numpy as np
    import torch
    from mt3_amd import _lib, checkpoints, network, spectrograms, synthetic

    params = checkpoints.load_compact_npz(os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz"))
    n_seg = args.segments
    _, wav = synthetic.synth_music(n_seg * SEG / 16000.0 + 1.0, seed=args.seed)
    wav = torch.as_tensor(np.asarray(wav, np.float32).reshape(-1)[: n_seg * SEG].reshape(n_seg, SEG))
    x = spectrograms.compute_spectrogram_batch(wav.cuda(), None).float().contiguous()
    eng = network.Transformer(network.T5Config(dtype=dtype), input_length=256, max_decode_length=1024, max_batch=args.slots)
    eng.load_params(params)
    chunk = args.slots // k

    def chunked():
        out, steps, forks = [], 0, 0
        for a in range(0, n_seg, chunk):
            eng.encode(x[a:a + chunk], num_beams=k)
            ids, _ = eng.decode_beams(k, num_steps=args.steps, early_exit=True)
            out.append(ids)
            steps += eng.steps_run
            forks += eng.status(_lib.STATUS_LAST_DECODE_FORKS)
        return torch.cat(out, 0), {"steps_run": steps, "forks": forks}

    def refill():
        ids = eng.transcribe(x, num_steps=args.steps, num_beams=k)
        st = dict(eng.transcribe_stats)
        return ids, {"steps_run": st["steps_run"], "forks": eng.status(_lib.STATUS_LAST_DECODE_FORKS),
                     "starved_polls": st["starved_polls"], "polls": st["polls"], "groups": st["groups"],
                     "encoder_chunks": st["encoder_chunks"], "used_graph": st["used_graph"]}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, info = fn()
        torch.cuda.synchronize()
        return ids, info, time.perf_counter() - t0

    a, _, _ = timed(chunked)                                                      # warm-up: graphs, staging ring
    b, _, _ = timed(refill)
    same = float((a == b).all(1).float().mean().item())
    rates = {"chunked": [], "refill": []}
    info = {}
    for _ in range(args.repeats):
        for name, fn in (("chunked", chunked), ("refill", refill)):
            _, info[name], dt = timed(fn)
            rates[name].append(round(n_seg * SEG_SECONDS / dt, 1))
    med = {n: sorted(v)[len(v) // 2] for n, v in rates.items()}
    print(json.dumps({"dtype": dtype, "k": k, "segments": n_seg, "slots": args.slots, "elements": chunk,
                      "identical_rows": same, "eos_rows": int((b == 1).any(1).sum().item()),
                      "audio_s_per_s": rates, "median": med,
                      "spread": {n: round((max(v) - min(v)) / med[n], 4) for n, v in rates.items()},
                      "refill_over_chunked": round(med["refill"] / med["chunked"], 4),
                      "chunked": info["chunked"], "refill": info["refill"]}), flush=True)


def refill_compare(args):
    """--refill: one child process per (dtype, k), each under its own time limit; nothing runs after a failed one"""
    import subprocess
    out = {"tool": "bench_beams --refill", "slots": args.slots, "segments": args.segments, "steps": args.steps,
           "repeats": args.repeats, "weights": "mt3_synthetic_ckpt", "runs": []}
    for dtype in args.dtypes.split(","):
        for k in (int(v) for v in args.beams.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--refill-step", "%s,%d" % (dtype, k), "--slots", str(args.slots),
                   "--segments", str(args.segments), "--steps", str(args.steps), "--repeats", str(args.repeats),
                   "--seed", str(args.seed)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print("bench_beams: %s k=%d ran past %d s; stopping" % (dtype, k, args.step_timeout), file=sys.stderr)
                return 1
            if r.returncode != 0:
                print("bench_beams: %s k=%d failed (%d); stopping\n%s" % (dtype, k, r.returncode, r.stderr[-2000:]),
                      file=sys.stderr)
                return 1
            out["runs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(out["runs"][-1]), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refill", action="store_true", help="compare in-flight batching with the batch-synchronous loop")
    ap.add_argument("--refill-step", default="", metavar="DTYPE,K", help="(one configuration of --refill, in this process)")
    ap.add_argument("--segments", type=int, default=640)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--beams", default="1,2,4")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    if args.refill_step:
        dtype, k = args.refill_step.split(",")
        return refill_step(args, dtype, int(k))
    if args.refill:
        if args.beams == "1,2,4":
            args.beams = "2,4"
        return refill_compare(args)
    import numpy as np
    import torch
    from mt3_amd import _lib, checkpoints, network, spectrograms, synthetic

    params = checkpoints.load_compact_npz(os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz"))
    n_seg = args.slots
    _, wav = synthetic.synth_music(n_seg * SEG / 16000.0 + 1.0, seed=args.seed)
    wav = torch.as_tensor(np.asarray(wav, np.float32).reshape(-1)[: n_seg * SEG].reshape(n_seg, SEG))
    x_all = spectrograms.compute_spectrogram_batch(wav.cuda(), None).float().contiguous()
    out = {"tool": "bench_beams", "slots": args.slots, "steps": args.steps, "weights": "mt3_synthetic_ckpt",
           "runs": []}
    for dtype in args.dtypes.split(","):
        cfg = network.T5Config(dtype=dtype)
        eng = network.Transformer(cfg, input_length=256, max_decode_length=1024, max_batch=args.slots)
        eng.load_params(params)
        esize = 4 if dtype == "float32" else 2
        fork_row_bytes = cfg.num_decoder_layers * cfg.num_heads * 64 * esize * 2    # K and V of one position
        for k in (int(v) for v in args.beams.split(",")):
            B = args.slots // k
            x = x_all[:B]
            eng.encode(x, num_beams=k)
            eng.decode_beams(k, num_steps=args.steps)                              # warm-up: graphs, caches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.encode(x, num_beams=k)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ids, _ = eng.decode_beams(k, num_steps=args.steps)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ran = eng.steps_run
            forks = eng.status(_lib.STATUS_LAST_DECODE_FORKS)
            out["runs"].append({
                "dtype": dtype, "k": k, "segments": B, "rows": B * k,
                "groups": eng.status(_lib.STATUS_LAST_DECODE_GROUPS),
                "ms_per_step": round((t2 - t1) * 1e3 / ran, 4), "steps_run": ran,
                "encode_ms": round((t1 - t0) * 1e3, 2), "decode_ms": round((t2 - t1) * 1e3, 1),
                "forks": forks, "forks_per_step": round(forks / ran, 3),
                "fork_copy_bytes_per_step": int(forks / ran * (args.steps / 2) * fork_row_bytes),
                "eos_rows": int((ids == 1).any(1).sum().item()),
                "audio_s_per_s": round(B * SEG_SECONDS / (t2 - t0), 2)})
            print(json.dumps(out["runs"][-1]), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
