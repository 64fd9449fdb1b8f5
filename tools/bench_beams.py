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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--beams", default="1,2,4")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
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
    main()
