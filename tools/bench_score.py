#!/usr/bin/env python3
"""Cost of teacher-forced scoring (mt3_engine_score) at the MT3 shape: B = 256 segments x length 1,024, f32 and bf16,
random weights, random regular-vocabulary targets (no padding: every position is scored).  For comparison the cached
teacher-forced decode of the same rows, Transformer.decode_forced(return_logits=False): 1,024 one-token steps on the
caller's stream (no row groups).  Prints one JSON line; per dtype:

  score_ms                wall time of one score call (median of --runs, after one warm-up call)
  segments_per_s / tokens_per_s   B / score_ms, B * length / score_ms
  decode_forced_ms        wall time of one decode_forced call (after one warm-up call); speedup = its ratio to score_ms
  tflops / mfma_fraction  the FLOP count below over score_ms, and over the matrix peak of the dtype's attention pipe
                          (f32: 157.3 TFLOP/s of v_mfma_f32 -- the dense layers run on the bf16 pipes as three planes, six
                          products each, so the f32 fraction counts the work the network asks for, not the products issued;
                          bf16: 2,516.6 TFLOP/s dense)
FLOP count per scored token (multiply-add = 2): dense 2 x (per decoder layer emb x (3HD + HD) + HD x emb x 2 + emb x 2 mlp +
mlp x emb, then emb x vocab), attention 2 x 2 x 64 x H x (causal keys at the mean depth (length + 1) / 2 + T cross keys)
per layer.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = {"float32": 157.3e12, "bfloat16": 2516.6e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--no-decode-forced", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from mt3_amd import _lib, network

    B, n, T = args.batch, args.length, 256
    out = {"tool": "bench_score", "batch": B, "length": n, "input_length": T, "runs": []}
    for dtype in args.dtypes.split(","):
        cfg = network.T5Config(dtype=dtype)
        hd, emb, mlp, V, H = cfg.num_heads * 64, cfg.emb_dim, cfg.mlp_dim, cfg.vocab_size, cfg.num_heads
        dense = 2 * (cfg.num_decoder_layers * (emb * 4 * hd + 2 * hd * emb + emb * 2 * mlp + mlp * emb) + emb * V)
        attn = 2 * 2 * 64 * H * ((n + 1) / 2 + T) * cfg.num_decoder_layers
        eng = network.Transformer(cfg, input_length=T, max_decode_length=1024, max_batch=B)
        eng.load_params(network.init_random_params(cfg, seed=0))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((B, T, cfg.input_depth), device="cuda", generator=g) * 2.0 - 4.0
        tgt = torch.randint(3, 3 + 1388, (B, n), device="cuda", dtype=torch.int32, generator=g)
        eng.encode(x)
        eng.score(tgt)                                        # warm-up: workspace, planes
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            eng.score(tgt)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        sc = statistics.median(ts)
        run = {"dtype": dtype, "score_ms": round(sc * 1e3, 2), "score_ms_all": [round(t * 1e3, 2) for t in ts],
               "chunks": eng.status(_lib.STATUS_SCORE_CHUNKS), "segments_per_s": round(B / sc, 1),
               "tokens_per_s": round(B * n / sc, 0), "mflop_per_token_dense": round(dense / 1e6, 2),
               "mflop_per_token_attention": round(attn / 1e6, 2),
               "tflop_per_call": round((dense + attn) * B * n / 1e12, 3),
               "tflops": round((dense + attn) * B * n / sc / 1e12, 1),
               "mfma_fraction": round((dense + attn) * B * n / sc / PEAK[dtype], 4),
               "device_bytes": eng.device_bytes}
        if not args.no_decode_forced:
            eng.decode_forced(tgt, return_logits=False)        # warm-up: step graph
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.decode_forced(tgt, return_logits=False)
            torch.cuda.synchronize()
            df = time.perf_counter() - t0
            run["decode_forced_ms"] = round(df * 1e3, 1)
            run["speedup_vs_decode_forced"] = round(df / sc, 2)
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
