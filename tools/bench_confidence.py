#!/usr/bin/env python3
"""What note confidences cost: InferenceModel.transcribe_wav against transcribe_wav_scored (the same decode, then one
mt3_engine_score_segments pass over the decoded rows and the traced note decode) on one synthetic file of --seconds
(default 600 = 10 minutes, 293 segments), in f32 and bf16, on the trained fixture checkpoint.

Per dtype: one warm-up call of each form (engine sized to the job, step graphs, score workspace and planes), then --runs
(default 5) timed pairs, the two forms ALTERNATING so that drift of the shared host hits both; every call sits between
two device events on the current stream and ends in a synchronise (the calls block on their own: they return notes).
Reported: the median of each form in ms (events; the host clock's median next to it), all samples, and
ratio = scored / plain.  `plain` is the code path the parent commit times as transcribe_wav: this change does not touch it.
Prints one JSON line.

    python tools/bench_confidence.py [--seconds 600] [--runs 5] [--dtypes float32,bfloat16] [--checkpoint PATH]
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
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--checkpoint", default=os.path.join(ROOT, "tests", "golden", "mt3_synthetic_ckpt.npz"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_confidence: needs a GPU (a CPU run measures nothing)")
    from mt3_amd import _lib, audio_io, inference, synthetic

    _, samples = synthetic.synth_music(args.seconds, seed=13)
    wav = audio_io.samples_to_wav_data(samples, 16000)
    out = {"tool": "bench_confidence", "seconds": args.seconds, "runs": args.runs, "results": []}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        return r, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

    for dtype in args.dtypes.split(","):
        m = inference.InferenceModel(args.checkpoint, "mt3", dtype=dtype)
        ns, _, _ = timed(lambda: m.transcribe_wav(wav))                      # warm-up of both forms
        (ns_s, sc), _, _ = timed(lambda: m.transcribe_wav_scored(wav))
        assert [(n.start_time, n.end_time, n.pitch) for n in ns.notes] == \
            [(n.start_time, n.end_time, n.pitch) for n in ns_s.notes], "the scored call returned other notes"
        ev = {"plain": [], "scored": []}
        host = {"plain": [], "scored": []}
        for _ in range(args.runs):
            for name, fn in (("plain", lambda: m.transcribe_wav(wav)), ("scored", lambda: m.transcribe_wav_scored(wav))):
                _, e, h = timed(fn)
                ev[name].append(e)
                host[name].append(h)
        med = {k: statistics.median(v) for k, v in ev.items()}
        res = {"dtype": dtype, "segments": int(m.rows_per_engine_call[0]), "notes": len(ns.notes),
               "engine_slots": m.engine_slots, "score_chunks": m.model.status(_lib.STATUS_SCORE_CHUNKS),
               "plain_ms": round(med["plain"], 1), "scored_ms": round(med["scored"], 1),
               "ratio": round(med["scored"] / med["plain"], 4),
               "plain_host_ms": round(statistics.median(host["plain"]), 1),
               "scored_host_ms": round(statistics.median(host["scored"]), 1),
               "plain_ms_all": [round(t, 1) for t in ev["plain"]], "scored_ms_all": [round(t, 1) for t in ev["scored"]],
               "mean_onset_logprob": round(float(sc["onset_logprob"].mean()), 4) if len(ns.notes) else None}
        out["results"].append(res)
        print(json.dumps(res), file=sys.stderr, flush=True)
        m = None
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
