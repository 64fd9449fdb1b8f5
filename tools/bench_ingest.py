#!/usr/bin/env python3
"""Native-rate ingest: a 44.1 kHz stereo int16 WAV through the whole audio -> notes path, with the resample to 16 kHz on
the host (a) and on the device (b).  The workload is bench.py's `single_file`: a 10-minute synthetic file (six tones per
segment, seed 77), f32, beam-1, random weights with boosted note-event / EOS logits.  Its 16 kHz samples are
host-resampled up to 44.1 kHz and written as a stereo int16 WAV (both channels equal), which is what a user holds.

  a_host_resample   read_wav + audio_io.resample (scipy, float64, one CPU thread) + model(y16)
  b_device_resample read_wav + model(y, sample_rate=44100): upload, mt3_resampler_run, frontend, engine
  c_16k_file        model(y16) on the 16 kHz file itself: bench.py's single_file.file_sized_engine_refill on this box
  d_16k_resampled   model(y16) on the 16 kHz samples (a) resamples from the WAV: the model call of (a) and (b) alone (the
                    round trip through 44.1 kHz int16 changes the audio, so (a), (b) and (d) decode other notes than (c))
  e_wav_device      model.transcribe_wav(wav_bytes): the data chunk uploaded as it is, PCM decode + mixdown + resample in
                    one launch (mt3_resampler_run_pcm), frontend, engine
  e_wav_device_path the same from a path on disk (the chunk is read from the file inside the timed call)
Each wall time is the median of --runs timed calls after one warm-up call, clocked on the host around work that ends
in a device synchronise; min_s / max_s are the spread of those calls.  notes_identical: (a), (b) and both (e) give the
same notes.
  resample_kernel_ms  device time of mt3_resampler_run on the 10-minute file (events; median of 20)
  h2d_ms              the upload of the native f32 samples (events; pageable host memory, as the model call does it)
  pcm_kernel_ms       device time of mt3_resampler_run_pcm on the file's raw frames (events; median of 20; _min / _max
                      next to it, as for resample_kernel_ms)
  pcm_decode_ms       device time of mt3_pcm_decode on the same bytes (the path of a 16 kHz file), with the bytes it moves
                      per second (4 in and 4 out per stereo int16 frame) against the 8 TB/s HBM peak
  h2d_pcm_ms          the upload of the raw data chunk (events; out of the caller's bytes object)
  file_read_s         reading the data chunk from the file on disk (page cache warm; median of --runs)
  host_resample_s     audio_io.resample alone (median of --runs)
  read_wav_s          audio_io.read_wav alone: PCM decode and stereo mixdown on the host (median of --runs)
Prints one JSON line and writes it to --out.
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_ingest.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy.io import wavfile
    from mt3_amd import audio_io, inference, network, synthetic

    assert torch.cuda.is_available(), "bench_ingest needs a GPU"
    sr, minutes = args.rate, args.minutes
    n_seg = int(np.ceil(minutes * 60.0 / 2.048))
    wav16 = synthetic.synth_audio(n_seg, seed=77, tones=6).reshape(-1)[: int(minutes * 60.0 * 16000)].cpu().numpy()
    native = np.clip(audio_io.resample(wav16, 16000, sr), -1.0, 1.0)
    pcm = (native * 32767.0).astype(np.int16)
    buf = io.BytesIO()
    wavfile.write(buf, sr, np.stack([pcm, pcm], 1))
    wav_bytes = buf.getvalue()

    cfg = network.T5Config(dtype="float32")
    prm = synthetic.boost_note_events(network.init_random_params(cfg, seed=0), eos=4.0)
    m = inference.InferenceModel(prm, "mt3", dtype="float32", decoding="beam1")

    def notes(ns):
        return [(n.start_time, n.end_time, n.pitch, n.velocity, n.program, n.is_drum) for n in ns.notes]

    def path_a():
        y, r = audio_io.read_wav(wav_bytes)
        return m(audio_io.resample(y, r))

    def path_b():
        y, r = audio_io.read_wav(wav_bytes)
        return m(y, sample_rate=r)

    def path_c():
        return m(wav16)

    wav_dir = tempfile.TemporaryDirectory()
    wav_path = os.path.join(wav_dir.name, "ten_minutes.wav")
    with open(wav_path, "wb") as f:
        f.write(wav_bytes)

    def path_e():
        return m.transcribe_wav(wav_bytes)

    def path_e_path():
        return m.transcribe_wav(wav_path)

    y16_wav = audio_io.resample(*audio_io.read_wav(wav_bytes))

    def path_d():
        return m(y16_wav)

    def timed(fn):
        fn()                                      # warm-up: engine growth, graphs, resampler table upload
        torch.cuda.synchronize()
        walls, out = [], None
        for _ in range(args.runs):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        return statistics.median(walls), walls, out

    rec = {"tool": "bench_ingest", "minutes": minutes, "native_rate": sr, "native_samples": len(pcm),
           "samples_16k": audio_io.resampled_length(len(pcm), sr), "dtype": "float32", "decoding": "beam1",
           "runs": args.runs, "wav_bytes": len(wav_bytes)}
    res = {}
    for key, fn in (("c_16k_file", path_c), ("a_host_resample", path_a), ("b_device_resample", path_b),
                     ("d_16k_resampled", path_d), ("e_wav_device", path_e), ("e_wav_device_path", path_e_path)):
        wall, walls, ns = timed(fn)
        res[key] = notes(ns)
        rec[key] = {"wall_s": wall, "min_s": min(walls), "max_s": max(walls), "walls_s": walls, "notes": len(ns.notes)}
    rec["notes_identical"] = (res["a_host_resample"] == res["b_device_resample"] == res["e_wav_device"]
                              == res["e_wav_device_path"])
    rec["e_over_b"] = rec["e_wav_device"]["wall_s"] / rec["b_device_resample"]["wall_s"]
    rec["b_minus_e_s"] = rec["b_device_resample"]["wall_s"] - rec["e_wav_device"]["wall_s"]
    rec["b_over_c"] = rec["b_device_resample"]["wall_s"] / rec["c_16k_file"]["wall_s"]
    rec["a_over_c"] = rec["a_host_resample"]["wall_s"] / rec["c_16k_file"]["wall_s"]
    rec["b_over_d"] = rec["b_device_resample"]["wall_s"] / rec["d_16k_resampled"]["wall_s"]
    rec["notes_identical_d"] = res["d_16k_resampled"] == res["b_device_resample"]

    rw = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        y, r = audio_io.read_wav(wav_bytes)
        rw.append(time.perf_counter() - t0)
    rec["read_wav_s"] = statistics.median(rw)
    hs = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        y16h = audio_io.resample(y, r)
        hs.append(time.perf_counter() - t0)
    rec["host_resample_s"] = statistics.median(hs)
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    h2d, kern = [], []
    for _ in range(20):
        e0.record()
        yd = torch.from_numpy(y).cuda()
        e1.record()
        out = audio_io.resample_device(yd, r)
        e2.record()
        torch.cuda.synchronize()
        h2d.append(e0.elapsed_time(e1))
        kern.append(e1.elapsed_time(e2))
    rec["h2d_ms"] = statistics.median(h2d)
    rec["resample_kernel_ms"] = statistics.median(kern)
    rec["resample_kernel_ms_min"] = min(kern)
    rec["resample_kernel_ms_max"] = max(kern)
    # the same file through the PCM entries: raw chunk upload, fused decode + resample, decode alone
    from mt3_amd import _lib
    info = audio_io.wav_info(wav_bytes)
    lib, rs = _lib.load(), audio_io._resampler(r, 16000)
    stream = torch.cuda.current_stream().cuda_stream
    out_pcm = torch.empty(len(y16h), device="cuda", dtype=torch.float32)
    mono = torch.empty(info.frames, device="cuda", dtype=torch.float32)
    e3 = torch.cuda.Event(enable_timing=True)
    h2d_pcm, kern_pcm, dec = [], [], []
    for i in range(21):                           # the first pass warms the new kernels up and is not kept
        e0.record()
        pd = audio_io._upload_chunk(wav_bytes, info)
        e1.record()
        _lib.check(lib.mt3_resampler_run_pcm(rs, pd.data_ptr(), info.frames, info.channels, info.format,
                                             out_pcm.data_ptr(), out_pcm.shape[0], stream))
        e2.record()
        _lib.check(lib.mt3_pcm_decode(pd.data_ptr(), info.frames, info.channels, info.format, mono.data_ptr(),
                                      mono.shape[0], stream))
        e3.record()
        torch.cuda.synchronize()
        if i:
            h2d_pcm.append(e0.elapsed_time(e1))
            kern_pcm.append(e1.elapsed_time(e2))
            dec.append(e2.elapsed_time(e3))
    rec["h2d_pcm_ms"] = statistics.median(h2d_pcm)
    rec["pcm_kernel_ms"] = statistics.median(kern_pcm)
    rec["pcm_kernel_ms_min"] = min(kern_pcm)
    rec["pcm_kernel_ms_max"] = max(kern_pcm)
    rec["pcm_decode_ms"] = statistics.median(dec)
    rec["pcm_decode_bytes"] = info.data_bytes + 4 * info.frames
    rec["pcm_decode_tb_per_s"] = rec["pcm_decode_bytes"] / (rec["pcm_decode_ms"] * 1e-3) / 1e12
    rec["pcm_decode_share_of_hbm_peak"] = rec["pcm_decode_tb_per_s"] / 8.0
    rec["pcm_vs_float_path_samples_differing"] = int((out_pcm != out).sum().item())
    rec["pcm_decode_vs_read_wav_samples_differing"] = int((mono.cpu().numpy().view(np.int32) != y.view(np.int32)).sum())
    fr = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        np.fromfile(wav_path, np.uint8, info.data_bytes, offset=info.data_offset)
        fr.append(time.perf_counter() - t0)
    rec["file_read_s"] = statistics.median(fr)
    wav_dir.cleanup()
    taps = audio_io.kaiser_best_num_taps(r)
    up, down = audio_io.rate_ratio(r)
    rec["multiply_adds"] = int(len(y16h)) * (-(-taps // up))
    rec["kernel_gmacs_per_s"] = rec["multiply_adds"] / (rec["resample_kernel_ms"] * 1e-3) / 1e9
    d = out.cpu().numpy().view(np.int32).astype(np.int64) - y16h.view(np.int32).astype(np.int64)
    rec["kernel_vs_host_samples_differing"] = int((d != 0).sum())
    rec["kernel_vs_host_max_ulps"] = int(np.abs(d).max())
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
