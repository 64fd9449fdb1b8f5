// PCM decode and channel mixdown for gfx950: interleaved little-endian WAV frames -> mono float32, the samples
// audio_io.read_wav computes on the host (the sample sources and their arithmetic are in pcm.h).
//
// Replaces the decode inside note_seq.audio_io.wav_data_to_samples_librosa (NB cell 2) for a file that is already at
// 16 kHz: the output is the frontend's zero-padded [n_segments, T*hop] buffer.  At any other rate the same sources
// feed the resampler's input staging instead (mt3_resampler_run_pcm, resample.hip) and this kernel does not run.
//
// One lane per frame, 256 consecutive frames per workgroup: a wave reads 64 neighbouring frames and stores 256
// contiguous bytes.  Outputs n_frames <= n < out_capacity are written as +0.0; nothing at or past out_capacity is
// touched.  The kernel moves (sample bytes * channels + 4) bytes per frame and is bound by memory.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "common.h"
#include "mt3_hip.h"
#include "pcm.h"

namespace {

constexpr int kThreads = 256;

template <class Src>
__global__ __launch_bounds__(kThreads) void pcm_decode_kernel(Src src, int64_t n_frames, float* __restrict__ y,
                                                              int64_t cap) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (n < cap) y[n] = n < n_frames ? src(n) : 0.f;
}

}  // namespace

extern "C" int mt3_pcm_decode(const void* d_pcm, int64_t n_frames, int32_t channels, int32_t format, float* d_out,
                              int64_t out_capacity, void* stream) {
  const int rc = mt3::pcm_check("mt3_pcm_decode", d_pcm, d_out, n_frames, channels, format);
  if (rc != MT3_OK) return rc;
  if (out_capacity < n_frames)
    return mt3::fail(MT3_ERR_INVALID, "mt3_pcm_decode: out_capacity " + std::to_string(out_capacity) +
                                          " is less than the " + std::to_string(n_frames) + " output samples");
  const int64_t blocks = out_capacity / kThreads + (out_capacity % kThreads != 0);
  if (blocks > INT32_MAX) return mt3::fail(MT3_ERR_INVALID, "mt3_pcm_decode: out_capacity too large");
  return mt3::pcm_dispatch(format, d_pcm, channels, [&](auto src) -> int {
    hipLaunchKernelGGL(pcm_decode_kernel<decltype(src)>, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), src, n_frames, d_out, out_capacity);
    MT3_HIP_CHECK(hipGetLastError());
    return MT3_OK;
  });
}
