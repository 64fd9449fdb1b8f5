// Sample sources of the ingest kernels (resample.hip, pcm.hip): functors that give mono float32 sample k of an input,
// either a float32 array as it is or interleaved little-endian PCM frames decoded and mixed down on the fly with
// audio_io.read_wav's arithmetic (include/mt3_hip.h, "PCM decode", has the table).
//
//   * every integer scale is a power of two, so the multiplications by 2^-7 / 2^-15 / 2^-31 below are the exact
//     divisions read_wav performs; int32 -> f32 and f64 -> f32 are the hardware's round-to-nearest-even conversions,
//     as numpy's astype.
//   * the mixdown is numpy's mean over fewer than 8 addends: a float32 sum from +0.0 in channel order and ONE
//     division by float(channels) (hipcc's f32 `/` is correctly rounded unless asked otherwise, and build.py does not
//     ask).  A mono frame is returned as loaded: a float file keeps its -0.0 and its NaN bits.
//   * loads are one sample wide.  S24 is assembled from three byte loads: a sample may sit at any byte address, and
//     byte loads never read outside [d_pcm, d_pcm + n_frames * 3 * channels), which aligned dword loads around the
//     first and the last sample would.  Neighbouring lanes read neighbouring frames, so a wave's loads fall into the
//     same few 128-byte lines whatever the sample width.
//   * indices are int64: byte offsets pass 2^31 on a 10-minute multichannel file.
#ifndef MT3_PCM_H_
#define MT3_PCM_H_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "common.h"
#include "mt3_hip.h"

namespace mt3 {

// bytes of one sample of `format`; 0 for an unknown format
inline int pcm_sample_bytes(int32_t format) {
  switch (format) {
    case MT3_PCM_U8: return 1;
    case MT3_PCM_S16: return 2;
    case MT3_PCM_S24: return 3;
    case MT3_PCM_S32: return 4;
    case MT3_PCM_F32: return 4;
    case MT3_PCM_F64: return 8;
    default: return 0;
  }
}

// the argument checks the two PCM entry points share (`who` names the entry in the message); MT3_OK or MT3_ERR_INVALID
inline int pcm_check(const char* who, const void* d_pcm, const float* d_out, int64_t n_frames, int32_t channels,
                     int32_t format) {
  const std::string w(who);
  if (!d_pcm || !d_out) return fail(MT3_ERR_INVALID, w + ": null argument");
  if (n_frames < 1) return fail(MT3_ERR_INVALID, w + ": n_frames must be >= 1");
  if (channels < 1 || channels > MT3_PCM_MAX_CHANNELS)
    return fail(MT3_ERR_INVALID, w + ": channels must be 1 .. 7, got " + std::to_string(channels));
  if (!pcm_sample_bytes(format))
    return fail(MT3_ERR_INVALID, w + ": unknown format " + std::to_string(format) + " (MT3_PCM_*)");
  // byte offsets (n_frames * channels * sample bytes <= n_frames * 56) must stay in int64
  if (n_frames > INT64_MAX / (MT3_PCM_MAX_CHANNELS * 8)) return fail(MT3_ERR_INVALID, w + ": n_frames too large");
  return MT3_OK;
}

// sample i (counted in samples, not frames) of the buffer at p
template <int FMT>
__device__ __forceinline__ float pcm_sample(const uint8_t* __restrict__ p, int64_t i) {
  if constexpr (FMT == MT3_PCM_U8) {
    return (static_cast<float>(p[i]) - 128.f) * 0x1p-7f;
  } else if constexpr (FMT == MT3_PCM_S16) {
    return static_cast<float>(reinterpret_cast<const int16_t*>(p)[i]) * 0x1p-15f;
  } else if constexpr (FMT == MT3_PCM_S24) {
    const uint8_t* b = p + 3 * i;
    const uint32_t u = static_cast<uint32_t>(b[0]) << 8 | static_cast<uint32_t>(b[1]) << 16 |
                       static_cast<uint32_t>(b[2]) << 24;
    return static_cast<float>(static_cast<int32_t>(u)) * 0x1p-31f;
  } else if constexpr (FMT == MT3_PCM_S32) {
    return static_cast<float>(reinterpret_cast<const int32_t*>(p)[i]) * 0x1p-31f;
  } else if constexpr (FMT == MT3_PCM_F32) {
    return reinterpret_cast<const float*>(p)[i];
  } else {
    static_assert(FMT == MT3_PCM_F64, "unknown MT3_PCM_* format");
    return static_cast<float>(reinterpret_cast<const double*>(p)[i]);
  }
}

// x[k]: a float32 array
struct F32Samples {
  const float* __restrict__ x;
  __device__ __forceinline__ float operator()(int64_t k) const { return x[k]; }
};

// frame k of interleaved PCM, mixed down to mono
template <int FMT>
struct PcmFrames {
  const uint8_t* __restrict__ p;
  int32_t channels;  // 1 .. MT3_PCM_MAX_CHANNELS
  __device__ __forceinline__ float operator()(int64_t k) const {
    const int64_t i = k * channels;
    if (channels == 1) return pcm_sample<FMT>(p, i);
    float acc = 0.f;
    for (int c = 0; c < channels; ++c) acc = acc + pcm_sample<FMT>(p, i + c);
    return acc / static_cast<float>(channels);
  }
};

// f(PcmFrames<format>{p, channels}) for a runtime `format` that pcm_check has accepted
template <class F>
int pcm_dispatch(int32_t format, const void* d_pcm, int32_t channels, F&& f) {
  const uint8_t* p = static_cast<const uint8_t*>(d_pcm);
  switch (format) {
    case MT3_PCM_U8: return f(PcmFrames<MT3_PCM_U8>{p, channels});
    case MT3_PCM_S16: return f(PcmFrames<MT3_PCM_S16>{p, channels});
    case MT3_PCM_S24: return f(PcmFrames<MT3_PCM_S24>{p, channels});
    case MT3_PCM_S32: return f(PcmFrames<MT3_PCM_S32>{p, channels});
    case MT3_PCM_F32: return f(PcmFrames<MT3_PCM_F32>{p, channels});
    default: return f(PcmFrames<MT3_PCM_F64>{p, channels});
  }
}

}  // namespace mt3

#endif  // MT3_PCM_H_
