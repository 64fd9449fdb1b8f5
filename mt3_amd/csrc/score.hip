// Teacher-forced sequence scoring (mt3_engine_score): the decoder run as a PREFILL over all positions at once --
// Transformer.decode(..., decode=False) of mt3/network.py:303-361 -- followed by t5x score_batch's reduction.
//
// (1) score_embed_kernel: one workgroup per (segment, position) row of a chunk: the padded target row, the decoder
//     input token (shift_right(targets) with BOS = 0, or the caller's inputs) and Embed(tok) + FixedEmbed[t].
// (2) score_attn_kernel: flash-style attention of 64-query tiles (four waves of 16 queries) against K / V staged through
//     LDS in 64-key chunks.  The same MFMA arrangement as the encoder attention (attention.hip, enc_attn_chunk): S^T =
//     K Q^T with K as the A operand, so a lane holds the scores of ITS query, and the probabilities are already the A
//     operand of P V.  Two shapes:
//       causal self-attention (t5x make_decoder_mask: causal AND key target > 0), keys from the [rows, 3, H, 64] qkv
//       rows of the chunk; a 64-query tile visits only the key chunks at or before its last query;
//       cross-attention against the engine's cross-K/V cache [2][B][H][T][64] (T = 256 / 512 in 64-key chunks).
//     Masked keys are SELECTED away (their scores never enter the running maximum, their probabilities are 0 by
//     selection, not by exp underflow), and the V rows of keys whose target is 0 are staged as zeros, so no product of
//     the P V matrix step meets a value that was not finite or not causal-visible garbage.  A query without any
//     visible key (a padding position at 0) writes a zero row.
// (3) score_logprob_kernel: per row, log_softmax(logits)[target] * weight (0 where target == 0); the per-segment sum
//     (score_sum_kernel) runs over the positions in a FIXED order in double, so a sequence score has the same bits on
//     every run and in every batch.  score_token_stats_kernel (mt3_engine_score_segments with a top-1 output) is the
//     same reduction with the row's arg-max (lowest id on ties) and its log-probability next to the token score.
// (4) planes_kernel: an f32 matrix as the three bf16 planes of gemm_x6_kernel (hi = rne(w), mid = rne(w - hi), lo =
//     rne(w - hi - mid)), the same split upload_planes makes on the host, for the decoder matrices the f32 engine's
//     encoder-sized tile needs only when it scores.
#include <hip/hip_runtime.h>

#include "common.h"
#include "device.h"
#include "kernels.h"

namespace mt3k {

// ------------------------------------------------------------------------------------------------------ embedding
__global__ __launch_bounds__(128) void score_embed_kernel(ScoreEmbedArgs a) {
  const int r = blockIdx.x;                       // row of the chunk = seg * Lp + t
  const int seg = r / a.Lp, t = r % a.Lp;
  const bool in_len = t < a.length;
  const size_t src = static_cast<size_t>(a.seg0 + seg) * a.length + t;
  int tgt = in_len ? a.targets[src] : 0;
  int tok;
  if (a.dec_in) tok = in_len ? a.dec_in[src] : 0;
  else tok = (t == 0 || !in_len) ? 0 : a.targets[src - 1];
  // ids outside the vocabulary are the caller's error; they are clamped here so that no load leaves the table
  tgt = tgt < 0 ? 0 : (tgt >= a.vocab ? a.vocab - 1 : tgt);
  tok = tok < 0 ? 0 : (tok >= a.vocab ? a.vocab - 1 : tok);
  if (threadIdx.x == 0) a.tgt_pad[r] = tgt;
  const float* e = a.table + static_cast<size_t>(tok) * a.dim;
  const float* p = a.pos + static_cast<size_t>(t) * a.dim;
  float* y = a.y + static_cast<size_t>(r) * a.dim;
  for (int i = threadIdx.x * 4; i < a.dim; i += 512) {
    const float4 u = *reinterpret_cast<const float4*>(e + i), v = *reinterpret_cast<const float4*>(p + i);
    *reinterpret_cast<float4*>(y + i) = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
}

int launch_score_embed(const ScoreEmbedArgs& a, hipStream_t s) {
  if (!a.table || !a.pos || !a.targets || !a.y || !a.tgt_pad || a.Lp % 64 || a.length <= 0 || a.length > a.Lp ||
      a.rows % a.Lp || a.dim % 4)
    return mt3::fail(MT3_ERR_INVALID, "score_embed: bad arguments");
  hipLaunchKernelGGL(score_embed_kernel, dim3(a.rows), dim3(128), 0, s, a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ------------------------------------------------------------------------------------------------------ attention
template <typename CT>
__global__ __launch_bounds__(256) void score_attn_kernel(ScoreAttnArgs a) {
  constexpr int KPL = CTraits<CT>::KPL;
  constexpr int KG = CTraits<CT>::KGROUP;
  constexpr int D = 64;
  constexpr int CH = D / KPL;                     // 16-byte chunks per K / V row
  constexpr int ROWK = D + 2 * KPL;               // as the encoder attention: conflict-free b128 fragment reads
  constexpr int ROWV = 64 + 8;
  constexpr int NC = D / KG;
  __shared__ __attribute__((aligned(16))) CT Ks[64 * ROWK];
  __shared__ __attribute__((aligned(16))) CT Vt[D * ROWV];
  __shared__ int kok[64];                         // key visible by its target (causal visibility is per query)

  const int nqb = a.Lq / 64;
  const int qb = blockIdx.x % nqb, bh = blockIdx.x / nqb;
  const int b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int q0 = qb * 64 + wave * 16;             // the wave's 16 queries
  const CT* qbase = static_cast<const CT*>(a.q) + (static_cast<size_t>(b) * a.Lq) * a.q_stride + h * D;
  const int kvb = (b + a.kv_b0) / a.kv_share;      // kv_share = 1, kv_b0 = 0: b
  const CT* kbase = static_cast<const CT*>(a.k) + static_cast<size_t>(kvb) * a.kv_bstride + static_cast<size_t>(h) * a.kv_hstride;
  const CT* vbase = static_cast<const CT*>(a.v) + static_cast<size_t>(kvb) * a.kv_bstride + static_cast<size_t>(h) * a.kv_hstride;
  const int* ktgt = a.key_tgt ? a.key_tgt + static_cast<size_t>(b) * a.Lq : nullptr;

  u32x4 qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
    qf[c] = *reinterpret_cast<const u32x4*>(qbase + static_cast<size_t>(q0 + fr) * a.q_stride + c * KG + fg * KPL);

  float m = -3.0e38f, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int n_chunks = a.causal ? qb + 1 : a.n_keys / 64;
#pragma unroll 1
  for (int kc = 0; kc < n_chunks; ++kc) {
    const int key0 = kc * 64;
    if (kc) __syncthreads();                      // every wave is done with the previous chunk
    if (tid < 64) kok[tid] = ktgt ? (ktgt[key0 + tid] != 0) : 1;
    // K row-major; a key whose target is 0 is staged as zeros (its score is selected away anyway)
    for (int c = tid; c < 64 * CH; c += 256) {
      const int row = c / CH, ch = c % CH;
      const bool ok = !ktgt || ktgt[key0 + row] != 0;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (ok) v = *reinterpret_cast<const u32x4*>(kbase + static_cast<size_t>(key0 + row) * a.kv_stride + ch * KPL);
      *reinterpret_cast<u32x4*>(&Ks[row * ROWK + ch * KPL]) = v;
    }
    // V transposed [d][key]; zeros for keys whose target is 0
    for (int w = tid; w < 32 * CH; w += 256) {
      const int rp = w % 32, ch = w / 32;
      const int k0 = key0 + 2 * rp;
      const bool ok0 = !ktgt || ktgt[k0] != 0, ok1 = !ktgt || ktgt[k0 + 1] != 0;
      u32x4 v0 = u32x4{0u, 0u, 0u, 0u}, v1 = u32x4{0u, 0u, 0u, 0u};
      if (ok0) v0 = *reinterpret_cast<const u32x4*>(vbase + static_cast<size_t>(k0) * a.kv_stride + ch * KPL);
      if (ok1) v1 = *reinterpret_cast<const u32x4*>(vbase + static_cast<size_t>(k0 + 1) * a.kv_stride + ch * KPL);
      if constexpr (KPL == 8) {
        const bf16x8 x0 = __builtin_bit_cast(bf16x8, v0), x1 = __builtin_bit_cast(bf16x8, v1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
          const bf16x2 pr = {x0[j], x1[j]};
          *reinterpret_cast<bf16x2*>(&Vt[(ch * 8 + j) * ROWV + 2 * rp]) = pr;
        }
      } else {
        const f32x4 x0 = __builtin_bit_cast(f32x4, v0), x1 = __builtin_bit_cast(f32x4, v1);
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<float2*>(&Vt[(ch * 4 + j) * ROWV + 2 * rp]) = make_float2(x0[j], x1[j]);
      }
    }
    __syncthreads();

    // S^T block j: rows = keys j*16 + fg*4 + r, col = query q0 + fr
    f32x4 sc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const u32x4 kf = *reinterpret_cast<const u32x4*>(&Ks[(j * 16 + fr) * ROWK + c * KG + fg * KPL]);
        mfma_chunk<CT>(kf, qf[c], sc[j]);
      }
    }
    const int qi = q0 + fr;
    bool vis[4][4];
    float cm = -3.0e38f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = j * 16 + fg * 4 + r;
        vis[j][r] = kok[kk] && (!a.causal || key0 + kk <= qi);
        cm = vis[j][r] ? fmaxf(cm, sc[j][r]) : cm;
      }
    cm = fmaxf(cm, __shfl_xor(cm, 16));
    cm = fmaxf(cm, __shfl_xor(cm, 32));
    float alpha, ls = 0.f;
    if constexpr (sizeof(CT) == 2) {
      constexpr float kLog2e = 1.4426950408889634f;
      const float mn = fmaxf(m, cm * kLog2e);
      alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = vis[j][r] ? __builtin_amdgcn_exp2f(__builtin_fmaf(sc[j][r], kLog2e, -mn)) : 0.f;
          sc[j][r] = p;
          ls += p;
        }
    } else {
      const float mn = fmaxf(m, cm);
      alpha = expf(m - mn);
      m = mn;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = vis[j][r] ? expf(sc[j][r] - mn) : 0.f;
          sc[j][r] = p;
          ls += p;
        }
    }
    l = l * alpha + ls;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ar = __shfl(alpha, fg * 4 + r);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) o[nb][r] *= ar;
    }
    if constexpr (KPL == 8) {
#pragma unroll
      for (int kc2 = 0; kc2 < 2; ++kc2) {
        const float pv[8] = {sc[2 * kc2][0],     sc[2 * kc2][1],     sc[2 * kc2][2],     sc[2 * kc2][3],
                             sc[2 * kc2 + 1][0], sc[2 * kc2 + 1][1], sc[2 * kc2 + 1][2], sc[2 * kc2 + 1][3]};
        const u32x4 pa = pack_bf16x8(pv);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const CT* vrow = &Vt[(nb * 16 + fr) * ROWV + fg * 4];
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow + (2 * kc2) * 16);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + (2 * kc2 + 1) * 16);
          mfma_chunk<CT>(pa, u32x4{lo.x, lo.y, hi.x, hi.y}, o[nb]);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x4 pa = pack_f32x4(sc[j][0], sc[j][1], sc[j][2], sc[j][3]);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const u32x4 vb = *reinterpret_cast<const u32x4*>(&Vt[(nb * 16 + fr) * ROWV + j * 16 + fg * 4]);
          mfma_chunk<CT>(pa, vb, o[nb]);
        }
      }
    }
  }

  // normalise and store: O fragment row = query fg*4 + r, col = d = nb*16 + fr; 1/l of that query lives in lane fg*4 + r
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float linv = l > 0.f ? 1.f / l : 0.f;     // no visible key: a zero row
  float li[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) li[r] = __shfl(linv, fg * 4 + r);
  CT* out = static_cast<CT*>(a.out) + (static_cast<size_t>(b) * a.Lq + q0) * a.out_stride + h * D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    CT* dst = out + static_cast<size_t>(fg * 4 + r) * a.out_stride + fr;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) dst[nb * 16] = to_ct<CT>(o[nb][r] * li[r]);
  }
}

int launch_score_attention(int dtype, const ScoreAttnArgs& a, hipStream_t s) {
  if (!a.q || !a.k || !a.v || !a.out || a.B <= 0 || a.H <= 0 || a.Lq <= 0 || a.Lq % 64 ||
      (a.causal ? (a.n_keys != a.Lq) : (a.n_keys <= 0 || a.n_keys % 64)) || a.kv_share < 1 || a.kv_b0 < 0 ||
      a.kv_b0 >= a.kv_share)
    return mt3::fail(MT3_ERR_INVALID, "score_attention: bad arguments");
  const dim3 grid(a.B * a.H * (a.Lq / 64)), block(256);
  if (dtype == MT3_BF16) hipLaunchKernelGGL(score_attn_kernel<__bf16>, grid, block, 0, s, a);
  else if (dtype == MT3_F32) hipLaunchKernelGGL(score_attn_kernel<float>, grid, block, 0, s, a);
  else return mt3::fail(MT3_ERR_INVALID, "score_attention: unknown dtype");
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ------------------------------------------------------------------------------------------------------ reduction
// sum over the 64 lanes of a wave, then over the 4 waves through LDS: the same order on every run
template <typename F>
__device__ __forceinline__ F block_reduce(F v, F* red, bool is_max) {
  for (int off = 32; off > 0; off >>= 1) {
    const F u = __shfl_xor(v, off);
    v = is_max ? (v > u ? v : u) : v + u;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  F r = red[0];
  for (int w = 1; w < 4; ++w) r = is_max ? (r > red[w] ? r : red[w]) : r + red[w];
  return r;
}

__global__ __launch_bounds__(256) void score_logprob_kernel(ScoreReduceArgs a) {
  __shared__ float redf[4];
  const int r = blockIdx.x, seg = r / a.Lp, t = r % a.Lp;
  if (t >= a.length) return;                      // block-uniform
  const int tgt = a.tgt_pad[r];
  float sc = 0.f;
  if (tgt != 0) {
    const float* x = a.logits + static_cast<size_t>(r) * a.vocab;
    float mx = -3.0e38f;
    for (int i = threadIdx.x; i < a.vocab; i += 256) mx = fmaxf(mx, x[i]);
    mx = block_reduce<float>(mx, redf, true);
    float se = 0.f;
    for (int i = threadIdx.x; i < a.vocab; i += 256) se += expf(x[i] - mx);
    se = block_reduce<float>(se, redf, false);
    const float w = a.weights ? a.weights[static_cast<size_t>(a.seg0 + seg) * a.length + t] : 1.f;
    sc = (x[tgt] - mx - logf(se)) * w;
  }
  if (threadIdx.x == 0) {
    a.tok_pad[r] = sc;
    if (a.token_scores) a.token_scores[static_cast<size_t>(a.seg0 + seg) * a.length + t] = sc;
  }
}

__global__ __launch_bounds__(256) void score_sum_kernel(ScoreReduceArgs a) {
  __shared__ double redd[4];
  const int seg = blockIdx.x;
  const float* ts = a.tok_pad + static_cast<size_t>(seg) * a.Lp;
  double acc = 0.0;
  for (int t = threadIdx.x; t < a.length; t += 256) acc += static_cast<double>(ts[t]);
  acc = block_reduce<double>(acc, redd, false);
  if (threadIdx.x == 0) a.seq_scores[a.seg0 + seg] = static_cast<float>(acc);
}

int launch_score_reduce(const ScoreReduceArgs& a, hipStream_t s) {
  if (!a.logits || !a.tgt_pad || !a.tok_pad || !a.seq_scores || a.Lp % 64 || a.length <= 0 || a.length > a.Lp ||
      a.rows % a.Lp || a.vocab <= 0)
    return mt3::fail(MT3_ERR_INVALID, "score_reduce: bad arguments");
  hipLaunchKernelGGL(score_logprob_kernel, dim3(a.rows), dim3(256), 0, s, a);
  MT3_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(score_sum_kernel, dim3(a.rows / a.Lp), dim3(256), 0, s, a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ---------------------------------------------------------------------------------------------------- token statistics
// (value, id) pairs: the larger value wins, the LOWER id on equal values (lax.top_k's tie rule, as the beam kernels rank).
// The rule is symmetric, so after the butterfly every lane of a wave holds the same pair; the four waves are then
// combined in the order 0, 1, 2, 3.  The value that comes out is the one block_reduce<float>(.., true) finds.
__device__ __forceinline__ void argmax_take(float& v, int& id, float u, int uid) {
  const bool take = u > v || (u == v && uid < id);
  v = take ? u : v;
  id = take ? uid : id;
}

__device__ __forceinline__ void block_argmax(float& v, int& id, float* red_v, int* red_i) {
  for (int off = 32; off > 0; off >>= 1) {
    const float u = __shfl_xor(v, off);
    const int uid = __shfl_xor(id, off);
    argmax_take(v, id, u, uid);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    red_v[wave] = v;
    red_i[wave] = id;
  }
  __syncthreads();
  v = red_v[0];
  id = red_i[0];
  for (int w = 1; w < 4; ++w) argmax_take(v, id, red_v[w], red_i[w]);
}

// score_logprob_kernel plus the row's arg-max and its log-probability (mt3_engine_score_segments with a top-1 output,
// mt3_op_score_token_stats): the maximum and the sum of exp are reduced in score_logprob_kernel's order, so the token
// score has its bits; the arg-max rides in the pass that finds the maximum.
__global__ __launch_bounds__(256) void score_token_stats_kernel(ScoreStatsArgs s) {
  __shared__ float redf[4];
  __shared__ int redi[4];
  const ScoreReduceArgs& a = s.r;
  const int r = blockIdx.x, seg = r / a.Lp, t = r % a.Lp;
  if (t >= a.length) return;                      // block-uniform
  int tgt = a.tgt_pad[r];
  tgt = tgt < 0 ? 0 : (tgt >= a.vocab ? a.vocab - 1 : tgt);      // (the engine's rows arrive clamped by score_embed_kernel)
  float sc = 0.f, top = 0.f;
  int top_id = 0;
  if (tgt != 0) {
    const float* x = a.logits + static_cast<size_t>(r) * a.vocab;
    float mx = -3.0e38f;
    int id = 0x7fffffff;                          // nothing above -3e38 seen yet
    for (int i = threadIdx.x; i < a.vocab; i += 256) {
      const float v = x[i];
      if (v > mx) {                               // ascending i: the first of equal values stays
        mx = v;
        id = i;
      }
    }
    block_argmax(mx, id, redf, redi);
    top_id = id < a.vocab ? id : 0;
    float se = 0.f;
    for (int i = threadIdx.x; i < a.vocab; i += 256) se += expf(x[i] - mx);
    se = block_reduce<float>(se, redf, false);
    const float w = a.weights ? a.weights[static_cast<size_t>(a.seg0 + seg) * a.length + t] : 1.f;
    const float lse = logf(se);
    sc = (x[tgt] - mx - lse) * w;
    top = x[top_id] - mx - lse;
  }
  if (threadIdx.x == 0) {
    const size_t o = static_cast<size_t>(a.seg0 + seg) * a.length + t;
    if (a.tok_pad) a.tok_pad[r] = sc;
    if (a.token_scores) a.token_scores[o] = sc;
    if (s.top1_ids) s.top1_ids[o] = top_id;
    if (s.top1_scores) s.top1_scores[o] = top;
  }
}

int launch_score_stats(const ScoreStatsArgs& s, hipStream_t st) {
  const ScoreReduceArgs& a = s.r;
  if (!a.logits || !a.tgt_pad || !a.tok_pad || !a.seq_scores || a.Lp % 64 || a.length <= 0 || a.length > a.Lp ||
      a.rows % a.Lp || a.vocab < 2)
    return mt3::fail(MT3_ERR_INVALID, "score_stats: bad arguments");
  hipLaunchKernelGGL(score_token_stats_kernel, dim3(a.rows), dim3(256), 0, st, s);
  MT3_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(score_sum_kernel, dim3(a.rows / a.Lp), dim3(256), 0, st, a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ------------------------------------------------------------------------------------------------------ planes
__global__ __launch_bounds__(256) void planes_kernel(const float* __restrict__ w, __bf16* __restrict__ hi,
                                                     __bf16* __restrict__ mid, __bf16* __restrict__ lo, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = w[i];
  const __bf16 h = static_cast<__bf16>(v);
  const float r1 = v - static_cast<float>(h);
  const __bf16 m = static_cast<__bf16>(r1);
  const float r2 = r1 - static_cast<float>(m);
  hi[i] = h;
  mid[i] = m;
  lo[i] = static_cast<__bf16>(r2);
}

int launch_planes(const float* w, void* hi, void* mid, void* lo, size_t n, hipStream_t s) {
  if (!w || !hi || !mid || !lo || n == 0) return mt3::fail(MT3_ERR_INVALID, "planes: bad arguments");
  hipLaunchKernelGGL(planes_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, w,
                     static_cast<__bf16*>(hi), static_cast<__bf16*>(mid), static_cast<__bf16*>(lo), n);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

}  // namespace mt3k

// ---- include/mt3_hip.h: the statistics kernel on scripted logits (every row a "segment" of one position)
extern "C" int mt3_op_score_token_stats(const float* d_logits, const int32_t* d_targets, const float* d_weights,
                                        int32_t rows, int32_t vocab, float* d_token_scores, int32_t* d_top1_ids,
                                        float* d_top1_scores, void* stream) {
  if (!d_logits || !d_targets) return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_token_stats: null logits or targets");
  if (rows < 1 || vocab < 2) return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_token_stats: rows must be >= 1 and vocab >= 2");
  mt3k::ScoreStatsArgs s{};
  s.r = mt3k::ScoreReduceArgs{d_logits, d_targets, d_weights, nullptr, d_token_scores, nullptr, rows, 1, 1, 0, vocab};
  s.top1_ids = d_top1_ids;
  s.top1_scores = d_top1_scores;
  hipLaunchKernelGGL(mt3k::score_token_stats_kernel, dim3(rows), dim3(256), 0, static_cast<hipStream_t>(stream), s);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

// ---- include/mt3_hip.h: the other kernels of the scoring path, one at a time (test drivers: the launch description is
// filled and launched on `stream`, nothing else)
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int mt3_op_score_attention(int32_t dtype, const mt3_score_attn_view* v, void* stream) {
  const char* const me = "mt3_op_score_attention";
  if (!v) return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_attention: null view");
  if (dtype != MT3_BF16 && dtype != MT3_F32) return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_attention: unknown dtype");
  if (v->key_tgt && !v->causal)
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_attention: key_tgt is read by the causal form only");
  // the kernel loads query, K and V rows as 16-byte pieces
  const int per16 = dtype == MT3_BF16 ? 8 : 4;
  if (v->q_stride % per16 || v->kv_stride % per16 || v->kv_bstride % per16 || v->kv_hstride % per16 || !aligned16(v->q) ||
      !aligned16(v->k) || !aligned16(v->v))
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_attention: q / k / v and their strides must keep every row on 16 bytes");
  if (v->H > 0 && (v->q_stride < v->H * 64 || v->out_stride < v->H * 64 || v->kv_stride < 64))
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_attention: q_stride / out_stride below H * 64 or kv_stride below 64");
  mt3k::ScoreAttnArgs a{};
  a.q = v->q;
  a.q_stride = v->q_stride;
  a.k = v->k;
  a.v = v->v;
  a.kv_stride = v->kv_stride;
  a.kv_bstride = v->kv_bstride;
  a.kv_hstride = v->kv_hstride;
  a.key_tgt = v->key_tgt;
  a.out = v->out;
  a.out_stride = v->out_stride;
  a.B = v->B;
  a.H = v->H;
  a.Lq = v->Lq;
  a.n_keys = v->n_keys;
  a.causal = v->causal;
  return mt3::fail_as(me, mt3k::launch_score_attention(dtype, a, static_cast<hipStream_t>(stream)));
}

// rows / Lp / length of a chunk as launch_score_embed and launch_score_reduce take them (they divide by Lp)
static const char* bad_chunk(int32_t rows, int32_t Lp, int32_t length, int32_t seg0) {
  if (rows < 1 || Lp < 64 || seg0 < 0) return "rows must be >= 1, Lp >= 64 and seg0 >= 0";
  if (Lp % 64 || rows % Lp || length < 1 || length > Lp) return "Lp must be a multiple of 64, rows one of Lp, length in 1 .. Lp";
  return nullptr;
}

extern "C" int mt3_op_score_embed(const float* d_table, const float* d_pos, const int32_t* d_targets,
                                  const int32_t* d_dec_in, int32_t* d_tgt_pad, float* d_y, int32_t rows, int32_t Lp,
                                  int32_t length, int32_t seg0, int32_t dim, int32_t vocab, void* stream) {
  const char* const me = "mt3_op_score_embed";
  if (const char* why = bad_chunk(rows, Lp, length, seg0)) return mt3::fail(MT3_ERR_INVALID, std::string(me) + ": " + why);
  if (dim < 4 || dim % 4 || vocab < 1 || !aligned16(d_table) || !aligned16(d_pos) || !aligned16(d_y))
    return mt3::fail(MT3_ERR_INVALID, "mt3_op_score_embed: dim must be a positive multiple of 4, vocab >= 1, table / pos / "
                                      "y on 16 bytes");
  const mt3k::ScoreEmbedArgs a{d_table, d_pos, d_targets, d_dec_in, d_tgt_pad, d_y, rows, Lp, length, seg0, dim, vocab};
  return mt3::fail_as(me, mt3k::launch_score_embed(a, static_cast<hipStream_t>(stream)));
}

extern "C" int mt3_op_score_reduce(const float* d_logits, const int32_t* d_tgt_pad, const float* d_weights,
                                   float* d_tok_pad, float* d_token_scores, float* d_seq_scores, int32_t rows, int32_t Lp,
                                   int32_t length, int32_t seg0, int32_t vocab, int32_t* d_top1_ids, float* d_top1_scores,
                                   void* stream) {
  const char* const me = "mt3_op_score_reduce";
  if (const char* why = bad_chunk(rows, Lp, length, seg0)) return mt3::fail(MT3_ERR_INVALID, std::string(me) + ": " + why);
  const mt3k::ScoreReduceArgs a{d_logits, d_tgt_pad, d_weights, d_tok_pad, d_token_scores, d_seq_scores,
                                rows, Lp, length, seg0, vocab};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d_top1_ids || d_top1_scores)
    return mt3::fail_as(me, mt3k::launch_score_stats(mt3k::ScoreStatsArgs{a, d_top1_ids, d_top1_scores}, s));
  return mt3::fail_as(me, mt3k::launch_score_reduce(a, s));
}

extern "C" int mt3_op_planes(const float* d_w, void* d_hi, void* d_mid, void* d_lo, int64_t n, void* stream) {
  if (n < 1 || n > (int64_t{1} << 39)) return mt3::fail(MT3_ERR_INVALID, "mt3_op_planes: n must be in 1 .. 2^39");
  return mt3::fail_as("mt3_op_planes", mt3k::launch_planes(d_w, d_hi, d_mid, d_lo, static_cast<size_t>(n),
                                                          static_cast<hipStream_t>(stream)));
}
