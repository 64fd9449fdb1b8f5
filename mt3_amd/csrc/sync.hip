// Score-to-audio synchronisation for gfx950: chroma of a recording from the float32 log-mel the frontend has written
// (mt3_op_logmel_chroma), chroma of a score from its notes (mt3_op_note_chroma), and the dynamic-time-warping path between
// the two (mt3_op_sync_paths).  The rules: include/mt3_hip.h, "score-to-audio synchronisation"; their numpy statements:
// mt3_amd/sync.py, logmel_chroma_reference / note_chroma_reference / paths_reference.
//
// One file table serves the three ops; the kernels read its device copy, so a job of any number of files is one launch
// per kernel.
//
// logmel_chroma_kernel: a wave per feature frame, four to a workgroup, no barrier.  The frame finds its file by binary
// search over a0.  A lane owns V bins per pass (V = 4: one 16-byte load per row, a wave reads 1 KiB contiguous; V = 1 when
// n_mel is no multiple of 4 or the log-mel is not 16-byte aligned), folds the frame's rows per bin first -- a bin has one
// class -- and then the bin into one of twelve registers by twelve predicated selects (no register is indexed by a
// value).  Six xor moves per class reduce over the wave; NaN is the empty maximum and is skipped.  Lanes 0 .. 11 quantise
// with __fsub_rn / __fadd_rn / __fmul_rn -- three roundings, never a fused multiply-add -- and store one byte each.
//
// note_chroma: pianoroll.hip's idiom.  edges_kernel, a lane per note: per harmonic two return-less int32 atomics into the
// file's twelve difference rows (zeroed by the op's memset).  scan_kernel, grid (12, files): an add-scan of the row in
// tiles of 256 with the tiles before in a register, then min(255, .) into the byte [j][c].
//
// paths_kernel: ONE workgroup of 1024 lanes per file and nothing between workgroups.  The skewed column-strip form: lane
// l owns the 16 columns of strip l (a panel is 1024 strips; a longer score is walked panel by panel, the last column of
// a panel going through the workspace), holds their score features (48 dwords) and the row of D above (16 dwords) in
// registers, and at step t computes row i = t - l: cost = three sad_u8, the three-way minimum in the rule's order, two
// bits per choice.  The only value a lane needs from another is D[i][first column - 1]: lane l - 1's last value of the
// step before -- one __shfl_up inside a wave, one LDS word (double-buffered by the step's parity) from wave to wave, so a
// step costs ONE barrier.  The audio row of step t + 1 is loaded during step t.  The strip's 16 choices are one dword,
// stored at [step][lane]: a wave stores 256 contiguous bytes.  The rolling state never leaves the registers, so nothing
// is tiled through LDS and the workspace holds only the choices (2 bits a cell, plus the skew's n_strips - 1 rows) and
// the panel boundary.  Lane 0 then follows the choices from (n - 1, m - 1): dependent loads, one per row of the path (a
// step to the left inside a strip finds its bits in the dword it holds), filling the file's slots from the back; the
// workgroup moves the path to the front, a tile of 1024 at a time (the source of a tile never lies below its
// destination).  Whatever a dword holds, a step stays inside the matrix and the walk ends after n + m - 1 cells.
// Plain vector loads and stores and integer atomics only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "device.h"
#include "mt3_hip.h"

namespace {

constexpr int kClasses = MT3_SYNC_CLASSES;
constexpr int kThreads = 256;                         // the two chroma ops
constexpr int kWaves = kThreads / 64;
constexpr int kLanes = MT3_SYNC_LANES;                // the path op
constexpr int kPathWaves = kLanes / 64;
constexpr int kStrip = MT3_SYNC_STRIP;
constexpr int32_t kNone = INT32_MAX;                  // a predecessor that does not exist: compared, never added to
constexpr int kMaxMel = 4096;
constexpr int kMaxGridY = 65535;
static_assert(kStrip == 16, "a strip's choices are one dword");
static_assert((static_cast<int64_t>(2 * MT3_SYNC_MAX_FRAMES) + kStrip) * 3060 < kNone, "every D stays below kNone");

struct Weights {
  int32_t n, w[MT3_SYNC_HARMONICS];
};

// the larger of two values, NaN skipped: np.fmax
__device__ __forceinline__ float fmax_skip(float a, float b) { return (b == b && (a != a || b > a)) ? b : a; }

// the last file of the table whose `key` is not after `at`
template <typename Key>
__device__ __forceinline__ int file_of(const mt3_sync_file* files, int n_files, int64_t at, Key key) {
  int lo = 0, hi = n_files;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (key(files[mid]) <= at) lo = mid; else hi = mid;
  }
  return lo;
}

template <int V>
__global__ __launch_bounds__(kThreads) void logmel_chroma_kernel(
    const mt3_sync_file* __restrict__ files, int n_files, int64_t a_first, int64_t a_count,
    const float* __restrict__ logmel, int n_mel, const int8_t* __restrict__ bins, int pool, float range, float scale,
    float floor_, uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t local = static_cast<int64_t>(blockIdx.x) * kWaves + wave;
  if (local >= a_count) return;                       // the whole wave; the kernel has no barrier
  const int64_t g = a_first + local;
  const mt3_sync_file f = files[file_of(files, n_files, g, [](const mt3_sync_file& x) { return x.a0; })];
  const int64_t i = g - f.a0;
  if (i < 0 || i >= f.n) return;                      // a frame between two files belongs to none
  const int64_t r0 = i * pool;
  const int64_t r1 = r0 + pool < f.n_frames ? r0 + pool : f.n_frames;

  float v[kClasses];
#pragma unroll
  for (int c = 0; c < kClasses; ++c) v[c] = NAN;
  for (int b0 = lane * V; b0 < n_mel; b0 += 64 * V) {
    float x[V];
#pragma unroll
    for (int k = 0; k < V; ++k) x[k] = NAN;
    for (int64_t r = r0; r < r1; ++r) {
      const float* row = logmel + (f.row0 + r) * n_mel + b0;
      if constexpr (V == 4) {
        const float4 y = *reinterpret_cast<const float4*>(row);
        x[0] = fmax_skip(x[0], y.x), x[1] = fmax_skip(x[1], y.y), x[2] = fmax_skip(x[2], y.z), x[3] = fmax_skip(x[3], y.w);
      } else {
        x[0] = fmax_skip(x[0], row[0]);
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int cls = bins[b0 + k];
#pragma unroll
      for (int c = 0; c < kClasses; ++c)
        if (cls == c) v[c] = fmax_skip(v[c], x[k]);
    }
  }
  float mx = NAN, mine = NAN;
#pragma unroll
  for (int c = 0; c < kClasses; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[c] = fmax_skip(v[c], __shfl_xor(v[c], o));
    mx = fmax_skip(mx, v[c]);
    if (lane == c) mine = v[c];
  }
  if (lane < kClasses) {
    const float t = floorf(__fmul_rn(__fadd_rn(__fsub_rn(mine, mx), range), scale));
    int q = t >= 255.f ? 255 : t >= 0.f ? static_cast<int>(t) : 0;       // NaN: 0
    if (!(mx >= floor_)) q = 0;                       // silent; nothing measured among it
    out[g * kClasses + lane] = static_cast<uint8_t>(q);
  }
}

__global__ __launch_bounds__(kThreads) void edges_kernel(const mt3_sync_file* __restrict__ files, int n_files,
                                                         int64_t note_first, int64_t count,
                                                         const int32_t* __restrict__ d_j0, const int32_t* __restrict__ d_j1,
                                                         const int32_t* __restrict__ d_pitch, Weights w, int32_t* scratch) {
  const int64_t local = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (local >= count) return;
  const int64_t g = note_first + local;
  const mt3_sync_file f = files[file_of(files, n_files, g, [](const mt3_sync_file& x) { return x.first; })];
  if (g < f.first || g - f.first >= f.n_notes) return;
  const int32_t j0 = d_j0[g], j1 = d_j1[g], p = d_pitch[g], m = f.m;
  if (static_cast<uint32_t>(p) > 127u || j0 < 0 || j0 >= m || j1 <= j0 || j1 > m) return;
  int32_t* rows = scratch + f.s0 * kClasses;          // twelve rows of m words
#pragma unroll
  for (int h = 0; h < MT3_SYNC_HARMONICS; ++h) {
    if (h >= w.n || w.w[h] == 0) continue;
    int32_t* row = rows + static_cast<int64_t>((p + mt3s_offset(h)) % kClasses) * m;
    (void)__hip_atomic_fetch_add(row + j0, w.w[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j1 < m) (void)__hip_atomic_fetch_add(row + j1, -w.w[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid (12 classes, files): the row's edges -> the clipped running sums, as bytes [j][class]
__global__ __launch_bounds__(kThreads) void scan_kernel(const mt3_sync_file* __restrict__ files,
                                                        const int32_t* __restrict__ scratch, uint8_t* __restrict__ out) {
  __shared__ int s_sum[2][kWaves];
  const mt3_sync_file f = files[blockIdx.y];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int32_t m = f.m;
  const int32_t* row = scratch + f.s0 * kClasses + static_cast<int64_t>(c) * m;
  int carry = 0, set = 0;                             // uniform over the workgroup
  for (int32_t base = 0; base < m; base += kThreads, set ^= 1) {
    const int32_t j = base + tid;
    const int x = j < m ? row[j] : 0;
    int before, total;                                // the set of the tile before may still be read: this one is the other
    mt3k::block_scan_add<kWaves>(x, s_sum[set], &before, &total);
    const int sum = carry + before + x;
    carry += total;
    if (j < m) out[(f.s0 + j) * kClasses + c] = static_cast<uint8_t>(sum > 255 ? 255 : sum < 0 ? 0 : sum);
  }
}

__global__ __launch_bounds__(kLanes) void paths_kernel(const mt3_sync_file* __restrict__ files,
                                                       const uint8_t* __restrict__ d_a, const uint8_t* __restrict__ d_s,
                                                       uint32_t* work, int32_t* d_path_i, int32_t* d_path_j,
                                                       int32_t* __restrict__ d_path_len, int32_t* __restrict__ d_total) {
  __shared__ int32_t s_hand[2][kPathWaves];
  __shared__ int32_t s_len;
  const mt3_sync_file f = files[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t N = f.n, M = f.m;
  if (N <= 0 || M <= 0) {                             // uniform
    if (tid == 0) d_path_len[blockIdx.x] = 0, d_total[blockIdx.x] = 0;
    return;
  }
  const uint32_t* A = reinterpret_cast<const uint32_t*>(d_a) + f.a0 * 3;      // a row: twelve bytes, three dwords
  const uint32_t* S = reinterpret_cast<const uint32_t*>(d_s) + f.s0 * 3;
  uint32_t* choices = work + f.work0;
  const int64_t strips = (static_cast<int64_t>(M) + kStrip - 1) / kStrip;
  const int64_t n_panels = (strips + kLanes - 1) / kLanes;
  const int64_t panel_words = (static_cast<int64_t>(N) + kLanes - 1) * kLanes;   // of a full panel
  int32_t* boundary = reinterpret_cast<int32_t*>(work + f.work0 + mt3s_workspace_words(N, M) - N);
  // a wave's first lane reads its hand-over word in every step, also in the steps before the wave below has a live row
  // and has written it (the value is not used then): the words start defined
  if (tid < 2 * kPathWaves) s_hand[tid / kPathWaves][tid % kPathWaves] = kNone;
  __syncthreads();

  for (int64_t p = 0; p < n_panels; ++p) {
    const int Sp = static_cast<int>(strips - p * kLanes < kLanes ? strips - p * kLanes : kLanes);
    uint32_t* mine = choices + p * panel_words;
    const bool active = tid < Sp;
    const int64_t jbase = (p * kLanes + tid) * kStrip;
    uint32_t sj[kStrip][3];
    int32_t prev[kStrip];
#pragma unroll
    for (int k = 0; k < kStrip; ++k) {
      const bool in = active && jbase + k < M;        // a column past the score costs something and feeds nothing
      sj[k][0] = in ? S[(jbase + k) * 3] : 0u, sj[k][1] = in ? S[(jbase + k) * 3 + 1] : 0u;
      sj[k][2] = in ? S[(jbase + k) * 3 + 2] : 0u;
      prev[k] = kNone;
    }
    int32_t prevleft = (p == 0 && tid == 0) ? 0 : kNone;       // the corner above (0, 0) makes D[0][0] = cost(0, 0)
    int32_t last = kNone;
    const int32_t steps = N + Sp - 1;
    uint32_t a_next[3] = {0u, 0u, 0u};
    if (tid == 0) a_next[0] = A[0], a_next[1] = A[1], a_next[2] = A[2];
    for (int32_t t = 0; t < steps; ++t) {
      const int32_t i = t - tid;
      const bool live = active && i >= 0 && i < N;
      const uint32_t a0 = a_next[0], a1 = a_next[1], a2 = a_next[2];
      if (active && i + 1 >= 0 && i + 1 < N) {        // the row of the next step, in flight during this one
        const uint32_t* row = A + static_cast<int64_t>(i + 1) * 3;
        a_next[0] = row[0], a_next[1] = row[1], a_next[2] = row[2];
      }
      int32_t left = __shfl_up(last, 1);              // D[i][jbase - 1]: the lane before, one step ago
      if (lane == 0) left = wave > 0 ? s_hand[(t + 1) & 1][wave - 1] : kNone;
      if (tid == 0 && p > 0 && live) left = boundary[i];
      if (live) {
        int32_t diag = prevleft, l = left;
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < kStrip; ++k) {
          uint32_t c = __builtin_amdgcn_sad_u8(a0, sj[k][0], 0u);
          c = __builtin_amdgcn_sad_u8(a1, sj[k][1], c);
          c = __builtin_amdgcn_sad_u8(a2, sj[k][2], c);
          const int32_t up = prev[k];
          int32_t best = diag;
          uint32_t ch = 0;
          if (up < best) best = up, ch = 1;
          if (l < best) best = l, ch = 2;
          const int32_t cur = best + static_cast<int32_t>(c);
          bits |= ch << (2 * k);
          diag = up, l = cur, prev[k] = cur;
          if (i == N - 1 && jbase + k == M - 1) d_total[blockIdx.x] = cur;
        }
        prevleft = left, last = l;
        mine[static_cast<int64_t>(t) * Sp + tid] = bits;
        if (tid == kLanes - 1 && p + 1 < n_panels) boundary[i] = l;
      }
      if (lane == 63) s_hand[t & 1][wave] = last;
      __syncthreads();                                // the step's hand-over words, choices and boundary are written
    }
  }

  // ---- the path, from its end: one lane, dependent loads
  const int64_t cap = static_cast<int64_t>(N) + M - 1;
  int32_t* path_i = d_path_i + f.path0;
  int32_t* path_j = d_path_j + f.path0;
  if (tid == 0) {
    int32_t i = N - 1, j = M - 1;
    int64_t k = cap, held = -1;
    uint32_t word = 0;
    while (k > 0) {
      --k;
      path_i[k] = i, path_j[k] = j;
      if (i == 0 && j == 0) break;
      const int64_t strip = j / kStrip, p = strip / kLanes, l = strip % kLanes;
      const int64_t Sp = strips - p * kLanes < kLanes ? strips - p * kLanes : kLanes;
      const int64_t at = p * panel_words + (static_cast<int64_t>(i) + l) * Sp + l;
      if (at != held) word = choices[at], held = at;
      const uint32_t ch = (word >> (2 * (j % kStrip))) & 3u;
      // a stored choice always has its predecessor; whatever is read, the step stays inside the matrix
      if (ch == 0 && i > 0 && j > 0) --i, --j;
      else if (j == 0 || (ch != 2 && i > 0)) --i;
      else --j;
    }
    s_len = static_cast<int32_t>(cap - k);
    d_path_len[blockIdx.x] = static_cast<int32_t>(cap - k);
  }
  __syncthreads();
  const int64_t len = s_len, off = cap - len;
  if (off == 0) return;                               // uniform
  for (int64_t base = 0; base < len; base += kLanes) {
    const int64_t at = base + tid;
    int32_t vi = 0, vj = 0;
    if (at < len) vi = path_i[off + at], vj = path_j[off + at];
    __syncthreads();                                  // the tile is read before any of it is overwritten
    if (at < len) path_i[at] = vi, path_j[at] = vj;
  }
}

int check_table(const std::string& who, const mt3_sync_file* h_files, const mt3_sync_file* d_files, int32_t n_files) {
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (n_files > 0 && (!h_files || !d_files)) return mt3::fail(MT3_ERR_INVALID, who + "null file table (host or device)");
  return MT3_OK;
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

// [at, at + count) inside [0, total] and not before `*end`, which moves to its end
const char* check_range(int64_t at, int64_t count, int64_t total, int64_t* end) {
  if (at < 0 || count < 0 || at > total || count > total - at) return "inside";
  if (at < *end) return "order";
  *end = at + count;
  return nullptr;
}

int range_error(const std::string& who, const char* what, const std::string& kind, const std::string& array) {
  if (what[0] == 'i') return mt3::fail(MT3_ERR_INVALID, who + "a file's " + kind + " range must lie inside " + array);
  return mt3::fail(MT3_ERR_INVALID, who + kind + " ranges overlap or are out of order");
}

// n and m of every file within the limits of the path op
int check_sizes(const std::string& who, const mt3_sync_file* h_files, int32_t n_files) {
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_sync_file& f = h_files[i];
    if (f.n < 0 || f.m < 0 || f.n > MT3_SYNC_MAX_FRAMES || f.m > MT3_SYNC_MAX_FRAMES)
      return mt3::fail(MT3_ERR_INVALID, who + "n and m must be 0 .. 2^18 feature frames");
    if (static_cast<int64_t>(f.n) * f.m > MT3_SYNC_MAX_CELLS)
      return mt3::fail(MT3_ERR_INVALID, who + "n * m must not exceed 2^31 cells (there is no band constraint)");
  }
  return MT3_OK;
}

}  // namespace

extern "C" int64_t mt3_sync_workspace_bytes(const mt3_sync_file* h_files, int32_t n_files) {
  const std::string who = "mt3_sync_workspace_bytes: ";
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative"), -1;
  if (n_files > 0 && !h_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table"), -1;
  if (check_sizes(who, h_files, n_files)) return -1;
  int64_t words = 0;
  for (int32_t i = 0; i < n_files; ++i) words += mt3s_workspace_words(h_files[i].n, h_files[i].m);
  return words * 4;
}

extern "C" int mt3_op_logmel_chroma(const float* d_logmel, int64_t n_rows, int32_t n_mel, const mt3_sync_file* h_files,
                                    const mt3_sync_file* d_files, int32_t n_files, const int8_t* d_bins, int32_t pool,
                                    float range, float floor, uint8_t* d_a, int64_t total_a, void* stream) {
  const std::string who = "mt3_op_logmel_chroma: ";
  if (pool < 1 || pool > MT3_SYNC_MAX_POOL) return mt3::fail(MT3_ERR_INVALID, who + "pool must be 1 .. 16 rows");
  if (n_mel < 1 || n_mel > kMaxMel) return mt3::fail(MT3_ERR_INVALID, who + "n_mel must be 1 .. 4096");
  if (!(std::isfinite(range) && range > 0.f)) return mt3::fail(MT3_ERR_INVALID, who + "range must be finite and > 0");
  if (floor != floor) return mt3::fail(MT3_ERR_INVALID, who + "floor must not be NaN");
  if (n_rows < 0 || total_a < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_rows and total_a must not be negative");
  if (const int rc = check_table(who, h_files, d_files, n_files)) return rc;
  if (n_files == 0) return MT3_OK;
  int64_t a_end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_sync_file& f = h_files[i];
    if (f.n_frames < 0 || f.n < 0 || f.n != (static_cast<int64_t>(f.n_frames) + pool - 1) / pool)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's n must be ceil(n_frames / pool)");
    int64_t rows = 0;                                 // rows are only read: two files may share them
    if (const char* e = check_range(f.row0, f.n_frames, n_rows, &rows)) return range_error(who, e, "row", "[0, n_rows]");
    if (const char* e = check_range(f.a0, f.n, total_a, &a_end)) return range_error(who, e, "audio feature", "[0, total_a]");
  }
  const int64_t a_first = h_files[0].a0, a_count = a_end - a_first;
  if (a_count == 0) return MT3_OK;
  if (!d_logmel || !d_bins || !d_a) return mt3::fail(MT3_ERR_INVALID, who + "null log-mel, bins or output");
  if (misaligned(d_logmel)) return mt3::fail(MT3_ERR_INVALID, who + "the log-mel must be 4-byte aligned");
  const int64_t groups = (a_count + kWaves - 1) / kWaves;
  if (groups > INT32_MAX) return mt3::fail(MT3_ERR_INVALID, who + "too many feature frames for one launch");

  hipStream_t s = static_cast<hipStream_t>(stream);
  const float scale = static_cast<float>(255.0 / static_cast<double>(range));
  const bool wide = n_mel % 4 == 0 && (reinterpret_cast<uintptr_t>(d_logmel) & 15) == 0;
  if (wide)
    hipLaunchKernelGGL(logmel_chroma_kernel<4>, dim3(static_cast<uint32_t>(groups)), dim3(kThreads), 0, s, d_files,
                       static_cast<int>(n_files), a_first, a_count, d_logmel, static_cast<int>(n_mel), d_bins,
                       static_cast<int>(pool), range, scale, floor, d_a);
  else
    hipLaunchKernelGGL(logmel_chroma_kernel<1>, dim3(static_cast<uint32_t>(groups)), dim3(kThreads), 0, s, d_files,
                       static_cast<int>(n_files), a_first, a_count, d_logmel, static_cast<int>(n_mel), d_bins,
                       static_cast<int>(pool), range, scale, floor, d_a);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}

extern "C" int mt3_op_note_chroma(const int32_t* d_j0, const int32_t* d_j1, const int32_t* d_pitch, int64_t n_notes,
                                  const mt3_sync_file* h_files, const mt3_sync_file* d_files, int32_t n_files,
                                  const int32_t* h_weights, int32_t n_harmonics, int32_t* d_scratch, uint8_t* d_s,
                                  int64_t total_s, void* stream) {
  const std::string who = "mt3_op_note_chroma: ";
  if (n_notes < 0 || total_s < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes and total_s must not be negative");
  if (n_harmonics < 1 || n_harmonics > MT3_SYNC_HARMONICS || !h_weights)
    return mt3::fail(MT3_ERR_INVALID, who + "1 .. 6 harmonic weights");
  Weights w{};
  w.n = n_harmonics;
  for (int h = 0; h < n_harmonics; ++h) {
    if (h_weights[h] < 0 || h_weights[h] > 255) return mt3::fail(MT3_ERR_INVALID, who + "a harmonic weight must be 0 .. 255");
    w.w[h] = h_weights[h];
  }
  if (total_s > INT64_MAX / 64) return mt3::fail(MT3_ERR_INVALID, who + "total_s is too large");
  if (const int rc = check_table(who, h_files, d_files, n_files)) return rc;
  if (n_files == 0) return MT3_OK;
  int64_t note_end = 0, s_end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_sync_file& f = h_files[i];
    if (f.m > MT3_SYNC_MAX_FRAMES) return mt3::fail(MT3_ERR_INVALID, who + "m must be 0 .. 2^18 feature frames");
    if (const char* e = check_range(f.first, f.n_notes, n_notes, &note_end)) return range_error(who, e, "note", "[0, n_notes]");
    if (const char* e = check_range(f.s0, f.m, total_s, &s_end)) return range_error(who, e, "score feature", "[0, total_s]");
  }
  const int64_t s_first = h_files[0].s0, note_first = h_files[0].first, count = note_end - note_first;
  if (s_end == s_first) return MT3_OK;
  if (!d_scratch || !d_s) return mt3::fail(MT3_ERR_INVALID, who + "null scratch or output");
  if (misaligned(d_scratch)) return mt3::fail(MT3_ERR_INVALID, who + "the scratch must be 4-byte aligned");
  if (count > 0 && (!d_j0 || !d_j1 || !d_pitch)) return mt3::fail(MT3_ERR_INVALID, who + "null note column (j0, j1 or pitch)");
  const int64_t blocks = (count + kThreads - 1) / kThreads;
  if (blocks > INT32_MAX) return mt3::fail(MT3_ERR_INVALID, who + "too many notes for one launch");

  hipStream_t s = static_cast<hipStream_t>(stream);
  MT3_HIP_CHECK(hipMemsetAsync(d_scratch + s_first * kClasses, 0,
                               static_cast<size_t>(s_end - s_first) * kClasses * sizeof(int32_t), s));
  if (count > 0) {
    hipLaunchKernelGGL(edges_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kThreads), 0, s, d_files,
                       static_cast<int>(n_files), note_first, count, d_j0, d_j1, d_pitch, w, d_scratch);
    MT3_HIP_CHECK(hipGetLastError());
  }
  for (int32_t f0 = 0; f0 < n_files; f0 += kMaxGridY) {                  // (the grid's second dimension ends at 65535)
    const int n = n_files - f0 < kMaxGridY ? n_files - f0 : kMaxGridY;
    hipLaunchKernelGGL(scan_kernel, dim3(kClasses, static_cast<uint32_t>(n)), dim3(kThreads), 0, s, d_files + f0, d_scratch,
                       d_s);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}

extern "C" int mt3_op_sync_paths(const uint8_t* d_a, int64_t total_a, const uint8_t* d_s, int64_t total_s,
                                 const mt3_sync_file* h_files, const mt3_sync_file* d_files, int32_t n_files,
                                 void* d_workspace, int64_t workspace_bytes, int32_t* d_path_i, int32_t* d_path_j,
                                 int64_t total_path, int32_t* d_path_len, int32_t* d_total, void* stream) {
  const std::string who = "mt3_op_sync_paths: ";
  if (total_a < 0 || total_s < 0 || total_path < 0 || workspace_bytes < 0)
    return mt3::fail(MT3_ERR_INVALID, who + "total_a, total_s, total_path and workspace_bytes must not be negative");
  if (const int rc = check_table(who, h_files, d_files, n_files)) return rc;
  if (n_files == 0) return MT3_OK;
  if (const int rc = check_sizes(who, h_files, n_files)) return rc;
  int64_t a_end = 0, s_end = 0, path_end = 0, work_end = 0;
  bool any = false;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_sync_file& f = h_files[i];
    if (const char* e = check_range(f.a0, f.n, total_a, &a_end)) return range_error(who, e, "audio feature", "[0, total_a]");
    if (const char* e = check_range(f.s0, f.m, total_s, &s_end)) return range_error(who, e, "score feature", "[0, total_s]");
    if (const char* e = check_range(f.path0, MT3_SYNC_PATH_CAPACITY(f.n, f.m), total_path, &path_end))
      return range_error(who, e, "path", "[0, total_path]");
    any = any || (f.n > 0 && f.m > 0);
  }
  if (!d_path_len || !d_total) return mt3::fail(MT3_ERR_INVALID, who + "null path_len or total");
  if (any) {
    if (!d_a || !d_s || !d_path_i || !d_path_j) return mt3::fail(MT3_ERR_INVALID, who + "null features or path");
    if (misaligned(d_a) || misaligned(d_s)) return mt3::fail(MT3_ERR_INVALID, who + "the features must be 4-byte aligned");
    if (!d_workspace) return mt3::fail(MT3_ERR_INVALID, who + "null workspace");
    if (misaligned(d_workspace)) return mt3::fail(MT3_ERR_INVALID, who + "the workspace must be 4-byte aligned");
    for (int32_t i = 0; i < n_files; ++i) {
      const mt3_sync_file& f = h_files[i];
      if (const char* e = check_range(f.work0, mt3s_workspace_words(f.n, f.m), workspace_bytes / 4, &work_end)) {
        if (e[0] == 'i')
          return mt3::fail(MT3_ERR_INVALID, who + "the workspace is too short for a file's words (mt3_sync_workspace_bytes)");
        return range_error(who, e, "workspace", "");
      }
    }
  }

  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(paths_kernel, dim3(static_cast<uint32_t>(n_files)), dim3(kLanes), 0, s, d_files, d_a, d_s,
                     static_cast<uint32_t*>(d_workspace), d_path_i, d_path_j, d_path_len, d_total);
  MT3_HIP_CHECK(hipGetLastError());
  return MT3_OK;
}
