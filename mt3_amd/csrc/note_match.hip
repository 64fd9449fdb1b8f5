// Maximum note matching for gfx950: every (reference notes, estimated notes, rule) problem of a job -> the size of a
// maximum bipartite matching and the matching itself (mt3_op_match_notes).  The rule: include/mt3_hip.h, "note matching".
//
// One workgroup of 256 lanes per problem, 64 problems per launch (their tables ride in the kernel arguments), the
// launches of a job one after the other on the stream: at most 64 workgroups are in flight, a quarter of the CUs.  The
// edges are never stored: edge(i, j) is a dozen float64 operations on six loaded values and is re-evaluated
// wherever it is needed, over reference i's window [lo_i, hi_i) of the onset-sorted estimates (two binary searches, kept
// in the state).  Hopcroft-Karp in its level-synchronous form:
//   0. warm start (optional): mate_ref[i] is kept where it is inside the window, passes the edge rule and wins the
//      compare-and-swap on mate_est -- anything else becomes -1, so a bad warm start costs matches, never safety;
//   1. greedy: each free reference claims the first free estimate of its window by compare-and-swap on mate_est;
//   2. BFS: level 0 = the free references; level d + 1 = the mates of the estimates adjacent to level d that have no
//      level yet.  Every level is one strided sweep over the references (no queue), two flags in LDS: `found` (a level
//      touched a free estimate: stop, augment) and `next` (the level added a reference: go on).  Neither: maximum;
//   3. walk: one lane per free reference goes depth-first down the levels.  The path is held in `parent` and `cursor`
//      (per reference, in the state -- paths can be hundreds of vertices long, so there is no per-lane stack); an
//      estimate is entered only by the lane that wins the compare-and-swap on `claim`, so a reference other than a root
//      is reached only through its mate and belongs to one lane, and paths are vertex-disjoint.  A walk that reaches
//      a free estimate flips the mates along its path;
//   4. again from 2.
// Termination.  A cursor only advances within a phase and a walk steps back once per step down, so a walk ends after at
// most (window sizes + references) steps.  A BFS level that adds no reference ends the BFS, so it has at most n_ref + 1
// levels.  Concurrent walks can block each other (each holds the estimate the other needs); a phase whose BFS found a
// free estimate and whose walks augmented nothing repeats the walk with ONE lane and fresh claims, which is the
// sequential algorithm and finds a path.  Every phase but the last therefore adds a match, and there are at most
// min(n_ref, n_est) + 1 phases; the loop counts them, and past that bound writes -1 as the problem's count and returns.
// Within a phase a cell of mate_ref, mate_est, cursor or parent is written by one lane only (the owner of the claim);
// phases and steps are separated by workgroup barriers.  Plain vector loads, stores and atomics only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "mt3_hip.h"

#pragma clang fp contract(off)          // every product, difference and quotient of the rule is rounded on its own

namespace {

constexpr int kThreads = 256;
constexpr int kPerLaunch = 64;                       // problems whose tables fit one launch's arguments
constexpr int kMaxRules = MT3_NOTE_MATCH_MAX_RULES;
constexpr int kRefArrays = 6, kEstArrays = 2;        // state words per reference / per estimate

struct Rule {
  double onset_tol, pitch_tol, offset_ratio, offset_min_tol;
  int32_t strict, use_offset;
};

struct ProblemTable {                                // 2304 + 640 bytes by value: under 3 KiB
  int64_t ref0[kPerLaunch], est0[kPerLaunch], state0[kPerLaunch];
  int32_t n_ref[kPerLaunch], n_est[kPerLaunch], rule[kPerLaunch];
  Rule rules[kMaxRules];
};
static_assert(sizeof(ProblemTable) <= 3072, "the tables of one launch stay within 3 KiB");

// np.around(|a - b|, 6): one product, rint, one quotient
__device__ __forceinline__ double rounded_distance(double a, double b) { return rint(fabs(a - b) * 1e6) / 1e6; }

__device__ __forceinline__ bool within(double d, double tol, int strict) { return strict ? d < tol : d <= tol; }

struct Notes {                                       // one problem's view of the job's arrays
  const double* r_on;
  const double* r_off;
  const double* r_l2;
  const double* e_on;
  const double* e_off;
  const double* e_l2;
};

struct RefNote {
  double on, off, l2;
};

__device__ __forceinline__ RefNote load_ref(const Notes& n, int i) { return {n.r_on[i], n.r_off[i], n.r_l2[i]}; }

// metrics._hit_pairs' predicate for reference note `r` and estimate j (j inside r's window)
__device__ __forceinline__ bool edge(const Notes& n, const Rule& k, const RefNote& r, int j) {
  if (!within(rounded_distance(r.on, n.e_on[j]), k.onset_tol, k.strict)) return false;
  double cents = fabs(1200.0 * (r.l2 - n.e_l2[j]));
  if (cents != cents) cents = 0.0;                   // nan_to_num: log2(0) - log2(0)
  if (!within(cents, k.pitch_tol, k.strict)) return false;
  if (k.use_offset) {
    const double a = k.offset_ratio * (r.off - r.on);
    const double tol = a > k.offset_min_tol ? a : k.offset_min_tol;
    if (!within(rounded_distance(r.off, n.e_off[j]), tol, k.strict)) return false;
  }
  return true;
}

// first j in [0, n) with a[j] >= x (right == false) or a[j] > x (right == true): np.searchsorted; at most 32 halvings
__device__ __forceinline__ int search(const double* a, int n, double x, bool right) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const double v = a[mid];
    if (right ? v <= x : v < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int32_t peek(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void put(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ bool take(int32_t* p, int32_t expected, int32_t desired) {
  return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct State {
  int32_t* mate_ref;                                 // [n_ref] estimate of reference i, or -1 (the output)
  int32_t* lo;                                       // [n_ref] window [lo, hi) of reference i
  int32_t* hi;
  int32_t* level;                                    // [n_ref] BFS level, -1: none
  int32_t* cursor;                                   // [n_ref] next estimate the walk tries
  int32_t* parent;                                   // [n_ref] the reference the walk came from
  int32_t* mate_est;                                 // [n_est]
  int32_t* claim;                                    // [n_est] entered by a walk in this phase
};

// the walk from free reference `root`: true when it reached a free estimate and flipped its path.  Every iteration
// advances a cursor or steps back to a parent.
__device__ bool walk(const Notes& n, const Rule& k, const State& s, int root, int n_ref) {
  int cur = root;
  RefNote r = load_ref(n, cur);
  int lvl = 0;                                       // level[cur]
  for (;;) {
    const int j = s.cursor[cur];
    if (j >= s.hi[cur]) {                            // nothing left below cur
      if (cur == root) return false;
      cur = s.parent[cur];
      r = load_ref(n, cur);
      --lvl;
      continue;
    }
    s.cursor[cur] = j + 1;
    if (!edge(n, k, r, j)) continue;
    int32_t m = peek(s.mate_est + j);
    if (m >= 0 && s.level[m] != lvl + 1) continue;   // not a step down the levels: leave it to whoever it serves
    if (!take(s.claim + j, 0, 1)) continue;          // another walk is there
    m = peek(s.mate_est + j);                        // ours now: nobody else writes it in this phase
    if (m < 0) {                                     // free: flip the path back to the root, at most n_ref steps
      int e = j, v = cur;
      for (int step = 0; step < n_ref; ++step) {
        const int32_t before = s.mate_ref[v];
        s.mate_ref[v] = e;
        put(s.mate_est + e, v);                      // other walks peek at this cell before they try the claim
        if (v == root) break;
        e = before;
        v = s.parent[v];
      }
      return true;
    }
    if (s.level[m] != lvl + 1) continue;
    s.parent[m] = cur;
    cur = m;
    r = load_ref(n, cur);
    ++lvl;
  }
}

__global__ __launch_bounds__(kThreads) void match_kernel(ProblemTable t, const double* __restrict__ onset,
                                                         const double* __restrict__ offset,
                                                         const double* __restrict__ log2_pitch, int32_t* workspace,
                                                         int32_t warm_start, int32_t* __restrict__ matched) {
  __shared__ int s_found, s_next, s_augmented, s_count;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n_ref = t.n_ref[p], n_est = t.n_est[p];
  const Rule k = t.rules[t.rule[p]];
  int32_t* base = workspace + t.state0[p];
  State s;
  s.mate_ref = base, s.lo = base + n_ref, s.hi = base + 2 * static_cast<int64_t>(n_ref);
  s.level = base + 3 * static_cast<int64_t>(n_ref), s.cursor = base + 4 * static_cast<int64_t>(n_ref);
  s.parent = base + 5 * static_cast<int64_t>(n_ref);
  s.mate_est = base + kRefArrays * static_cast<int64_t>(n_ref), s.claim = s.mate_est + n_est;
  Notes n;
  n.r_on = onset + t.ref0[p], n.r_off = offset + t.ref0[p], n.r_l2 = log2_pitch + t.ref0[p];
  n.e_on = onset + t.est0[p], n.e_off = offset + t.est0[p], n.e_l2 = log2_pitch + t.est0[p];

  if (n_ref == 0 || n_est == 0) {                    // an empty side: nothing matches
    for (int i = tid; i < n_ref; i += kThreads) s.mate_ref[i] = -1;
    if (tid == 0) matched[p] = 0;
    return;
  }

  // windows, and the warm start or the empty matching
  if (tid == 0) s_count = 0;
  for (int j = tid; j < n_est; j += kThreads) s.mate_est[j] = -1, s.claim[j] = 0;
  const double margin = k.onset_tol + 1e-6;
  for (int i = tid; i < n_ref; i += kThreads) {
    const double on = n.r_on[i];
    s.lo[i] = search(n.e_on, n_est, on - margin, false);
    s.hi[i] = search(n.e_on, n_est, on + margin, true);
  }
  __syncthreads();
  for (int i = tid; i < n_ref; i += kThreads) {
    const int32_t j = warm_start ? s.mate_ref[i] : -1;
    bool keep = j >= s.lo[i] && j < s.hi[i];         // inside the window, so inside [0, n_est)
    keep = keep && edge(n, k, load_ref(n, i), j) && take(s.mate_est + j, -1, i);
    if (!keep) s.mate_ref[i] = -1;
  }
  __syncthreads();
  // 1. greedy
  for (int i = tid; i < n_ref; i += kThreads) {
    if (s.mate_ref[i] >= 0) continue;
    const RefNote r = load_ref(n, i);
    const int hi = s.hi[i];
    for (int j = s.lo[i]; j < hi; ++j)
      if (peek(s.mate_est + j) < 0 && edge(n, k, r, j) && take(s.mate_est + j, -1, i)) {
        s.mate_ref[i] = j;
        break;
      }
  }
  __syncthreads();

  const int max_phases = (n_ref < n_est ? n_ref : n_est) + 1;
  bool maximum = false;
  for (int phase = 0; phase < max_phases; ++phase) {
    if (tid == 0) s_found = 0, s_augmented = 0;
    for (int i = tid; i < n_ref; i += kThreads) s.level[i] = s.mate_ref[i] < 0 ? 0 : -1, s.cursor[i] = s.lo[i];
    for (int j = tid; j < n_est; j += kThreads) s.claim[j] = 0;
    // 2. BFS, one sweep per level; a level that adds no reference is the last, so at most n_ref + 1 sweeps
    bool found = false;
    for (int d = 0; d <= n_ref; ++d) {
      if (tid == 0) s_next = 0;
      __syncthreads();
      for (int i = tid; i < n_ref; i += kThreads) {
        if (s.level[i] != d) continue;
        const RefNote r = load_ref(n, i);
        const int hi = s.hi[i];
        for (int j = s.lo[i]; j < hi; ++j) {
          if (!edge(n, k, r, j)) continue;
          const int32_t m = s.mate_est[j];
          if (m < 0) {
            s_found = 1;
          } else if (peek(s.level + m) < 0) {        // lanes that meet here all write d + 1
            put(s.level + m, d + 1);
            s_next = 1;
          }
        }
      }
      __syncthreads();
      found = s_found != 0;
      const bool next = s_next != 0;
      __syncthreads();                               // both flags read before lane 0 clears s_next again
      if (found || !next) break;
    }
    if (!found) {
      maximum = true;
      break;
    }
    // 3. walks, one lane per free reference
    for (int i = tid; i < n_ref; i += kThreads)
      if (s.level[i] == 0 && walk(n, k, s, i, n_ref)) atomicAdd(&s_augmented, 1);
    __syncthreads();
    if (s_augmented == 0) {                          // the walks blocked each other: one lane, fresh claims
      for (int i = tid; i < n_ref; i += kThreads) s.cursor[i] = s.lo[i];
      for (int j = tid; j < n_est; j += kThreads) s.claim[j] = 0;
      __syncthreads();
      if (tid == 0)
        for (int i = 0; i < n_ref; ++i)
          if (s.level[i] == 0 && walk(n, k, s, i, n_ref)) s_augmented = 1;
    }
    __syncthreads();
  }

  int mine = 0;
  for (int i = tid; i < n_ref; i += kThreads) mine += s.mate_ref[i] >= 0;
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (tid == 0) matched[p] = maximum ? s_count : -1; // -1: the phase bound was passed, which the argument above excludes
}

bool finite_tolerance(double v) { return std::isfinite(v) && v >= 0.0; }

}  // namespace

extern "C" int64_t mt3_note_match_state_words(int32_t n_ref, int32_t n_est) {
  if (n_ref < 0 || n_est < 0) return -1;
  return static_cast<int64_t>(kRefArrays) * n_ref + static_cast<int64_t>(kEstArrays) * n_est;
}

extern "C" int mt3_op_match_notes(const double* d_onset, const double* d_offset, const double* d_log2_pitch,
                                  int64_t n_notes, int32_t n_problems, const mt3_match_problem* h_problems,
                                  int32_t n_rules, const mt3_match_rule* h_rules, int32_t* d_workspace,
                                  int64_t workspace_words, int32_t warm_start, int32_t* d_matched, void* stream) {
  const std::string who = "mt3_op_match_notes: ";
  if (n_problems < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_problems must not be negative");
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (n_rules < 0 || n_rules > kMaxRules)
    return mt3::fail(MT3_ERR_INVALID, who + "n_rules must be 0 .. " + std::to_string(kMaxRules));
  if (workspace_words < 0) return mt3::fail(MT3_ERR_INVALID, who + "workspace_words must not be negative");
  if (n_rules > 0 && !h_rules) return mt3::fail(MT3_ERR_INVALID, who + "null rule table");
  for (int32_t i = 0; i < n_rules; ++i) {
    const mt3_match_rule& r = h_rules[i];
    if (!finite_tolerance(r.onset_tolerance) || !finite_tolerance(r.pitch_tolerance) ||
        !finite_tolerance(r.offset_min_tolerance))
      return mt3::fail(MT3_ERR_INVALID, who + "a tolerance is negative or not finite");
    if (!finite_tolerance(r.offset_ratio) && r.offset_ratio != MT3_NOTE_MATCH_NO_OFFSET)
      return mt3::fail(MT3_ERR_INVALID, who + "offset_ratio is negative or not finite (and not MT3_NOTE_MATCH_NO_OFFSET)");
  }
  if (n_problems == 0) return MT3_OK;
  if (!h_problems) return mt3::fail(MT3_ERR_INVALID, who + "null problem table");
  if (!d_matched) return mt3::fail(MT3_ERR_INVALID, who + "null d_matched");
  if (n_notes > 0 && (!d_onset || !d_offset || !d_log2_pitch)) return mt3::fail(MT3_ERR_INVALID, who + "null note array");
  int64_t state_end = 0;
  for (int32_t i = 0; i < n_problems; ++i) {
    const mt3_match_problem& q = h_problems[i];
    if (q.n_ref < 0 || q.n_est < 0) return mt3::fail(MT3_ERR_INVALID, who + "a negative note count");
    if (q.ref0 < 0 || q.ref0 > n_notes - q.n_ref || q.est0 < 0 || q.est0 > n_notes - q.n_est)
      return mt3::fail(MT3_ERR_INVALID, who + "a note range must lie inside [0, n_notes]");
    if (q.rule < 0 || q.rule >= n_rules) return mt3::fail(MT3_ERR_INVALID, who + "a rule index out of range");
    const int64_t words = mt3_note_match_state_words(q.n_ref, q.n_est);
    if (q.state0 < state_end) return mt3::fail(MT3_ERR_INVALID, who + "state ranges overlap or are out of order");
    if (q.state0 > workspace_words - words) return mt3::fail(MT3_ERR_INVALID, who + "a state range ends past workspace_words");
    state_end = q.state0 + words;
  }
  if (state_end > 0 && !d_workspace) return mt3::fail(MT3_ERR_INVALID, who + "null d_workspace");

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t p0 = 0; p0 < n_problems; p0 += kPerLaunch) {
    const int n = n_problems - p0 < kPerLaunch ? n_problems - p0 : kPerLaunch;
    ProblemTable t{};
    for (int j = 0; j < n; ++j) {
      const mt3_match_problem& q = h_problems[p0 + j];
      t.ref0[j] = q.ref0, t.est0[j] = q.est0, t.state0[j] = q.state0;
      t.n_ref[j] = q.n_ref, t.n_est[j] = q.n_est, t.rule[j] = q.rule;
    }
    for (int j = 0; j < n_rules; ++j) {
      const mt3_match_rule& r = h_rules[j];
      const bool use_offset = r.offset_ratio != MT3_NOTE_MATCH_NO_OFFSET;
      t.rules[j] = {r.onset_tolerance, r.pitch_tolerance, use_offset ? r.offset_ratio : 0.0, r.offset_min_tolerance,
                    r.strict != 0, use_offset};
    }
    hipLaunchKernelGGL(match_kernel, dim3(static_cast<uint32_t>(n)), dim3(kThreads), 0, s, t, d_onset, d_offset,
                       d_log2_pitch, d_workspace, warm_start, d_matched + p0);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}
