// Note consensus for gfx950: the transcriptions of a file by several voters -> the notes a quorum of them agrees on, and
// for every note the number of voters that have it (mt3_op_note_consensus).  The rule: include/mt3_hip.h, "note
// consensus"; its numpy statement: mt3_amd/consensus.py, consensus_reference.
//
// One workgroup of 256 lanes per file, 64 files per launch (their table rides in the kernel arguments).  The file's notes
// lie sorted by (key, onset, ...), so a cluster is a run [a, b) and everything a note needs is inside its run:
//   1. tiles of 256 notes, one per lane: head flag (one float64 difference), block_scan_add carried from tile to tile ->
//      the note's cluster number c, into scratch; a head writes its position as the start of cluster c;
//   2. tiles again: the lane of a head walks its run and ORs the voter bits, popcount = votes; kept = votes >= min_votes;
//      block_scan_add of the kept flags, carried, gives the cluster's place in the output (-1: dropped);
//   3. every note of a kept cluster counts the members whose (offset, position) and (velocity, position) lie below its
//      own; the one of rank (m - 1) / 2 writes that field of the emitted note, the one AT position a + (m - 1) / 2 writes
//      onset, key, votes and members.  Ranks under a total order are a permutation of 0 .. m - 1: one writer per word.
// A run's bounds come from the scan alone: start[c] < start[c + 1] <= n whatever the columns hold, so unsorted input gives
// other notes, never an index outside the file.  Scratch words written in one pass are read in the next by other lanes of
// the same workgroup, after a __syncthreads.  Plain vector loads and stores only, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "common.h"
#include "device.h"
#include "mt3_hip.h"

#pragma clang fp contract(off)          // the one difference of the rule is rounded on its own

namespace {

constexpr int kTile = MT3_CONSENSUS_TILE;            // notes per tile = lanes of the workgroup
constexpr int kWaves = kTile / 64;
constexpr int kPerLaunch = 64;                       // files whose table fits one launch's arguments

struct ConsensusTable {                              // 512 + 256 + 256 bytes by value
  int64_t first[kPerLaunch];
  int32_t n_notes[kPerLaunch], min_votes[kPerLaunch];
};
static_assert(sizeof(ConsensusTable) <= 1024, "the table of one launch stays within 1 KiB");

__global__ __launch_bounds__(kTile) void consensus_kernel(
    ConsensusTable t, const double* __restrict__ d_onset, const double* __restrict__ d_offset,
    const int32_t* __restrict__ d_key, const int32_t* __restrict__ d_velocity, const int32_t* __restrict__ d_voter,
    int64_t n_job, double tolerance, double* __restrict__ d_out_onset, double* __restrict__ d_out_offset,
    int32_t* __restrict__ d_out_key, int32_t* __restrict__ d_out_velocity, int32_t* __restrict__ d_out_votes,
    int32_t* __restrict__ d_out_members, int32_t* __restrict__ d_note_votes, int32_t* __restrict__ d_counts,
    int32_t* d_scratch) {
  __shared__ int s_add[kWaves];
  const int tid = threadIdx.x;
  const int64_t first = t.first[blockIdx.x];
  const int32_t n = t.n_notes[blockIdx.x];
  const int32_t min_votes = t.min_votes[blockIdx.x];
  const double* onset = d_onset + first;
  const double* offset = d_offset + first;
  const int32_t* key = d_key + first;
  const int32_t* velocity = d_velocity + first;
  const int32_t* voter = d_voter + first;
  int32_t* cluster_of = d_scratch + first;             // [n] per note: its cluster's number within the file
  int32_t* start_of = d_scratch + n_job + first;       // [clusters] per cluster: its first note
  int32_t* votes_of = d_scratch + 2 * n_job + first;   // [clusters]
  int32_t* place_of = d_scratch + 3 * n_job + first;   // [clusters] where the emitted note goes, -1: dropped

  // ---- 1: cluster numbers and cluster starts
  int32_t clusters = 0;                                // so far; uniform
  for (int64_t t0 = 0; t0 < n; t0 += kTile) {
    const int64_t i = t0 + tid;
    int head = 0;
    if (i < n) head = i == 0 || key[i] != key[i - 1] || onset[i] - onset[i - 1] > tolerance;
    int before, total;
    mt3k::block_scan_add<kWaves>(head, s_add, &before, &total);
    if (i < n) {
      const int32_t c = clusters + before + head - 1;  // note 0 is a head: c >= 0
      cluster_of[i] = c;
      if (head) start_of[c] = static_cast<int32_t>(i);
    }
    clusters += total;
    __syncthreads();                                   // s_add is free again; after the last tile: scratch is written
  }

  // ---- 2: votes of every cluster, and the place of the kept ones
  int32_t kept_so_far = 0;                             // uniform
  for (int64_t t0 = 0; t0 < n; t0 += kTile) {
    const int64_t i = t0 + tid;
    int32_t c = 0;
    int keep = 0;
    bool head = false;
    if (i < n) {
      c = cluster_of[i];
      head = start_of[c] == i;
    }
    if (head) {
      const int32_t b = c + 1 < clusters ? start_of[c + 1] : n;
      uint64_t mask = 0;
      for (int32_t j = static_cast<int32_t>(i); j < b; ++j) mask |= 1ull << (voter[j] & 63);
      const int32_t votes = __popcll(mask);
      votes_of[c] = votes;
      keep = votes >= min_votes;
    }
    int before, total;
    mt3k::block_scan_add<kWaves>(keep, s_add, &before, &total);
    if (head) place_of[c] = keep ? kept_so_far + before : -1;
    kept_so_far += total;
    __syncthreads();
  }
  if (tid == 0) d_counts[blockIdx.x] = kept_so_far;

  // ---- 3: the emitted notes, and every note's votes
  for (int64_t i = tid; i < n; i += kTile) {
    const int32_t c = cluster_of[i];
    const int32_t a = start_of[c];
    const int32_t b = c + 1 < clusters ? start_of[c + 1] : n;
    const int32_t m = b - a, k = (m - 1) / 2;
    const int32_t votes = votes_of[c];
    const int32_t place = place_of[c];
    d_note_votes[first + i] = votes;
    if (place < 0) continue;
    const int64_t at = first + place;                  // place < the file's kept clusters <= n
    if (i == a + k) {
      d_out_onset[at] = onset[i];
      d_out_key[at] = key[i];
      d_out_votes[at] = votes;
      d_out_members[at] = m;
    }
    const double my_offset = offset[i];
    const int32_t my_velocity = velocity[i];
    int32_t rank_offset = 0, rank_velocity = 0;
    for (int32_t j = a; j < b; ++j) {
      const double o = offset[j];
      const int32_t v = velocity[j];
      rank_offset += o < my_offset || (o == my_offset && j < i);
      rank_velocity += v < my_velocity || (v == my_velocity && j < i);
    }
    if (rank_offset == k) d_out_offset[at] = my_offset;
    if (rank_velocity == k) d_out_velocity[at] = my_velocity;
  }
}

}  // namespace

extern "C" int mt3_op_note_consensus(const double* d_onset, const double* d_offset, const int32_t* d_key,
                                     const int32_t* d_velocity, const int32_t* d_voter, int64_t n_notes,
                                     const mt3_consensus_file* h_files, int32_t n_files, double tolerance,
                                     double* d_out_onset, double* d_out_offset, int32_t* d_out_key,
                                     int32_t* d_out_velocity, int32_t* d_out_votes, int32_t* d_out_members,
                                     int32_t* d_note_votes, int32_t* d_counts, int32_t* d_scratch, int64_t scratch_words,
                                     void* stream) {
  const std::string who = "mt3_op_note_consensus: ";
  if (n_notes < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_notes must not be negative");
  if (n_files < 0) return mt3::fail(MT3_ERR_INVALID, who + "n_files must not be negative");
  if (!(tolerance >= 0.0) || !std::isfinite(tolerance))
    return mt3::fail(MT3_ERR_INVALID, who + "tolerance must be finite and not negative");
  if (n_files == 0) return MT3_OK;
  if (!h_files) return mt3::fail(MT3_ERR_INVALID, who + "null file table");
  if (n_notes > 0 && (!d_onset || !d_offset || !d_key || !d_velocity || !d_voter))
    return mt3::fail(MT3_ERR_INVALID, who + "null note column (onset, offset, key, velocity or voter)");
  if (n_notes > 0 && (!d_out_onset || !d_out_offset || !d_out_key || !d_out_velocity || !d_out_votes || !d_out_members))
    return mt3::fail(MT3_ERR_INVALID, who + "null consensus column (onset, offset, key, velocity, votes or members)");
  if (n_notes > 0 && !d_note_votes) return mt3::fail(MT3_ERR_INVALID, who + "null note_votes");
  if (!d_counts) return mt3::fail(MT3_ERR_INVALID, who + "null counts");
  if (n_notes > 0 && !d_scratch) return mt3::fail(MT3_ERR_INVALID, who + "null scratch");
  if (n_notes > INT64_MAX / 4 || scratch_words < MT3_CONSENSUS_SCRATCH_WORDS(n_notes))
    return mt3::fail(MT3_ERR_INVALID, who + "scratch too small: 4 * n_notes int32 words are needed");
  int64_t end = 0;
  for (int32_t i = 0; i < n_files; ++i) {
    const mt3_consensus_file& f = h_files[i];
    if (f.first < 0 || f.n_notes < 0 || f.first > n_notes || f.n_notes > n_notes - f.first)
      return mt3::fail(MT3_ERR_INVALID, who + "a file's note range must lie inside [0, n_notes]");
    if (f.first < end) return mt3::fail(MT3_ERR_INVALID, who + "note ranges overlap or are out of order");
    end = f.first + f.n_notes;
    if (f.n_voters < 1 || f.n_voters > MT3_CONSENSUS_MAX_VOTERS)
      return mt3::fail(MT3_ERR_INVALID, who + "n_voters must be 1 .. " + std::to_string(MT3_CONSENSUS_MAX_VOTERS));
    if (f.min_votes < 1 || f.min_votes > f.n_voters)
      return mt3::fail(MT3_ERR_INVALID, who + "min_votes must be 1 .. n_voters");
  }

  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int32_t p0 = 0; p0 < n_files; p0 += kPerLaunch) {
    const int n = n_files - p0 < kPerLaunch ? n_files - p0 : kPerLaunch;
    ConsensusTable t{};
    for (int i = 0; i < n; ++i)
      t.first[i] = h_files[p0 + i].first, t.n_notes[i] = h_files[p0 + i].n_notes, t.min_votes[i] = h_files[p0 + i].min_votes;
    hipLaunchKernelGGL(consensus_kernel, dim3(static_cast<uint32_t>(n)), dim3(kTile), 0, s, t, d_onset, d_offset, d_key,
                       d_velocity, d_voter, n_notes, tolerance, d_out_onset, d_out_offset, d_out_key, d_out_velocity,
                       d_out_votes, d_out_members, d_note_votes, d_counts + p0, d_scratch);
    MT3_HIP_CHECK(hipGetLastError());
  }
  return MT3_OK;
}
