// swarm_sizes.h -- the capacity constants and LDS-size formulas that the
// host's planning (swarm_plan.h), the launch layer (swarm_engine_host.cuh) and
// the kernels' own layouts share.  Plain C++17, no HIP types: a host compiler
// reads it alone (tests/csrc/plan_selftest.cpp), the device headers include it
// and use the names in namespace swarm as before.  (The host-readable headers:
// this one, swarm_plan.h, swarm_select.h and swarm_pack.h, the packing
// contract between the cluster build and the run kernels.)
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/swarmrl_amd.h"

#ifdef __HIPCC__
#define SWARM_HD __host__ __device__
#else
#define SWARM_HD
#endif

namespace swarm {

// dynamic + static LDS of one workgroup (gfx950: 160 KB per CU)
constexpr size_t kMaxLds = 160 * 1024;
// static LDS of k_global, k_check and the run kernels: PairTables, cut2 and
// sig6 per species pair (swarm_engine.hip asserts the struct's size)
constexpr size_t kPairTablesBytes = 2 * SWARM_MAX_SPECIES * SWARM_MAX_SPECIES * sizeof(float);

constexpr int kMaxWindow = 128;   // sub-steps per cluster window
constexpr int kPairsPerWave = 256;  // neighbour pairs of one 64-lane wave (4 passes)
// Clusters wider than a wave ("big" clusters) run in k_check's workgroup, one
// member per thread: up to kBigMax members and kBigPairs pairs per env.
constexpr int kBigMax = 1024;
constexpr int kBigPairs = 4096;
constexpr int kBmWords = 256;  // sc.bmisc words per env (multi-workgroup build, k_mwb_*)
constexpr int kMaxMovers = 1024;       // listed movers per env (more: exact re-run)
// Candidate lists of the next window's pair search (latency-bound ride-along
// builds, see cand_build_body): per particle up to kCandMax partners j > i
// within r_i + r_j + skin + 2 cand_disp of the window-start positions.
constexpr int kCandMax = 24;
constexpr int kNlMax = 48;  // neighbours per colloid (more: the env re-runs)
// Device control block (uint64 words): step counter, window counter, and
// the two noise tables' first step / length (by window parity, see k_noise).
constexpr int kCtlWords = 8;
// the register-resident global path: particles per thread of a 1024-thread block
constexpr int kGlobalCH = 4;

// Wave slots per env: every cluster packs into one wave, worst case 2 N
// slots plus per-size-class rounding.  One-pass packing (latency-bound
// launches, see k_cluster_build) reserves up to 2 s lanes for a cluster of
// s particles: worst case 4 N.
SWARM_HD inline int slots_per_env(int n, bool one_pass = false) {
  return (one_pass ? 4 : 2) * n + 64 * 66;
}

// Dynamic LDS of a workgroup that runs block_env_run (swarm_env_block.cuh),
// in 4-byte words: wave sums, cell counts, a word to align what follows to 8
// bytes, the sorted positions (uint2), with dirs the sorted directors
// (float2), the sorted ids, the particle state (q, img, ang: 5 words), then
// the tail_words a path keeps of its own.
SWARM_HD inline size_t env_lds_words(int n, int ncell, bool dirs, size_t tail_words) {
  return 16 + (size_t)ncell + 1 + 1 + (dirs ? 10 : 8) * (size_t)n + tail_words;
}

// What k_langevin_run (swarm_langevin.cuh) keeps after the particle state: the
// env's velocities v_x[n], v_y[n], omega[n].
SWARM_HD inline size_t langevin_tail_words(int n) { return 3 * (size_t)n; }

// LDS words the LDS-resident global path needs after the cell counts (with
// one spare word, which the capacity thresholds below have always counted),
// 0 when it does not apply (3-D, or more than kGlobalCH particles per thread
// of a 1024-thread block).
SWARM_HD inline size_t global_lds_extra_words(int n, int dims, int ncell) {
  const size_t extra = env_lds_words(n, ncell, false, 1) - (16 + (size_t)ncell + 1);
  // k_check's layout (the larger): 16 + 16 + 1024 + ncell + 1 words first,
  // and 4 KB of static LDS beside it
  const bool fits = (16 + 16 + 1024 + (size_t)ncell + 1 + extra) * 4 + 4096 <= kMaxLds;
  return dims == 2 && n <= kGlobalCH * 1024 && fits ? extra : 0;
}

// LDS words of k_cluster_build: 168 fixed + per-wave pair counters +
// parent[N] + 3 N (cluster sizes, bases, slots) + the env's pair list.
SWARM_HD inline size_t build_lds_words(int n, int pair_cap) {
  const int wmax = slots_per_env(n, true) / 64;  // either packing
  return 16 + 16 + 3 * 68 + (size_t)((wmax + 3) & ~3) + 4 * (size_t)n + (size_t)pair_cap;
}

// LDS words of the large-N variant: the union-find forest only.
SWARM_HD inline size_t build_lds_words_big(int n) {
  const int wmax = slots_per_env(n, true) / 64;  // either packing
  return 16 + 16 + 3 * 68 + (size_t)((wmax + 3) & ~3) + (size_t)n;
}

// LDS words of the packed large-N build: two words per particle (N < 65536).
SWARM_HD inline size_t build_lds_words_packed(int n) {
  const int wmax = slots_per_env(n, true) / 64;
  return 16 + 16 + 3 * 68 + (size_t)((wmax + 3) & ~3) + 2 * (size_t)n;
}

// Words of k_build_env's sort/search region (wave sums, cell ends, sorted
// x, y, id), which must fit below the pair list of the build's LDS layout.
SWARM_HD inline size_t build_env_sort_words(int n, int ncell) {
  return 16 + (size_t)((ncell + 2) & ~1) + 3 * (size_t)n;
}

// One noise table (swarm_integrator.cuh, k_noise): three normals per
// (particle, sub-step) of a full window.
SWARM_HD inline size_t noise_table_words(size_t M) { return (size_t)kMaxWindow * 3 * M; }

// The l1_pairs pair-search role of a fused launch (swarm_observe.cuh,
// l1_pairs_role): the fallback cell search's tables.
constexpr size_t l1_role_lds_bytes() {
  return (SWARM_MAX_SPECIES * SWARM_MAX_SPECIES + 2 * 1024) * sizeof(int32_t);
}

// ---- host formulas over the cell grids' exponents (cells a side: 2^lx, 2^ly, 2^lz)

// k_global: wave sums, cell counts and (2-D, N <= 4096) the register-resident
// path's sorted copy
inline size_t global_lds_bytes(int lx, int ly, int n, int dims) {
  return (16 + (size_t)(1 << (lx + ly)) + 1 + global_lds_extra_words(n, dims, 1 << (lx + ly))) * 4;
}

// Pair-list capacity of the cluster build: up to 3 N pairs (mean degree 6),
// at least N, within the LDS left after the other arrays of k_cluster_build;
// 3 N in global memory for the large-N variant.
inline int build_pair_cap(int n, bool big) {
  if (big) return 3 * n;
  const size_t fixed = build_lds_words(n, 0) * 4;
  const size_t room = fixed < kMaxLds ? (kMaxLds - fixed) / 4 : 0;
  const size_t want = 3 * (size_t)n;
  return (int)(room < want ? room : want);
}

// The LDS build needs room for at least N pairs; beyond that, the large-N
// variant keeps only the union-find forest in LDS.
inline bool build_is_big(int n) { return build_lds_words(n, n) * 4 > kMaxLds; }

inline size_t check_lds_bytes(int lx, int ly, int n, int dims) {
  // the global-path re-run region (cell counts + LDS path) or the big
  // clusters' positions and force sums, after 16 + 16 + 1024 words
  const size_t rerun = (size_t)(1 << (lx + ly)) + 1 + global_lds_extra_words(n, dims, 1 << (lx + ly));
  const size_t big = 6 * (size_t)kBigMax + 2;  // uint2 positions, 2 x u64 sums
  return (16 + 16 + 1024 + (rerun > big ? rerun : big)) * 4;
}

// k_check3: wave sums, misc, movers, then the 3-D global path's cell counts
inline size_t check3_lds_bytes(int lx, int ly, int lz) {
  return (16 + 16 + (size_t)kMaxMovers + (size_t)(1 << (lx + ly + lz)) + 1) * 4;
}

// k_build_sort (and the fused launches carrying it) on the build grid: wave
// sums, cell counts and, staged, the sorted x | y | id rows.
inline size_t sort_lds_bytes(int lx, int ly, int lz, int sort_stage_k) {
  const size_t ncb = (size_t)1 << (lx + ly + lz);
  return (16 + ((ncb + 4) & ~(size_t)3) + 3 * (size_t)sort_stage_k) * 4;
}

}  // namespace swarm
