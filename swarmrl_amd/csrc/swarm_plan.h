// swarm_plan.h -- everything an engine fixes at creation, decided in one pure
// function: the parameter checks, both cell grids, every path choice and the
// size of every creation-time device buffer.  Plain C++17 over swarm_sizes.h
// and the C ABI's header; no HIP, no device query, no getenv, no kernel named
// (tests/csrc/plan_selftest.cpp runs it on the host against a table recorded
// before this file existed).  swarm_engine_create reads the overrides, calls
// plan_engine, allocates what the plan lists and launches by its flags.
//
// Results are bit-identical on every path, so nothing but this file's test
// and the benchmark notices a threshold that slipped: the thresholds below
// are measured ones ("Which path an engine takes").
#pragma once

#include "../../include/swarmrl_amd.h"
#include "swarm_sizes.h"

namespace swarm {

// Verlet skin of the cluster decomposition (um): pairs closer than
// r_i + r_j + skin at the window start share a cluster.  Performance only:
// results do not depend on it.  2 um keeps inter-cluster approaches below
// the cutoff over a 100-step slice a ~5-sigma event at the reference's
// defaults.
constexpr double kSkinUm = 2.0;

// SWARMRL_AMD_* overrides of a path choice: the first character of each
// variable's value, 0 for unset (swarm_engine.hip:read_plan_overrides).
struct PlanOverrides {
  char cluster_path = 0;  // SWARMRL_AMD_CLUSTER_PATH  clears
  char local_uf = 0;      // SWARMRL_AMD_LOCAL_UF      sets unless '0'
  char nlist = 0;         // SWARMRL_AMD_NLIST         clears or sets
  char noise_table = 0;   // SWARMRL_AMD_NOISE_TABLE   clears or sets
  char env_build = 0;     // SWARMRL_AMD_ENV_BUILD     clears or sets
  char wide_run = 0;      // SWARMRL_AMD_WIDE_RUN      clears
  char rot_helper = 0;    // SWARMRL_AMD_ROT_HELPER    clears
  char defer_check = 0;   // SWARMRL_AMD_DEFER_CHECK   only '1' sets
};

// The four parsing rules, v being the choice without the override.
// '0' clears; anything else leaves v as it is.
inline bool ov_clears(char c, bool v) { return c == '0' ? false : v; }
// '0' clears, '1' sets; anything else leaves v as it is.
inline bool ov_clears_or_sets(char c, bool v) { return c == '0' ? false : c == '1' ? true : v; }
// Set at all: '0' clears, anything else sets.
inline bool ov_sets_unless_0(char c, bool v) { return c ? c != '0' : v; }
// Set at all: only '1' sets.
inline bool ov_only_1_sets(char c, bool v) { return c ? c == '1' : v; }

// SWARMRL_AMD_DEFER_CHECK unset: the check of an eligible engine rides in
// the reward launch (+4 % on the headline)
constexpr bool kDeferCheckDefault = true;

// The creation-time device buffers, one row each, in allocation order:
//   X(id, bytes per element, the member that takes it, elements; 0: not allocated)
// The one list behind the plan's counts (plan_engine, where E, N, M = E N,
// D = dims, waves = E wmax and pcap = max(pair_cap, 1) are in scope) and
// swarm_engine_create's allocation table (e: the engine; vcheck: Scratch's
// vtag | verdict | varrive | cstats, one allocation).  Derived is one struct of
// the device headers: 0 bytes here, create takes its size from the member.
#define SWARM_ENGINE_BUFS(X)                                                            \
  X(Q, 4, e->st.q, 3 * M)                                                               \
  X(Img, 4, e->st.img, 3 * M)                                                           \
  X(Ang, 4, e->st.ang, M)                                                               \
  X(FSwim, 4, e->st.f_swim, M)                                                          \
  X(TorqueZ, 4, e->st.torque_z, M)                                                      \
  X(FExt, 4, e->st.f_ext, 3 * M)                                                        \
  X(Vel, 4, e->st.vel, 3 * M)                                                           \
  X(Omega, 4, e->st.omega, M)                                                           \
  X(Species, 1, e->st.species, N)                                                       \
  X(Derived, 0, e->d_derived, 1)                                                        \
  X(Box, 8, e->d_box, 3)                                                                \
  X(Order, 4, e->d_order, M)                                                            \
  X(Count1, 4, e->d_count, 1)                                                           \
  X(Step, 8, e->d_step, kCtlWords)                                                      \
  X(Arrive, 4, e->d_arrive, 1)                                                          \
  /* integrator scratch */                                                              \
  X(Sqx, 4, e->sc.sqx, M)                                                               \
  X(Sqy, 4, e->sc.sqy, M)                                                               \
  X(Sqz, 4, e->sc.sqz, M)                                                               \
  X(Simg, 4, e->sc.simg, periodic ? 1 : 3 * M)                                          \
  X(Dir3, 4, e->st.dir3, 3 * M)                                                         \
  X(TorqueXy, 4, e->st.torque_xy, 2 * M)                                                \
  X(OmegaXy, 4, e->st.omega_xy, 2 * M)                                                  \
  X(WallViol, 8, e->st.wall_viol, 1)                                                    \
  X(FPrev, 4, e->st.f_prev, 2 * M) /* two slots (window parity) */                      \
  X(TzPrev, 4, e->st.tz_prev, 2 * M)                                                    \
  X(AngPrev, 4, e->st.ang_prev, 2 * M)                                                  \
  X(Dir3Prev, 4, e->st.dir3_prev, three_d ? 6 * M : 1)                                  \
  X(TxyPrev, 4, e->st.txy_prev, three_d ? 4 * M : 1)                                    \
  X(Nmov, 4, e->sc.nmov, E)                                                             \
  X(Movers, 4, e->sc.movers, E * kMaxMovers)                                            \
  X(Sidx, 4, e->sc.sidx, M)                                                             \
  X(Bq, 4, e->sc.bq, D * M)                                                             \
  X(Bimg, 4, e->sc.bimg, D * M)                                                         \
  X(Bdir3, 4, e->sc.bdir3, three_d ? 3 * M : 1)                                         \
  X(Bang, 4, e->sc.bang, M)                                                             \
  X(Root, 4, e->sc.root, M)                                                             \
  X(SlotOf, 4, e->sc.slot_of, M)                                                        \
  X(Perm, 4, e->sc.perm, E * (size_t)pl.S)                                              \
  X(Pairs, 4, e->sc.pairs, waves * kPairsPerWave)                                       \
  X(Bsq, 4, e->sc.bsq, D * M)                                                           \
  X(Nl, 4, e->sc.nl, pl.nlist_path ? (size_t)kNlMax * M : 1)                            \
  X(Nn, 4, e->sc.nn, pl.nlist_path ? M : 1)                                             \
  X(Qalt, 4, e->sc.qalt, pl.nlist_path ? D * M : 1)                                     \
  X(Qa, 16, e->sc.qa, pl.nlist_path ? 2 * M : 1)                                        \
  X(Bsid, 4, e->sc.bsid, M)                                                             \
  X(Bcstart, 4, e->sc.bcstart, E * (((size_t)1 << lcb) + 1))                            \
  X(Gplist, 4, e->sc.gplist, E * pcap)                                                  \
  X(Xpairs, 4, e->sc.xpairs, E * pcap)                                                  \
  X(Lroot, 4, e->sc.lroot, M)                                                           \
  X(Gnx, 4, e->sc.gnx, E)                                                               \
  /* the chip-wide sort's per-cell counters and each particle's cell / rank */          \
  X(Gcnt, 4, e->sc.gcnt, pl.chip_sort ? E << (pl.lxb + pl.lyb) : 0)                     \
  X(Gcell, 4, e->sc.gcell, pl.chip_sort ? M : 0)                                        \
  X(Grank, 4, e->sc.grank, pl.chip_sort ? M : 0)                                        \
  X(Gnpairs, 4, e->sc.gnpairs, E)                                                       \
  X(Gclus, 4, e->sc.gclus, pl.big_build ? (pl.mwb ? 4 : 3) * M : 0)                     \
  X(Bmisc, 4, e->sc.bmisc, pl.mwb ? E * kBmWords : 0)                                   \
  X(WaveNpairs, 4, e->sc.wave_npairs, waves)                                            \
  X(Phase, 8, e->sc.phase, 32 + 4 * waves)                                              \
  X(Disp, 4, e->sc.disp, M)                                                             \
  X(EnvWaves, 4, e->sc.env_waves, E)                                                    \
  X(Fallback, 4, e->sc.fallback, E)                                                     \
  X(BigList, 4, e->sc.big_list, E * kBigMax)                                            \
  X(BigPairs, 4, e->sc.big_pairs, E * kBigPairs)                                        \
  X(BigN, 4, e->sc.big_n, E)                                                            \
  X(BigNp, 4, e->sc.big_np, E)                                                          \
  X(VsRec, 16, e->vs.rec, 2 * M)                                                        \
  X(VsAgentRow, 4, e->vs.agent_row, N)                                                  \
  X(Noise, 4, e->d_noise, pl.noise_table ? 2 * noise_table_words(M) : 0) /* two tables */ \
  X(Cand, 4, e->sc.cand, pl.l1_pairs ? (size_t)kCandMax * M : 0)                        \
  X(Ncand, 4, e->sc.ncand, pl.l1_pairs ? M : 0)                                         \
  X(CandOk, 4, e->sc.cand_ok, E)                                                        \
  X(CandOvf, 4, e->sc.cand_ovf, E)                                                      \
  X(SortDone, 8, e->sc.sort_done, E)                                                    \
  X(Stats, 8, e->sc.stats, 4)                                                           \
  /* a check that rides in the reward launch: [E] x 3 and four outcome counters */      \
  X(Vcheck, 8, vcheck, pl.l1_pairs ? 3 * E + 4 : 0)

#define SWARM_BUF_ID(id, bytes, member, elements) kBuf##id,
enum EngineBuf : int { SWARM_ENGINE_BUFS(SWARM_BUF_ID) kNumEngineBufs };
#undef SWARM_BUF_ID
#define SWARM_BUF_BYTES(id, bytes, member, elements) bytes,
constexpr unsigned char kBufElemBytes[kNumEngineBufs] = {SWARM_ENGINE_BUFS(SWARM_BUF_BYTES)};
#undef SWARM_BUF_BYTES

struct EnginePlan {
  int lxg = 0, lyg = 0, lzg = 0;  // global-path grid: cell side >= rc_max (lzg: 3-D)
  int lxb = 0, lyb = 0, lzb = 0;  // cluster-build grid: cell side >= rc_max + skin
  bool latency_bound = false;  // E * N <= 32768: few envs x particles fill few SIMDs
  bool cluster_path = false;   // windows of cluster build -> run -> check (else k_global)
  // boxes whose rc + skin graph percolates: chip-wide sub-steps over a
  // per-window Verlet list instead of per-wave clusters
  bool nlist_path = false;
  bool big_build = false;  // k_cluster_build<true>: cluster arrays in global memory
  bool chip_sort = false;  // 2-D envs above 4096 colloids: the three-launch chip-wide sort
  bool local_uf = false;   // block-local union-find in the 2-D pair search
  bool mwb = false;        // the large-N 2-D build spread over the chip (k_mwb_*)
  bool one_pass = true;    // one pair pass per wave and sub-step
  bool fill_singletons = false;  // singletons take the tail lanes of the other classes
  bool noise_table = false;  // latency-bound windows read their normals from a table (k_noise)
  bool env_build = false;    // k_build_env: the whole build in one workgroup per env
  // k_cluster_run_wide: one block of run_wpb run waves per CU and
  // (noise_blocks > 0) the next window's noise table filled beside the run
  bool wide_run = false;
  bool rot_helper = true;  // a rotation helper wave beside each run wave (run_wpb <= 2)
  bool l1_pairs = false;   // the pair search as a filter of candidate lists (Scratch::l1_pairs)
  bool defer_check = false;  // an l1_pairs engine's check may ride in the reward launch
  int pair_cap = 0, S = 0, wmax = 0, sort_stage_k = 0;
  int noise_blocks = 0, run_wpb = 4;
  double cand_disp = 0.0;  // l1_pairs: widening of the candidate radius (um)
  // elements per creation-time buffer; 0: not allocated
  size_t count[kNumEngineBufs] = {};
};

// An engine whose every sub-step runs on one workgroup per env (a rod,
// ellipsoids, the Langevin thermostat): no cluster windows, and none of what
// prepares or checks them.
// The one rewrite of a plan after creation.
inline void plan_no_cluster_windows(EnginePlan& pl) {
  pl.cluster_path = false;
  pl.nlist_path = false;
  pl.noise_table = false;
  pl.wide_run = false;
  pl.env_build = false;
  pl.defer_check = false;
}

inline int ilog2_floor(double v) {
  int l = 0;
  while ((double)(1 << (l + 1)) <= v && l < 20) ++l;
  return l;
}

// Power-of-two cell grid with side >= cutoff and at most max(n, 64) cells
// (identical rule in oracle/swarm_oracle.c:or_cell_grid).
inline void cell_grid(const swarm_params_t& p, int n, double cutoff, int* lx, int* ly) {
  int l[2];
  for (int a = 0; a < 2; ++a) {
    const double m = cutoff > 0.0 ? p.box[a] / cutoff : 1024.0;
    l[a] = m >= 1.0 ? ilog2_floor(m) : 0;
    if (l[a] > 15) l[a] = 15;
  }
  const int cap = n > 64 ? n : 64;
  while ((1 << (l[0] + l[1])) > cap) {
    if (l[0] >= l[1] && l[0] > 0)
      l[0]--;
    else if (l[1] > 0)
      l[1]--;
    else
      break;
  }
  *lx = l[0];
  *ly = l[1];
}

// 3-D: the same rule over three axes (3-D global path).
inline void cell_grid3(const swarm_params_t& p, int n, double cutoff, int* lx, int* ly, int* lz) {
  int l[3];
  for (int a = 0; a < 3; ++a) {
    const double m = cutoff > 0.0 ? p.box[a] / cutoff : 1024.0;
    l[a] = m >= 1.0 ? ilog2_floor(m) : 0;
    if (l[a] > 10) l[a] = 10;
  }
  const int n64 = n > 64 ? n : 64;
  const int cap = n64 < 8192 ? n64 : 8192;  // counts fit the default 64 KB of LDS
  while ((1 << (l[0] + l[1] + l[2])) > cap) {
    int k = 0;
    for (int a = 1; a < 3; ++a)
      if (l[a] > l[k]) k = a;
    if (l[k] == 0) break;
    l[k]--;
  }
  *lx = l[0];
  *ly = l[1];
  *lz = l[2];
}

// The widest cutoff, radius[s] + radius[t]: the cell side of the global-path
// grid (Derived::rc_max is this value).
inline double max_cutoff(const swarm_params_t& p) {
  double rc_max = 0.0;
  for (int s = 0; s < p.n_species; ++s)
    for (int t = 0; t < p.n_species; ++t)
      rc_max = p.radius[s] + p.radius[t] > rc_max ? p.radius[s] + p.radius[t] : rc_max;
  return rc_max;
}

// static_lds: the static LDS of the kernels beside their dynamic LDS (the
// pair tables of k_global, k_check and the run kernels).
inline int plan_engine(const swarm_params_t& p, int n_envs, int n, const PlanOverrides& ov,
                       size_t static_lds, EnginePlan* out, const char** msg) {
  // the checks of swarm_engine_create on its parameters and sizes, in the
  // order the C ABI has always made them
  auto bad = [&](int code, const char* m) { return *msg = m, code; };
  if (p.n_dims != 2 && p.n_dims != 3) return bad(SWARM_EINVAL, "n_dims must be 2 or 3");
  if (n_envs < 1 || n < 1) return bad(SWARM_EINVAL, "n_envs and n_particles must be >= 1");
  if (p.n_species < 1 || p.n_species > SWARM_MAX_SPECIES)
    return bad(SWARM_EINVAL, "n_species out of range");
  for (int a = 0; a < p.n_dims; ++a)
    if (!(p.box[a] > 0.0)) return bad(SWARM_EINVAL, "box lengths must be positive");
  // the run kernels' 1/r^2 (rcp_rn) is exact for r^2 in [2^-96, 2^96]: a
  // fixed-point grid step of at least 2^-48 and radii below 2^40
  for (int a = 0; a < p.n_dims; ++a)
    if (!(p.box[a] >= 0x1p-16)) return bad(SWARM_EINVAL, "box lengths must be >= 2^-16");
  if (!(p.time_step > 0.0)) return bad(SWARM_EINVAL, "time_step must be positive");
  for (int s = 0; s < p.n_species; ++s) {
    if (!(p.gamma_t[s] > 0.0) || !(p.gamma_r[s] > 0.0) || !(p.radius[s] >= 0.0))
      return bad(SWARM_EINVAL, "friction coefficients must be positive");
    if (!(p.radius[s] < 0x1p40)) return bad(SWARM_EINVAL, "radius must be < 2^40");
  }
  if (n > (1 << 20))
    return bad(SWARM_ECAPACITY, "more than 2^20 particles per env are not supported");

  EnginePlan pl;
  const bool three_d = p.n_dims == 3;
  const bool periodic = p.periodic != 0;
  double rmax = 0.0;
  for (int s = 0; s < p.n_species; ++s) rmax = p.radius[s] > rmax ? p.radius[s] : rmax;
  const double rc_max = max_cutoff(p);
  if (three_d) {
    cell_grid3(p, n, rc_max, &pl.lxg, &pl.lyg, &pl.lzg);
    cell_grid3(p, n, rc_max + kSkinUm, &pl.lxb, &pl.lyb, &pl.lzb);
  } else {
    cell_grid(p, n, rc_max, &pl.lxg, &pl.lyg);
    cell_grid(p, n, rc_max + kSkinUm, &pl.lxb, &pl.lyb);
  }
  const int lcb = pl.lxb + pl.lyb + pl.lzb;  // build cells 2^lcb
  if (check_lds_bytes(pl.lxg, pl.lyg, n, p.n_dims) + static_lds > kMaxLds)
    return bad(SWARM_ECAPACITY, "env cell grid does not fit the LDS of one workgroup");
  // the cluster path needs the build workgroup's LDS and a non-degenerate
  // build grid; otherwise every window runs on the global path
  pl.big_build = build_is_big(n);
  pl.pair_cap = build_pair_cap(n, pl.big_build);
  // block-local union-find in the 2-D pair search (default: for envs above
  // 4096 colloids, whose one-workgroup union phase is long; at 4096 the pair
  // search's block barriers cost more than the union saves, measured)
  pl.local_uf = ov_sets_unless_0(ov.local_uf, n > 4096);
  // the 2-D build sort stages its scatter in LDS: the sorted rows of up to
  // K entries per pass beside the cell counts (K a multiple of 4, at least
  // N / 4)
  {
    const size_t counts = (16 + ((size_t)1 << (pl.lxb + pl.lyb)) + 1) * 4;
    const size_t room = counts + 4096 < kMaxLds ? kMaxLds - counts - 4096 : 0;
    const size_t k = ((size_t)n < room / 12 ? (size_t)n : room / 12) & ~(size_t)3;
    pl.sort_stage_k = !three_d && n <= 16 * 1024 && 4 * k >= (size_t)n ? (int)k : 0;
  }
  // non-periodic boxes run windowed in 2-D and 3-D (edge cells and
  // unwrapped distances in the build and the exact check; a listed pair's
  // folded difference is its unwrapped one); SWARMRL_AMD_CLUSTER_PATH=0
  // forces the global path (A/B and parity)
  // (n < 65536, the packed build's 16-bit ids, never decides: the forest's
  // LDS already ends the cluster path at N = 38264)
  pl.cluster_path = pl.pair_cap >= n && n < 65536 && build_lds_words_big(n) * 4 <= kMaxLds &&
                    (size_t)(16 + (1 << lcb) + 1) * 4 <= kMaxLds && (1 << pl.lxb) >= 3 &&
                    (1 << pl.lyb) >= 3 && (!three_d || (1 << pl.lzb) >= 3) &&
                    (!three_d || check3_lds_bytes(pl.lxg, pl.lyg, pl.lzg) <= kMaxLds);
  pl.cluster_path = ov_clears(ov.cluster_path, pl.cluster_path);
  if (pl.cluster_path) {
    // mean number of colloids within 2 r_max + skin of one (deg): above ~2
    // in 3-D, ~3 in 2-D the links percolate into clusters wider than a wave
    // (3-D: re-run on the global path; 2-D: k_check's one-workgroup big
    // cluster run, then the global path), so the window runs on the
    // neighbour-list path instead.  SWARMRL_AMD_NLIST=0|1 overrides.
    constexpr double kTwoPi = 6.283185307179586476925;
    const double link = 2.0 * rmax + kSkinUm;
    const double deg =
        three_d ? (double)n / (p.box[0] * p.box[1] * p.box[2]) * (2.0 / 3.0) * kTwoPi * link *
                      link * link
                : (double)n / (p.box[0] * p.box[1]) * 0.5 * kTwoPi * link * link;
    pl.nlist_path = ov_clears_or_sets(ov.nlist, deg > (three_d ? 2.0 : 3.0));
    if (!periodic) pl.nlist_path = false;  // the Verlet-list window is periodic-only
  }
  // One pair pass per wave and sub-step (k_cluster_build): the run kernel
  // lasts as long as its slowest waves, at any env count.  Latency-bound
  // launches (few envs x particles fill few SIMDs) also read their normals
  // from a table (k_noise; SWARMRL_AMD_NOISE_TABLE=0|1 overrides).
  const size_t E = (size_t)n_envs, N = (size_t)n, M = E * N;
  pl.latency_bound = (long)n_envs * n <= 32768;
  pl.one_pass = true;
  // fewer, fuller waves only pay when the waves compete for the SIMDs; a
  // latency-bound launch has SIMDs to spare and a shorter build is worth more
  pl.fill_singletons = !pl.latency_bound;
  pl.S = slots_per_env(n, pl.one_pass);
  pl.wmax = pl.S / 64;
  // chip-wide build sort of large 2-D envs (k_sort_count/scan/scatter)
  pl.chip_sort = !three_d && n > 4096;
  // 2-D envs of the large-N build after the block-local pair search: the
  // build spread over the chip (k_mwb_*) instead of one workgroup, with a
  // fourth per-particle word (the offset of its pairs in the pair list)
  pl.mwb = pl.big_build && !three_d && pl.local_uf;
  // noise table for latency-bound windows: few envs fill few SIMDs, so the
  // normals are better produced chip-wide ahead of the run; 3-D and
  // neighbour-list windows draw their normals in the kernels
  pl.noise_table = ov_clears_or_sets(ov.noise_table, pl.latency_bound) && p.kT > 0.0 &&
                   pl.cluster_path && !three_d && !pl.nlist_path;
  // the one-launch build (one CU per env) for throughput-bound engines
  // when its sort region fits below the pair list; latency-bound ones keep
  // the three-launch build, whose pair search spreads over the chip
  // (one env: 42 us for the three launches, 52 us for k_build_env)
  {
    const size_t below = 16 + 16 + 3 * 68 + (size_t)((pl.wmax + 3) & ~3) + 4 * N;
    const bool can = pl.cluster_path && !pl.big_build && !three_d && !pl.nlist_path && periodic &&
                     build_env_sort_words(n, 1 << (pl.lxb + pl.lyb)) <= below;
    pl.env_build = can && ov_clears_or_sets(ov.env_build, !pl.latency_bound);
  }
  // one block per CU for latency-bound runs; beside a run of up to 16384
  // particles, 64 CUs produce the next window's table in its shadow (C5:
  // no k_noise launch between the policy and the run)
  pl.wide_run = ov_clears(ov.wide_run, pl.noise_table);
  // (32 noise workgroups above 4096 colloids, so that C4's 8 x 1024 gets one
  // run wave per CU, measured slower: C4 81.1 -> 72.9 M, same box)
  pl.noise_blocks = pl.wide_run && M <= 16384 ? 64 : 0;
  pl.rot_helper = ov_clears(ov.rot_helper, true);
  // run waves per CU: a wave alone on its CU does not share the CU's
  // texture path with other waves' scattered noise-table gathers; four per
  // CU once the run's waves (~1 per 46 particles) would not fit one per CU
  {
    const long est = (long)M / 46 + 1;
    pl.run_wpb = est + pl.noise_blocks <= 224 ? 1 : (est / 2 + pl.noise_blocks <= 256 ? 2 : 4);
  }
  // l1_pairs: the ride-along build's pair search moves into the slice's
  // first launch as a filter of candidate lists prepared during the last
  // run (periodic 2-D, the plain pair search, a build grid of at least 5
  // cells a side for the 5 x 5 candidate stencil)
  pl.l1_pairs = pl.wide_run && pl.cluster_path && !pl.nlist_path && !pl.env_build &&
                !pl.big_build && !three_d && periodic && !pl.local_uf && (1 << pl.lxb) >= 5 &&
                (1 << pl.lyb) >= 5;
  if (pl.l1_pairs) {
    // widening of the candidate radius: up to 1.5 um of motion per window
    // (the bench's swimmers move ~0.3 um; > 1.5 um is a > 6 sigma event),
    // at most half a cell side (the 5 x 5 stencil) and at least skin / 2
    // (k_check sees every particle that moved more: the movers)
    const double sx = p.box[0] / (1 << pl.lxb), sy = p.box[1] / (1 << pl.lyb);
    const double half = 0.5 * (sx < sy ? sx : sy);
    const double cap = 1.5 < half ? 1.5 : half;
    pl.cand_disp = 0.5 * kSkinUm > cap ? 0.5 * kSkinUm : cap;
    pl.defer_check = ov_only_1_sets(ov.defer_check, kDeferCheckDefault);
  }

  const size_t D = three_d ? 3 : 2, waves = E * (size_t)pl.wmax;
  const size_t pcap = (size_t)(pl.pair_cap > 1 ? pl.pair_cap : 1);
#define SWARM_BUF_COUNT(id, bytes, member, elements) pl.count[kBuf##id] = (elements);
  SWARM_ENGINE_BUFS(SWARM_BUF_COUNT)
#undef SWARM_BUF_COUNT
  *out = pl;
  return SWARM_OK;
}

}  // namespace swarm
