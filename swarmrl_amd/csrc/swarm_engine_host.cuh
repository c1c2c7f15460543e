// swarm_engine_host.cuh -- the host launch layer of the engine and its
// observables: every integrator, build, check, cone and reward launch
// ("Host launch layer").
//
// Part of swarm_engine.hip's translation unit, included after struct
// swarm_engine: everything here takes the engine and uses fail, HIP_TRY,
// dev_malloc / dev_free and cell_grid; what creation fixed it reads from
// e->plan (swarm_plan.h).  swarm_engine.hip keeps the C ABI (argument checks,
// engine state, uploads and downloads); what it launches beyond single fixed
// kernels it launches through here.
//
// Every decision that picks a kernel or sizes a launch is taken in one place:
//   *_lds_bytes       the dynamic LDS of each kernel family
//   allow_engine_lds  dynamic LDS above 64 KB, once per device
//   launch_sort / launch_pairs / launch_cluster_build   the build's stages
//   launch_check / launch_check3                        the window's check
//   launch_nlist_steps   the neighbour-list sub-steps, 2-D and 3-D
//   xcd_grid          the XCD-aware grid of the run and the cone
// and template flags reach a kernel through swarm_select.h only: one generic
// lambda per launch site that names each flag once.
#pragma once

#include <algorithm>
#include <mutex>
#include <vector>

#include "swarm_select.h"

namespace {

using swarm_select::bools;
using swarm_select::kVisionGWide;

// ---- dynamic LDS

// the formulas the plan shares with the kernels' layouts: swarm_sizes.h
using swarm::kMaxLds;
using swarm::check_lds_bytes;
using swarm::global_lds_bytes;

size_t build_lds_bytes(int n, int pair_cap) { return swarm::build_lds_words(n, pair_cap) * 4; }

size_t check3_lds_bytes(const swarm_engine* e) {
  const swarm::EnginePlan& pl = e->plan;
  return swarm::check3_lds_bytes(pl.lxg, pl.lyg, pl.lzg);
}

size_t sort_lds_bytes(const swarm_engine* e) {
  const swarm::EnginePlan& pl = e->plan;
  return swarm::sort_lds_bytes(pl.lxb, pl.lyb, pl.lzb, e->sc.sort_stage_k);
}

// LDS of the vision grid's workgroup: wave sums, cell counts and, staged,
// the env's 2 x uint4 records (host and device agree through va.staged).
size_t vision_grid_lds_bytes(int lx, int ly, int n, bool staged) {
  const size_t counts = (16 + ((size_t)1 << (lx + ly)) + 1) * 4;
  return staged ? ((counts + 15) & ~(size_t)15) + 32 * (size_t)n : counts;
}

// LDS of a launch carrying the l1_pairs pair search (its fallback tables)
// beside workgroups that need `other` bytes.
size_t l1_launch_lds(const swarm_engine* e, size_t other) {
  return e->sc.l1_pairs ? std::max(other, swarm::l1_role_lds_bytes()) : other;
}

// ROCm admits dynamic LDS up to the device limit at launch; this attribute
// is only a hint, a refusal is not an error (a launch that really exceeds the
// limit fails at hipGetLastError after the launch).  Given at engine creation,
// once per device, and not at the launch sites: a first launch can fall inside
// a stream capture.  Kernels with template flags are walked over every
// variant the launch layer can select.
// Nothing depends on the order of this walk.  A side effect worth knowing
// when a figure moves: a template kernel is emitted into the code object where
// the translation unit first names it, which for these kernels is here (and
// for the others the order in which a launch site's `bools` visits them).
// With the orders as written 215 of the 244 kernels have the address they had
// before the launch layer existed (profiles/r10_engine_host_repeats.txt has
// the figures of this build and of one with other orders).
void allow_engine_lds(int device) {
  static std::mutex mu;
  static std::vector<int> done;
  const std::lock_guard<std::mutex> lock(mu);
  if (std::find(done.begin(), done.end(), device) != done.end()) return;
  auto allow = [](auto* fn) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
  };
  allow(&swarm::k_global);
  allow(&swarm::k_rod_run);
  // (no k_cluster_build<true, true>: the large-N build after the block-local
  // pair search is k_mwb_*)
  allow(&swarm::k_cluster_build<false, false>);
  allow(&swarm::k_cluster_build<false, true>);
  allow(&swarm::k_cluster_build<true, false>);
  allow(&swarm::k_cluster_build_packed);
  swarm_select::each_sort_chunk([&](auto ch) { allow(&swarm::k_build_sort<ch>); });
  allow(&swarm::k_sort_scan);
  allow(&swarm::k_build_env);
  allow(&swarm::k_check);
  allow(&k_grid_build);
  allow(&k_vision_grid);
  swarm_select::each_bools<3>([&](auto multi, auto walls, auto pot) {
    allow(&swarm::k_cluster_run_wide<multi, walls, pot>);
  });
  swarm_select::each_sort_chunk([&](auto ch) { allow(&k_vgrid_sort<ch>); });
  swarm_select::each_bools<1>([&](auto check) {
    swarm_select::each_sort_chunk([&](auto ch) { allow(&k_field_vgrid_sort<ch, check>); });
  });
  allow(&k_policy_cbuild<4, 4, 4>);
  // (last: every kernel above keeps its place in the code object)
  swarm_select::each_bools<1>([&](auto gb) { allow(&swarm::k_ellipsoid_run<gb>); });
  allow(&swarm::k_langevin_run);
  allow(&swarm::k_global_envs);
  allow(&swarm::k_global_marked);
  (void)hipGetLastError();
  done.push_back(device);
}

// ---- the global path, the rod, the ellipsoids, the Langevin thermostat, the noise table

int launch_global(swarm_engine* e, int n_steps, int sd_mode, float g, float md) {
  const swarm::EnginePlan& pl = e->plan;
  if (e->params.n_dims == 3) {
    hipLaunchKernelGGL(swarm::k_global3, dim3(e->n_envs), dim3(1024),
                       (16 + (size_t)(1 << (pl.lxg + pl.lyg + pl.lzg)) + 1) * 4, e->stream,
                       e->d_derived, e->st, e->sc, n_steps, e->d_step, e->d_arrive, pl.lxg,
                       pl.lyg, pl.lzg, sd_mode, g, md);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  }
  if (e->has_rod) {
    hipLaunchKernelGGL(swarm::k_rod_run, dim3(e->n_envs), dim3(1024),
                       swarm::env_lds_words(e->n, 1 << (pl.lxg + pl.lyg), false,
                                            swarm::kRodTailWords) * 4, e->stream,
                       e->d_derived, e->st, e->rod, n_steps, e->d_step, e->d_arrive, pl.lxg, pl.lyg,
                       sd_mode, g, md);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  }
  if (e->has_ell) {
    bools([&](auto gb) {
      hipLaunchKernelGGL(swarm::k_ellipsoid_run<gb>, dim3(e->n_envs), dim3(1024),
                         swarm::env_lds_words(e->n, 1 << (pl.lxg + pl.lyg), true, 0) * 4, e->stream,
                         e->d_derived, e->st, e->d_ell, n_steps, e->d_step, e->d_arrive, pl.lxg,
                         pl.lyg, sd_mode, g, md);
    }, e->ell_gb);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  }
  if (e->has_lv) {
    hipLaunchKernelGGL(swarm::k_langevin_run, dim3(e->n_envs), dim3(1024),
                       swarm::env_lds_words(e->n, 1 << (pl.lxg + pl.lyg), false,
                                            swarm::langevin_tail_words(e->n)) * 4, e->stream,
                       e->d_derived, e->st, e->d_lv, n_steps, e->d_step, e->d_arrive, pl.lxg,
                       pl.lyg, sd_mode, g, md);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  }
  hipLaunchKernelGGL(swarm::k_global, dim3(e->n_envs), dim3(1024),
                     global_lds_bytes(pl.lxg, pl.lyg, e->n, e->params.n_dims), e->stream, e->d_derived, e->st, e->sc,
                     n_steps, e->d_step, e->d_arrive, pl.lxg, pl.lyg, sd_mode, g, md);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// swarm_engine_reset_envs (swarm_reset.cuh): the placement of the n_listed
// envs in e->d_reset_envs, and n_steps of their overlap removal (launch_global
// in steepest-descent mode over the list; plain colloids only).
int launch_place(swarm_engine* e, int n_listed) {
  const long items = (long)n_listed * e->n;
  const swarm::ResetArgs a{e->d_reset_envs, n_listed,      e->d_group_of,  e->d_groups,
                           e->d_home_q,     e->d_home_img, e->d_home_ang,  e->d_home_dir3,
                           e->reset_ordinal, e->sc.cand_ok};
  hipLaunchKernelGGL(swarm::k_place_envs, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                     e->stream, e->d_derived, e->st, a);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int launch_global_envs(swarm_engine* e, int n_listed, int n_steps, float g, float md) {
  const swarm::EnginePlan& pl = e->plan;
  if (e->params.n_dims == 3)
    hipLaunchKernelGGL(swarm::k_global3_envs, dim3(n_listed), dim3(1024),
                       (16 + (size_t)(1 << (pl.lxg + pl.lyg + pl.lzg)) + 1) * 4, e->stream,
                       e->d_derived, e->st, e->sc, e->d_reset_envs, n_steps, e->d_step, pl.lxg,
                       pl.lyg, pl.lzg, g, md);
  else
    hipLaunchKernelGGL(swarm::k_global_envs, dim3(n_listed), dim3(1024),
                       global_lds_bytes(pl.lxg, pl.lyg, e->n, e->params.n_dims), e->stream,
                       e->d_derived, e->st, e->sc, e->d_reset_envs, n_steps, e->d_step, pl.lxg,
                       pl.lyg, g, md);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// swarm_engine_reset_marked: the same over every env, the marked ones acting;
// the grids do not depend on the mask.  The per-env reset counts are bumped
// in a launch of their own after the placement has read them.
int launch_place_marked(swarm_engine* e, const uint8_t* d_mask) {
  const long items = (long)e->n_envs * e->n;
  const swarm::ResetArgs a{nullptr,     e->n_envs,     e->d_group_of, e->d_groups,
                           e->d_home_q, e->d_home_img, e->d_home_ang, e->d_home_dir3,
                           0,           e->sc.cand_ok};
  hipLaunchKernelGGL(swarm::k_place_marked, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                     e->stream, e->d_derived, e->st, a, d_mask, e->d_reset_counts);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(swarm::k_count_marked, dim3((unsigned)((e->n_envs + 255) / 256)), dim3(256),
                     0, e->stream, d_mask, e->d_reset_counts, e->n_envs);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int launch_global_marked(swarm_engine* e, const uint8_t* d_mask, int n_steps, float g, float md) {
  const swarm::EnginePlan& pl = e->plan;
  if (e->params.n_dims == 3)
    hipLaunchKernelGGL(swarm::k_global3_marked, dim3(e->n_envs), dim3(1024),
                       (16 + (size_t)(1 << (pl.lxg + pl.lyg + pl.lzg)) + 1) * 4, e->stream,
                       e->d_derived, e->st, e->sc, d_mask, n_steps, e->d_step, pl.lxg, pl.lyg,
                       pl.lzg, g, md);
  else
    hipLaunchKernelGGL(swarm::k_global_marked, dim3(e->n_envs), dim3(1024),
                       global_lds_bytes(pl.lxg, pl.lyg, e->n, e->params.n_dims), e->stream,
                       e->d_derived, e->st, e->sc, d_mask, n_steps, e->d_step, pl.lxg, pl.lyg, g,
                       md);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// The rod's beads onto the centre's line (swarm_rod.cuh:rod_place).
int launch_rod_snap(swarm_engine* e) {
  const int items = e->n_envs * (e->rod.n - 1);
  if (items <= 0) return SWARM_OK;
  hipLaunchKernelGGL(swarm::k_rod_snap, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                     e->stream, e->d_derived, e->st, e->rod, e->n_envs);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// Noise table (latency-bound windows) for n sub-steps from the current
// step counter.
int launch_noise(swarm_engine* e, hipStream_t stream, int n) {
  const long M = (long)e->n_envs * e->n;
  const long items = M * (long)swarm::noise_items(n);
  hipLaunchKernelGGL(swarm::k_noise, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream,
                     e->d_derived, e->st, e->d_step, e->d_noise, n);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// ---- the stages of the cluster build: sort, pair search, cluster build

// One block of 256 threads per 256 colloids, per env (the pair searches, the
// chip-wide sort, the k_mwb_* stages).
dim3 per_colloid_grid(const swarm_engine* e) {
  return dim3((unsigned)((e->n + 255) / 256), (unsigned)e->n_envs);
}

// Stage 1, the cell sort of every env.  chip: the three-launch chip-wide sort
// of 2-D envs above 4096 colloids (launch_build; the deferred build's sort is
// always the one-workgroup k_build_sort, the stage the fused launches carry).
int launch_sort(swarm_engine* e, hipStream_t stream, bool chip) {
  const swarm::EnginePlan& pl = e->plan;
  if (e->params.n_dims == 3) {
    swarm_select::sort_chunk(e->n, [&](auto ch) {
      hipLaunchKernelGGL(swarm::k_build_sort3<ch>, dim3(e->n_envs), dim3(1024), sort_lds_bytes(e),
                         stream, e->st, e->sc, pl.lxb, pl.lyb, pl.lzb);
    });
  } else if (chip) {
    hipLaunchKernelGGL(swarm::k_sort_count, per_colloid_grid(e), dim3(256), 0, stream, e->st,
                       e->sc, pl.lxb, pl.lyb);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(swarm::k_sort_scan, dim3(e->n_envs), dim3(1024),
                       (size_t)(16 + (1 << (pl.lxb + pl.lyb)) + 1) * 4, stream, e->sc, pl.lxb,
                       pl.lyb);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(swarm::k_sort_scatter, per_colloid_grid(e), dim3(256), 0, stream, e->st,
                       e->sc, pl.lxb, pl.lyb);
  } else {
    swarm_select::sort_chunk(e->n, [&](auto ch) {
      hipLaunchKernelGGL(swarm::k_build_sort<ch>, dim3(e->n_envs), dim3(1024), sort_lds_bytes(e),
                         stream, e->st, e->sc, pl.lxb, pl.lyb);
    });
  }
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// Stage 2, the pair search over the sorted cells (cluster path).
int launch_pairs(swarm_engine* e, hipStream_t stream) {
  const swarm::EnginePlan& pl = e->plan;
  if (e->params.n_dims == 3) {
    hipLaunchKernelGGL(swarm::k_build_pairs3, per_colloid_grid(e), dim3(256), 0, stream,
                       e->d_derived, e->st, e->sc, pl.lxb, pl.lyb, pl.lzb);
  } else {
    bools([&](auto local) {
      hipLaunchKernelGGL(swarm::k_build_pairs<local>, per_colloid_grid(e), dim3(256), 0, stream,
                         e->d_derived, e->st, e->sc, pl.lxb, pl.lyb);
    }, e->sc.local_uf != 0);
  }
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// Stage 2 of the neighbour-list path: Verlet lists, no clusters.
int launch_nlist_build(swarm_engine* e, hipStream_t stream) {
  const swarm::EnginePlan& pl = e->plan;
  if (e->params.n_dims == 3)
    hipLaunchKernelGGL(swarm::k_build_nlist3, per_colloid_grid(e), dim3(256), 0, stream,
                       e->d_derived, e->st, e->sc, pl.lxb, pl.lyb, pl.lzb);
  else
    hipLaunchKernelGGL(swarm::k_build_nlist2, per_colloid_grid(e), dim3(256), 0, stream,
                       e->d_derived, e->st, e->sc, pl.lxb, pl.lyb);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// Stage 3, clusters from the pair list.
int launch_cluster_build(swarm_engine* e, hipStream_t stream) {
  const swarm::EnginePlan& pl = e->plan;
  // 2-D: the pair search left block-local union-find roots and a cross list
  // (build_pairs_body); 3-D (k_build_pairs3): the whole pair list is unioned
  const bool local = e->params.n_dims == 2 && e->sc.local_uf;
  if (e->sc.bmisc) {  // multi-workgroup build: union, sizes, classes, slots, wave pair lists
    const unsigned nbp = (unsigned)((e->n + 255) / 256);
    hipLaunchKernelGGL(swarm::k_mwb_union, dim3((nbp + 3) / 4, e->n_envs), dim3(256), 0, stream,
                       e->st, e->sc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(swarm::k_mwb_size, dim3(nbp, e->n_envs), dim3(256), 0, stream, e->st, e->sc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(swarm::k_mwb_class, dim3((unsigned)((e->n + 1023) / 1024), e->n_envs),
                       dim3(1024), 0, stream, e->st, e->sc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(swarm::k_mwb_slots, dim3(nbp, e->n_envs), dim3(256), 0, stream, e->st,
                       e->sc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(swarm::k_mwb_pairs, dim3((unsigned)((e->sc.wmax + 3) / 4), e->n_envs),
                       dim3(256), 0, stream, e->st, e->sc);
  } else if (pl.big_build && !local && swarm::build_lds_words_packed(e->n) * 4 <= kMaxLds) {
    hipLaunchKernelGGL(swarm::k_cluster_build_packed, dim3(e->n_envs), dim3(1024),
                       swarm::build_lds_words_packed(e->n) * 4, stream, e->st, e->sc);
  } else if (pl.big_build) {  // (2-D envs with the local pair search took k_mwb_*)
    hipLaunchKernelGGL((swarm::k_cluster_build<true, false>), dim3(e->n_envs), dim3(1024),
                       swarm::build_lds_words_big(e->n) * 4, stream, e->st, e->sc);
  } else {
    bools([&](auto loc) {
      hipLaunchKernelGGL((swarm::k_cluster_build<false, loc>), dim3(e->n_envs), dim3(1024),
                         build_lds_bytes(e->n, e->sc.pair_cap), stream, e->st, e->sc);
    }, local);
  }
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// Cluster build of the next window.
int launch_build(swarm_engine* e, hipStream_t stream) {
  const swarm::EnginePlan& pl = e->plan;
  if (pl.env_build) {
    hipLaunchKernelGGL(swarm::k_build_env, dim3(e->n_envs), dim3(1024),
                       build_lds_bytes(e->n, e->sc.pair_cap), stream, e->d_derived, e->st, e->sc,
                       pl.lxb, pl.lyb);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  }
  if (const int rc = launch_sort(e, stream, pl.chip_sort)) return rc;
  if (pl.nlist_path) return launch_nlist_build(e, stream);
  if (const int rc = launch_pairs(e, stream)) return rc;
  return launch_cluster_build(e, stream);
}

// Launch the deferred build's pending stages on the engine stream (no
// consumer carried them along); the window then uses the build.
// swarm_engine_defer_build grants the deferred build to 2-D cluster-path
// engines without env_build, big_build and the neighbour-list path only, for
// which launch_build's pair search and cluster build are the two launched
// here (no k_mwb_*, packed or large-N arm: they need big_build).  The sort
// differs: above 4096 colloids launch_build takes the chip-wide sort, the
// deferred build k_build_sort<16>, as its fused carriers do.
int flush_ride_along(swarm_engine* e) {
  const int stage = e->ride_stage;
  e->vgrid_ready = false;
  if (stage == 0) return SWARM_OK;
  e->ride_stage = 0;
  if (stage <= 1)
    if (const int rc = launch_sort(e, e->stream, false)) return rc;
  if (stage <= 2)
    if (const int rc = launch_pairs(e, e->stream)) return rc;
  if (const int rc = launch_cluster_build(e, e->stream)) return rc;
  e->prebuilt = true;
  return SWARM_OK;
}

// ---- the window: run, check

// XCD-aware env placement (swarm::xcd_env_block) once the envs fill the
// eight XCDs evenly (or nearly: 64 and more): whole envs of bpe blocks dealt
// round the XCDs, else `flat` blocks.  bpe: what the kernel takes, 0 if flat.
struct XcdGrid {
  unsigned blocks;
  int bpe;
};
XcdGrid xcd_grid(int E, int bpe, long flat) {
  const bool xcd = E >= 8 && (E % 8 == 0 || E >= 64);
  return {(unsigned)(xcd ? 8L * ((E + 7) / 8) * bpe : flat), xcd ? bpe : 0};
}

// The 2-D cluster window's run kernel (k_cluster_run_wide for latency-bound
// engines, else k_cluster_run) over the current decomposition.
constexpr int kMaxStamps = 512;  // captured run nodes with launch stamps

int launch_run(swarm_engine* e, int n_steps, unsigned long long* tstamp = nullptr) {
  const swarm::EnginePlan& pl = e->plan;
  const long waves = (long)e->n_envs * e->sc.wmax;
  const bool multi = e->params.n_species > 1;
  const bool walls = e->derived.n_walls != 0;
  const bool pot = e->derived.pot.phi != nullptr;  // swarm_engine_set_potential_field
  if (pl.wide_run) {
    // dynamic LDS beyond half a CU's keeps one block (run_wpb run waves) per CU
    const int R = pl.run_wpb;
    // l1_pairs: the next window's candidate lists built beside the run
    const int ncb = e->sc.l1_pairs ? e->n_envs * ((e->n + 1023) / 1024) : 0;
    const dim3 grid((unsigned)(pl.noise_blocks + ncb + (waves + R - 1) / R));
    // one block per CU; with rotation helpers (run_wpb <= 2, round 6) their
    // director tables in the dynamic LDS
    const int helpers = pl.rot_helper && R <= 2 ? 1 : 0;
    const size_t lds = helpers ? std::max<size_t>(96 * 1024, R * swarm::helper_lds_bytes())
                               : 96 * 1024;
    bools([&](auto kMulti, auto kWalls, auto kPot) {
      hipLaunchKernelGGL((swarm::k_cluster_run_wide<kMulti, kWalls, kPot>), grid, dim3(1024), lds,
                         e->stream, e->d_derived, e->st, e->sc, e->n_envs, n_steps, e->d_step,
                         e->d_noise, pl.noise_blocks, R, ncb, pl.lxb, pl.lyb, tstamp, helpers);
    }, multi, walls, pot);
    e->next_table_ready = pl.noise_blocks > 0;
  } else {
    const XcdGrid xg = xcd_grid(e->n_envs, (e->sc.wmax + 3) / 4, (waves + 3) / 4);
    bools([&](auto kTable, auto kMulti, auto kWalls, auto kPot) {
      hipLaunchKernelGGL((swarm::k_cluster_run<kMulti, kTable, kWalls, kPot>), dim3(xg.blocks),
                         dim3(256), 0, e->stream, e->d_derived, e->st, e->sc, e->n_envs, n_steps,
                         e->d_step, e->d_noise, xg.bpe, tstamp);
    }, pl.noise_table, multi, walls, pot);
    e->next_table_ready = false;
  }
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// The 2-D window's exact check (and re-run on failure).  k_check takes each
// mover's candidates from the cells of the window's cell-sorted snapshot in
// global memory: every 2-D build leaves it there (k_build_env too), on the
// build grid.  after_nlist: the window ran on the neighbour-list path.
int launch_check(swarm_engine* e, int n_steps, bool after_nlist = false) {
  const swarm::EnginePlan& pl = e->plan;
  hipLaunchKernelGGL(swarm::k_check, dim3(e->n_envs), dim3(1024),
                     check_lds_bytes(pl.lxg, pl.lyg, e->n, e->params.n_dims), e->stream,
                     e->d_derived, e->st, e->sc, n_steps, e->d_step, e->d_arrive, pl.lxg, pl.lyg,
                     after_nlist ? 1 : 0, pl.lxb, pl.lyb);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int launch_check3(swarm_engine* e, int n_steps, bool after_nlist) {
  const swarm::EnginePlan& pl = e->plan;
  hipLaunchKernelGGL(swarm::k_check3, dim3(e->n_envs), dim3(1024), check3_lds_bytes(e), e->stream,
                     e->d_derived, e->st, e->sc, n_steps, e->d_step, e->d_arrive, pl.lxg, pl.lyg,
                     pl.lzg, after_nlist ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// Enqueue a pending check (swarm_engine::check_pending) as a launch of its
// own.  Every C-ABI entry that touches the engine calls this at its head.
int flush_check(swarm_engine* e) {
  if (!e->check_pending) return SWARM_OK;
  e->check_pending = false;
  return launch_check(e, e->check_steps);
}

// The sub-steps of a neighbour-list window, one launch each (k_nl_step2 in
// 2-D, k_nl_step3 in 3-D: the same arguments and geometry).
int launch_nlist_steps(swarm_engine* e, int n_steps) {
  const bool multi = e->params.n_species > 1;
  const bool walls = e->derived.n_walls != 0;
  const bool three_d = e->params.n_dims == 3;
  const long M = (long)e->n_envs * e->n;
  // latency-bound windows: one wave per workgroup (spread over more CUs);
  // a multiple of 8 workgroups (the kernels' XCD-aware order)
  const int tpb = M <= 32768 ? 64 : 256;
  const dim3 grid((unsigned)(((M + tpb - 1) / tpb + 7) & ~7L));
  for (int s = 0; s < n_steps; ++s) {
    if (!three_d)
      bools([&](auto kWalls, auto kMulti) {
        hipLaunchKernelGGL((swarm::k_nl_step2<kMulti, kWalls>), grid, dim3(tpb), 0, e->stream,
                           e->d_derived, e->st, e->sc, n_steps, s, e->d_step);
      }, walls, multi);
    else
      bools([&](auto kWalls, auto kMulti) {
        hipLaunchKernelGGL((swarm::k_nl_step3<kMulti, kWalls>), grid, dim3(tpb), 0, e->stream,
                           e->d_derived, e->st, e->sc, n_steps, s, e->d_step);
      }, walls, multi);
    HIP_TRY(hipGetLastError());
  }
  return SWARM_OK;
}

// One integration window: cluster build -> cluster run -> check/fallback.
// use_prebuilt: the build ran already; noise_ready: the noise table holds
// this many sub-steps from the current counter.
// may_defer: the caller announced the reward launch (defer_hint) and this is
// the call's last window.
int launch_window(swarm_engine* e, int n_steps, bool use_prebuilt, int noise_ready,
                  bool may_defer = false) {
  const swarm::EnginePlan& pl = e->plan;
  if (!use_prebuilt) {
    const int rc = launch_build(e, e->stream);
    if (rc) return rc;
  }
  if (pl.noise_table && !e->next_table_ready && n_steps > noise_ready) {
    const int rc = launch_noise(e, e->stream, n_steps);
    if (rc) return rc;
  }
  const bool three_d = e->params.n_dims == 3;
  if (pl.nlist_path) {
    if (const int rc = launch_nlist_steps(e, n_steps)) return rc;
    return three_d ? launch_check3(e, n_steps, true) : launch_check(e, n_steps, true);
  }
  if (three_d) {
    const long waves = (long)e->n_envs * e->sc.wmax;
    // one wave per block (so per CU) while the waves fit the chip, else four
    const int tpb = waves <= 256 ? 64 : 256;
    const dim3 grid((unsigned)((waves * 64 + tpb - 1) / tpb));
    bools([&](auto kWalls, auto kMulti, auto kPot) {
      hipLaunchKernelGGL((swarm::k_cluster_run3<kMulti, kWalls, kPot>), grid, dim3(tpb), 0,
                         e->stream, e->d_derived, e->st, e->sc, e->n_envs, n_steps, e->d_step);
    }, e->derived.n_walls != 0, e->params.n_species > 1, e->derived.pot.phi != nullptr);
    HIP_TRY(hipGetLastError());
    return launch_check3(e, n_steps, false);
  }
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool in_graph = false, events = false;
  if (e->profile) {
    // eager: HIP events around the run launch; under stream capture the run
    // node stamps itself (launch stamps below: event-record nodes put ~15 us
    // gaps into the replayed graph)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(e->stream, &cs));
    in_graph = cs == hipStreamCaptureStatusActive;
    events = !in_graph;
  }
  if (events) {
    HIP_TRY(hipEventCreate(&ev0));
    HIP_TRY(hipEventCreate(&ev1));
    HIP_TRY(hipEventRecord(ev0, e->stream));
  }
  unsigned long long* tstamp = nullptr;
  if (e->profile && in_graph && e->d_tstamp && e->stamp_next < kMaxStamps)
    tstamp = e->d_tstamp + (size_t)2 * swarm::kStampSub * e->stamp_next++;
  // the check and the launches up to the next run record their roles in
  // this run's slot (profiling under capture only)
  e->sc.rstamp = tstamp && e->d_rstamp
                     ? e->d_rstamp + (size_t)(e->stamp_next - 1) * 2 * swarm::kRoles *
                                         swarm::kStampSub
                     : nullptr;
  int rc = launch_run(e, n_steps, tstamp);
  if (rc) return rc;
  if (events) {
    HIP_TRY(hipEventRecord(ev1, e->stream));
    e->prof_events.emplace_back(ev0, ev1);
  }
  if (may_defer && pl.defer_check && pl.wide_run && e->sc.l1_pairs) {
    e->check_pending = true;
    e->check_steps = n_steps;
    return SWARM_OK;
  }
  return launch_check(e, n_steps);
}

int run_bd(swarm_engine* e, int n_steps) {
  const bool hint = e->defer_hint;  // one-shot
  e->defer_hint = false;
  if (e->ride_stage > 0) {  // a deferred build no launch carried along
    const int rc = flush_ride_along(e);
    if (rc) return rc;
  }
  bool pre = e->prebuilt;
  int noise_ready = e->prebuilt_noise_steps;
  e->prebuilt = false;
  e->prebuilt_noise_steps = 0;
  while (n_steps > 0) {
    const int w = std::min(n_steps, swarm::kMaxWindow);
    const int rc = e->plan.cluster_path
                       ? launch_window(e, w, pre, noise_ready, hint && w == n_steps)
                       : launch_global(e, w, 0, 0.0f, 0.0f);
    if (rc) return rc;
    pre = false;
    noise_ready = 0;
    n_steps -= w;
  }
  return SWARM_OK;
}

// ---- observables: the cell grid, the vision cone, the reward

int ensure_grid_scratch(swarm_engine* e, int lx, int ly) {
  const size_t need = (size_t)e->n_envs * ((size_t)(1 << (lx + ly)) + 1);
  if (need > e->start_cap) {
    // the speculative vision grid's saved arguments point into the old buffer
    e->vgrid_ready = false;
    e->spec_ok = false;
    e->start_cap = 0;
    HIP_TRY(dev_free(e, &e->d_start));
    HIP_TRY(dev_malloc(e, &e->d_start, need * sizeof(int32_t)));
    e->start_cap = need;
  }
  return SWARM_OK;
}

int build_grid(swarm_engine* e, int lx, int ly) {
  int rc = ensure_grid_scratch(e, lx, ly);
  if (rc) return rc;
  // this grid overwrites the cell starts a speculative vision grid left
  e->vgrid_ready = false;
  const int ncell = 1 << (lx + ly);
  const size_t lds = 16 * 4 + (size_t)(ncell + 1) * 4;
  if (lds > kMaxLds) return fail(SWARM_ECAPACITY, "observable cell grid too large");
  hipLaunchKernelGGL(k_grid_build, dim3(e->n_envs), dim3(1024), lds, e->stream, e->st, lx, ly,
                     e->d_start, e->d_order);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

bool same_grid_args(const VisionArgs& a, const VisionArgs& b) {
  return std::memcmp(&a.vp, &b.vp, sizeof(a.vp)) == 0 && a.lx == b.lx && a.ly == b.ly &&
         a.radii == b.radii && a.types == b.types && a.agents == b.agents &&
         a.n_agents == b.n_agents && a.n_envs == b.n_envs;
}

int l1_blocks_per_env(const swarm_engine* e) { return e->sc.l1_pairs ? (e->n + 1023) / 1024 : 0; }

// pol (swarm_engine_vision_policy): the rollout policy of the cone's agents
// runs in the cone's launch (PolicyTail); the caller checked its limits
// (n_cones * n_types <= 4 = d_in, k <= 4, hidden <= 256).
int vision_cone_impl(swarm_engine_t* e, const swarm_vision_params_t* vp, const int32_t* agent_idx,
                     int32_t n_agents, const float* radii, const int32_t* types, float* out,
                     bool persistent, const swarm::MlpArgs* pol = nullptr) {
  if (!e || !vp || !agent_idx || !radii || !types || !out) return fail(SWARM_EINVAL, "null argument");
  const swarm::EnginePlan& pl = e->plan;
  if (const int frc = flush_check(e)) return frc;
  if (e->params.n_dims != 2) return fail(SWARM_EINVAL, "the vision-cone kernel is 2-D only");
  if (vp->n_cones < 1 || vp->n_cones > SWARM_MAX_CONES || vp->n_types < 1 ||
      vp->n_types > SWARM_MAX_DETECTED_TYPES || vp->n_cones * vp->n_types > 2 * SWARM_MAX_CONES)
    return fail(SWARM_ECAPACITY, "n_cones * n_types exceeds this build's limit (32)");
  if (n_agents <= 0) return SWARM_OK;
  if (e->n >= (1 << 24)) return fail(SWARM_ECAPACITY, "vision records hold particle ids < 2^24");
  // a range of half the box or more: every record is a candidate (k_vision<.., kAll>)
  const bool all = !(2.0 * vp->vision_range < std::min(e->params.box[0], e->params.box[1]));
  int lx, ly;
  cell_grid(e->params, e->n, (double)vp->vision_range, &lx, &ly);
  int rc = ensure_grid_scratch(e, lx, ly);
  if (rc) return rc;
  // records staged in LDS when the env's fit (N <= 8 x 1024: the register path)
  const bool staged = e->n <= 8 * 1024 && vision_grid_lds_bytes(lx, ly, e->n, true) <= kMaxLds;
  const VisionArgs va{*vp,          lx,        ly,    radii, types, agent_idx, n_agents,
                      e->d_start,   e->vs,     out,   e->n_envs, staged ? 1 : 0, e->sc.rstamp};
  const long total = (long)e->n * e->n_envs;  // one group per sorted particle
  const int nb = vp->n_cones * vp->n_types;
  // lanes per agent: enough threads to give every SIMD a few waves, few
  // enough that the lanes of a wave stay busy (measured, tools/vision_time.py:
  // 64 x 4096 agents 107 -> 93 us with G = 4 instead of 1)
  int G = total >= (1L << 15) ? kVisionGWide : 16;
  if (const char* og = std::getenv("SWARMRL_AMD_VISION_G")) {
    const int v = std::atoi(og);
    if (v == kVisionGWide || v == 16) G = v;
  }
  const size_t glds = vision_grid_lds_bytes(lx, ly, e->n, staged);
  if (glds > kMaxLds) return fail(SWARM_ECAPACITY, "observable cell grid too large");
  // the grid of the current positions for these arguments, built by the
  // reward launch (launch_field) while nothing moved the colloids since
  const bool l1 = e->sc.l1_pairs != 0;
  const bool have_grid = !all && e->vgrid_ready && e->ride_stage == (l1 ? 3 : 2) &&
                         same_grid_args(e->spec_va, va);
  e->vgrid_ready = false;
  e->spec_ok = persistent && !all;
  if (e->spec_ok) e->spec_va = va;
  // a deferred build rides along in the grid and cone launches (stages 1, 2;
  // with l1_pairs the pair search rides in the grid's launch and the
  // cluster build, stage 3, in the fused policy's or the policy's launch)
  // when their fused variants apply; else its pending stages launch first
  const bool ride_ok = !all && nb <= 4 && G == 16;
  if (e->ride_stage > 0 && !(ride_ok && (e->ride_stage <= 2 || (l1 && e->ride_stage == 3)))) {
    rc = flush_ride_along(e);
    if (rc) return rc;
  }
  if (e->ride_stage == 1) {  // grid | sort (| pairs), then cone | pairs or cluster build
    const size_t slds = sort_lds_bytes(e);
    const int nfb = l1_blocks_per_env(e);
    const dim3 grid((unsigned)((2 + nfb) * e->n_envs));
    const size_t lds = l1_launch_lds(e, std::max(glds, slds));
    swarm_select::sort_chunk(e->n, [&](auto ch) {
      hipLaunchKernelGGL((k_vgrid_sort<ch>), grid, dim3(1024), lds, e->stream, e->st, va, e->sc,
                         pl.lxb, pl.lyb, e->d_derived, nfb, e->d_step);
    });
    HIP_TRY(hipGetLastError());
    e->ride_stage = l1 ? 3 : 2;
  } else if (!have_grid) {
    hipLaunchKernelGGL(k_vision_grid, dim3(e->n_envs), dim3(1024), glds, e->stream, e->st, va);
    HIP_TRY(hipGetLastError());
  }
  if (pol && ride_ok && e->ride_stage == 3) {  // cluster build | cone + policy (l1_pairs)
    // 32 lanes per agent: with the actor rows staged in LDS the cone's bins
    // are summed ~1.5 us sooner and the MLP tail no longer outweighs it
    // (same box: head 53.1 -> 53.3 M, C2 14.5 -> 14.8 M; with the rows read
    // from L2 the tail took ~2 us longer and 16 lanes won)
    constexpr int GC = 32;
    const int ncb = (int)((total * GC + 1023) / 1024);
    const size_t rows = ((size_t)pol->hidden * swarm::MlpRow<4, 4>::kStride + 4) * sizeof(float);
    const size_t lds = std::max(build_lds_bytes(e->n, e->sc.pair_cap),
                                (size_t)kVisionHits * 1024 * sizeof(uint32_t) + rows);
    hipLaunchKernelGGL((k_vision_policy_cbuild<4, GC, 4, 4>), dim3((unsigned)(e->n_envs + ncb)),
                       dim3(1024), lds, e->stream, e->st, e->d_derived, va, *pol, e->sc);
    HIP_TRY(hipGetLastError());
    e->ride_stage = 0;
    e->prebuilt = true;
    return SWARM_OK;
  }
  if (e->ride_stage == 2) {  // pairs | cone (+ policy)
    const int nvb = (int)((total * 16 + 255) / 256);
    const int pbx = (e->n + 255) / 256;
    const int npb = pbx * e->n_envs;
    const dim3 grid((unsigned)(nvb + npb));
    if (pol)
      bools([&](auto local) {
        hipLaunchKernelGGL((k_vision_policy_pairs<4, 16, local, 4, 4>), grid, dim3(256), 0,
                           e->stream, e->st, e->d_derived, va, *pol, npb, e->sc, pl.lxb, pl.lyb, pbx);
      }, e->sc.local_uf != 0);
    else
      bools([&](auto local) {
        hipLaunchKernelGGL((k_vision_pairs<4, 16, local>), grid, dim3(256), 0, e->stream, e->st,
                           e->d_derived, va, npb, e->sc, pl.lxb, pl.lyb, pbx);
      }, e->sc.local_uf != 0);
    HIP_TRY(hipGetLastError());
    e->ride_stage = 3;
    return SWARM_OK;
  }
  if (all) {
    if (pol) return fail(SWARM_ECAPACITY, "the fused policy needs vision_range < half the box");
    const dim3 agrid((unsigned)((total * 16 + 255) / 256));
    swarm_select::bins(nb, [&](auto kBins) {
      hipLaunchKernelGGL((k_vision<kBins, 16, true>), agrid, dim3(256), 0, e->stream, e->st,
                         e->d_derived, va, 0);
    });
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  }
  // XCD-aware env placement once the envs fill the eight XCDs (as k_cluster_run)
  const XcdGrid xg =
      xcd_grid(e->n_envs, (int)(((long)e->n * G + 255) / 256), (total * G + 255) / 256);
  if (pol)  // cone + policy, no build stage riding along
    swarm_select::cone_lanes(G, [&](auto kLanes) {
      hipLaunchKernelGGL((k_vision_policy<4, kLanes, 4, 4>), dim3(xg.blocks), dim3(256), 0,
                         e->stream, e->st, e->d_derived, va, *pol, xg.bpe);
    });
  else
    swarm_select::bins(nb, [&](auto kBins) {
      swarm_select::cone_lanes(G, [&](auto kLanes) {
        hipLaunchKernelGGL((k_vision<kBins, kLanes>), dim3(xg.blocks), dim3(256), 0, e->stream,
                           e->st, e->d_derived, va, xg.bpe);
      });
    });
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// k_field, or with a pending deferred build and a persistent vision cone the
// fused k_field_vgrid_sort (stage 1 and the next observable's grid ride
// along in the reward launch).
int launch_field(swarm_engine* e, const FieldArgs& f) {
  const swarm::EnginePlan& pl = e->plan;
  const int total = f.n_agents * e->n_envs;
  // the reward launch of a slice with a deferred build carries stage 1 (and
  // the l1_pairs pair search), and for a persistent vision cone the next
  // observable's grid; without a vision cone only with l1_pairs (the
  // cluster build then rides in the policy launch: k_policy_cbuild)
  const bool grid_too = e->spec_ok;
  if (e->ride_stage == 1 && (grid_too || e->sc.l1_pairs)) {
    VisionArgs none{};
    none.n_envs = e->n_envs;
    const VisionArgs& va = grid_too ? e->spec_va : none;
    const size_t glds = grid_too ? vision_grid_lds_bytes(va.lx, va.ly, e->n, va.staged != 0) : 0;
    const size_t slds = sort_lds_bytes(e);
    const int nfb = (total + 1023) / 1024;
    const int npf = l1_blocks_per_env(e);  // l1_pairs: the pair search rides here too
    dim3 grid((unsigned)(nfb + (2 + npf) * e->n_envs));
    size_t lds = l1_launch_lds(e, std::max(glds, slds));
    CheckArgs ck{};
    bool with_check = false;
    if (e->check_pending) {
      // the window's check rides along as the first workgroups of the launch
      // while every workgroup is resident (the other roles wait for its
      // verdict) and the check's LDS (4 KB of it static) fits
      const dim3 cgrid((unsigned)(nfb + (3 + npf) * e->n_envs));
      const size_t clds = std::max(lds, check_lds_bytes(pl.lxg, pl.lyg, e->n, e->params.n_dims));
      with_check = (int)cgrid.x <= e->n_cus && clds + 4096 <= kMaxLds;
      if (with_check) {
        ck = CheckArgs{e->check_steps, e->d_step, e->d_arrive, pl.lxg, pl.lyg, pl.lxb, pl.lyb};
        grid = cgrid;
        lds = clds;
      } else if (const int rc = flush_check(e)) {
        return rc;
      }
    }
    swarm_select::sort_chunk(e->n, [&](auto ch) {
      bools([&](auto check) {
        hipLaunchKernelGGL((k_field_vgrid_sort<ch, check>), grid, dim3(1024), lds, e->stream, f,
                           nfb, e->st, va, e->sc, pl.lxb, pl.lyb, e->d_derived, npf, e->d_step,
                           grid_too ? 1 : 0, ck);
      }, with_check);
    });
    HIP_TRY(hipGetLastError());
    if (with_check) e->check_pending = false;
    e->ride_stage = e->sc.l1_pairs ? 3 : 2;
    e->vgrid_ready = grid_too;
    return SWARM_OK;
  }
  // no launch to carry a pending check (the last slice of an episode)
  if (const int frc = flush_check(e)) return frc;
  hipLaunchKernelGGL(k_field, dim3((total + 255) / 256), dim3(256), 0, e->stream, e->st, f);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

}  // namespace
