// swarm_reset.cuh -- in-place reset of chosen envs (swarm_engine_reset_envs):
// a fresh random start on the device, then the overlap removal of those envs
// alone (DESIGN.md section 3 "Reset placement", section 10 "In-place reset").
//
//   k_place_envs     one thread per (listed env, particle): a particle of a
//                    placement group is drawn uniformly in the group's disc
//                    (2-D) or ball (3-D) with a uniform director, every other
//                    particle returns to its home state; velocities, actions
//                    and both reuse_forces slots as a fresh engine has them.
//   k_global_envs    k_global in steepest-descent mode, env = envs[blockIdx.x]
//   k_global3_envs   k_global3 likewise
//
//   k_place_marked, k_count_marked, k_global_marked, k_global3_marked,
//   k_field_history_marked    the same for the envs a device mask marks
//                    (swarm_engine_reset_marked, swarm_field_history_marked)
//
// An env that is not listed is not touched by a single store.
#pragma once

#include "swarm_device.cuh"
#include "swarm_integrator.cuh"
#include "swarm_integrator3.cuh"

namespace swarm {

// Philox stream tags of the placement: counter (particle, reset ordinal lo,
// hi, kResetTag + b), b = 0, 1 (the second block in 3-D only).  Apart from
// the Brownian groups (kGroupTag + 0..2), the velocity draws (tags 1, 2) and
// kLangevinTag.
constexpr uint32_t kResetTag = 0x30u;

// A placement group's centre in the engine's fixed point, and its radius.
struct ResetGroup {
  uint32_t cq[3];
  int32_t cimg[3];
  float radius;
  int32_t reserved;
};

struct ResetArgs {
  const int32_t* envs;         // [n_listed] the envs to reset
  int32_t n_listed;
  const int32_t* group_of;     // [N] the particle's group, -1: home
  const ResetGroup* groups;
  const uint32_t* home_q;      // [3][M]
  const int32_t* home_img;     // [3][M]
  const uint32_t* home_ang;    // [M]
  const float* home_dir3;      // [3][M] (3-D)
  uint64_t ordinal;            // the engine's reset counter
  int32_t* cand_ok;            // [E] Scratch::cand_ok
};

// U = (word >> 8) 2^-24 in [0, 1)
__device__ __forceinline__ float unit_from_word(uint32_t w) {
  return (float)(w >> 8) * 5.9604644775390625e-08f;
}

// The centre's coordinate moved by dx (|dx| below half the box edge).
__device__ __forceinline__ void place_axis(uint32_t cq, int32_t cimg, float dx, float inv_sx,
                                           uint32_t* q, int32_t* img) {
  *q = cq;
  *img = cimg;
  advance(*q, *img, f2i32(dx * inv_sx));
}

// Particle i of env: its placement with this reset ordinal and everything a
// fresh engine has beside it (the body of k_place_envs and k_place_marked).
__device__ __forceinline__ void place_particle(const Derived* __restrict__ d, const DevState& st,
                                               const ResetArgs& a, int env, int i,
                                               uint64_t ordinal) {
  const int N = st.n;
  const size_t M = (size_t)st.m, gi = (size_t)env * N + i;
  const bool three_d = st.dims == 3;

  uint32_t q[3] = {a.home_q[gi], a.home_q[M + gi], a.home_q[2 * M + gi]};
  int32_t img[3] = {a.home_img[gi], a.home_img[M + gi], a.home_img[2 * M + gi]};
  uint32_t ang = a.home_ang[gi];
  float dir[3] = {0.0f, 0.0f, 0.0f};
  if (three_d) {
    dir[0] = a.home_dir3[gi];
    dir[1] = a.home_dir3[M + gi];
    dir[2] = a.home_dir3[2 * M + gi];
  }

  const int g = a.group_of[i];
  if (g >= 0) {
    const ResetGroup grp = a.groups[g];
    const uint32_t k0 = d->key0, k1 = d->key1 ^ (uint32_t)env;
    u32x4 c;
    c.x = (uint32_t)i;
    c.y = (uint32_t)ordinal;
    c.z = (uint32_t)(ordinal >> 32);
    c.w = kResetTag;
    const u32x4 r = philox4x32_10(c, k0, k1);
    float sn, cs;
    if (!three_d) {
      // radius R max(U1, U2), polar angle and director angle as turn words
      const float rad = grp.radius * fmaxf(unit_from_word(r.x), unit_from_word(r.y));
      sincos_turn(r.z, &sn, &cs);
      place_axis(grp.cq[0], grp.cimg[0], rad * cs, d->inv_sx[0], &q[0], &img[0]);
      place_axis(grp.cq[1], grp.cimg[1], rad * sn, d->inv_sx[1], &q[1], &img[1]);
      ang = r.w;
    } else {
      c.w = kResetTag + 1u;
      const u32x4 r2 = philox4x32_10(c, k0, k1);
      const float rad = grp.radius * fmaxf(fmaxf(unit_from_word(r.x), unit_from_word(r.y)),
                                           unit_from_word(r.z));
      // a uniform direction: z = 2 U - 1, azimuth a turn word
      const float zc = 2.0f * unit_from_word(r2.x) - 1.0f;
      const float sxy = sqrt_rn(1.0f - zc * zc);
      sincos_turn(r.w, &sn, &cs);
      place_axis(grp.cq[0], grp.cimg[0], rad * (sxy * cs), d->inv_sx[0], &q[0], &img[0]);
      place_axis(grp.cq[1], grp.cimg[1], rad * (sxy * sn), d->inv_sx[1], &q[1], &img[1]);
      place_axis(grp.cq[2], grp.cimg[2], rad * zc, d->inv_sx[2], &q[2], &img[2]);
      const float zd = 2.0f * unit_from_word(r2.y) - 1.0f;
      const float sd = sqrt_rn(1.0f - zd * zd);
      sincos_turn(r2.z, &sn, &cs);
      dir[0] = sd * cs;
      dir[1] = sd * sn;
      dir[2] = zd;
      ang = 0u;
    }
  }

#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    st.q[ax * M + gi] = q[ax];
    st.img[ax * M + gi] = img[ax];
    st.vel[ax * M + gi] = 0.0f;
  }
  st.ang[gi] = ang;
  st.omega[gi] = 0.0f;
  st.f_swim[gi] = 0.0f;
  st.torque_z[gi] = 0.0f;
  if (three_d) {
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) st.dir3[ax * M + gi] = dir[ax];
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
      st.omega_xy[ax * M + gi] = 0.0f;
      st.torque_xy[ax * M + gi] = 0.0f;
    }
  }
  // both reuse_forces slots as after a fresh upload and its overlap removal:
  // no action yet, the orientation just placed
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const PrevSlot w = prev_slot(st, p);
    w.f[gi] = 0.0f;
    w.tz[gi] = 0.0f;
    w.ang[gi] = ang;
    if (three_d) {
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) w.dir3[ax * M + gi] = dir[ax];
      w.txy[gi] = 0.0f;
      w.txy[M + gi] = 0.0f;
    }
  }
  // the candidate lists of the env's last window (l1_pairs) list the old
  // positions' neighbours
  if (i == 0) a.cand_ok[env] = 0;
}

__global__ __launch_bounds__(256) void k_place_envs(const Derived* __restrict__ d, DevState st,
                                                    ResetArgs a) {
  const int N = st.n;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)a.n_listed * N) return;
  const int k = (int)(t / N), i = (int)(t - (long)k * N);
  place_particle(d, st, a, a.envs[k], i, a.ordinal);
}

// k_global's steepest descent over the listed envs.
__global__ __launch_bounds__(1024) void k_global_envs(const Derived* __restrict__ d, DevState st,
                                                      Scratch sc,
                                                      const int32_t* __restrict__ envs,
                                                      int n_steps,
                                                      const uint64_t* __restrict__ step_ctr,
                                                      int lx, int ly, float g, float md) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ PairTables pt;
  stage_pair_tables(d, &pt);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  const int env = envs[blockIdx.x];
  // steepest descent writes the reuse_forces slot the next window reads (k_global)
  const int par = window_parity(step_ctr);
  if (global_lds_extra_words(st.n, st.dims, 1 << (lx + ly)) && blockDim.x == 1024 && d->periodic)
    block_env_run(d, st, env, n_steps, 0ull, lx, ly, true, g, md, cnt, wave_sums,
                  cnt + (1 << (lx + ly)) + 1, &pt, par, PlainEnvPath{});
  else
    block_global_run(d, st, sc, env, n_steps, 0ull, lx, ly, true, g, md, cnt, wave_sums, &pt,
                     par);
  save_forces_env(st, env, par);
}

// k_global3's steepest descent over the listed envs.
__global__ __launch_bounds__(1024) void k_global3_envs(const Derived* __restrict__ d, DevState st,
                                                       Scratch sc,
                                                       const int32_t* __restrict__ envs,
                                                       int n_steps,
                                                       const uint64_t* __restrict__ step_ctr,
                                                       int lx, int ly, int lz, float g, float md) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ PairTables pt;
  stage_pair_tables(d, &pt);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  const int env = envs[blockIdx.x];
  const int par = window_parity(step_ctr);
  block_global_run3(d, st, sc, env, n_steps, 0ull, lx, ly, lz, true, g, md, cnt, wave_sums, &pt,
                    par);
  save_forces_env(st, env, par);
}

// ---- swarm_engine_reset_marked: the envs a device mask marks.  Every grid is
// the full one whatever the mask holds, so the launches can sit in a captured
// graph; a thread (workgroup) of an unmarked env returns before any store
// (before its first barrier).

// Bit 63 of a marked reset's ordinal: apart from the host path's 0, 1, ...
constexpr uint64_t kMarkedOrdinal = 1ull << 63;

// k_place_envs over every env: env e draws with the ordinal 2^63 | counts[e],
// the device-mask resets it has had.  k_count_marked bumps counts after this
// launch: threads of one env sit in several workgroups here.
__global__ __launch_bounds__(256) void k_place_marked(const Derived* __restrict__ d, DevState st,
                                                      ResetArgs a,
                                                      const uint8_t* __restrict__ mask,
                                                      const uint32_t* __restrict__ counts) {
  const int N = st.n;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)a.n_listed * N) return;
  const int env = (int)(t / N), i = (int)(t - (long)env * N);
  if (!mask[env]) return;
  place_particle(d, st, a, env, i, kMarkedOrdinal | counts[env]);
}

__global__ __launch_bounds__(256) void k_count_marked(const uint8_t* __restrict__ mask,
                                                      uint32_t* __restrict__ counts, int n_envs) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env < n_envs && mask[env]) counts[env] += 1u;
}

// k_global_envs with env = blockIdx.x, marked envs only.
__global__ __launch_bounds__(1024) void k_global_marked(const Derived* __restrict__ d, DevState st,
                                                        Scratch sc,
                                                        const uint8_t* __restrict__ mask,
                                                        int n_steps,
                                                        const uint64_t* __restrict__ step_ctr,
                                                        int lx, int ly, float g, float md) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ PairTables pt;
  const int env = blockIdx.x;
  if (!mask[env]) return;  // (the whole workgroup: before stage_pair_tables' barrier)
  stage_pair_tables(d, &pt);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  const int par = window_parity(step_ctr);
  if (global_lds_extra_words(st.n, st.dims, 1 << (lx + ly)) && blockDim.x == 1024 && d->periodic)
    block_env_run(d, st, env, n_steps, 0ull, lx, ly, true, g, md, cnt, wave_sums,
                  cnt + (1 << (lx + ly)) + 1, &pt, par, PlainEnvPath{});
  else
    block_global_run(d, st, sc, env, n_steps, 0ull, lx, ly, true, g, md, cnt, wave_sums, &pt,
                     par);
  save_forces_env(st, env, par);
}

// k_global3_envs likewise.
__global__ __launch_bounds__(1024) void k_global3_marked(const Derived* __restrict__ d,
                                                         DevState st, Scratch sc,
                                                         const uint8_t* __restrict__ mask,
                                                         int n_steps,
                                                         const uint64_t* __restrict__ step_ctr,
                                                         int lx, int ly, int lz, float g,
                                                         float md) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ PairTables pt;
  const int env = blockIdx.x;
  if (!mask[env]) return;
  stage_pair_tables(d, &pt);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  const int par = window_parity(step_ctr);
  block_global_run3(d, st, sc, env, n_steps, 0ull, lx, ly, lz, true, g, md, cnt, wave_sums, &pt,
                    par);
  save_forces_env(st, env, par);
}

// swarm_field_history_marked: the fixed-point position history of k_field
// (hist_q, hist_img [3][E * A], slot env * A + agent) <- the current q / img
// for the agents of marked envs, as k_field's init_only does for every env.
__global__ __launch_bounds__(256) void k_field_history_marked(DevState st,
                                                              const uint8_t* __restrict__ mask,
                                                              const int32_t* __restrict__ agents,
                                                              int n_agents, int n_envs,
                                                              uint32_t* __restrict__ hq,
                                                              int32_t* __restrict__ himg) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int A = n_agents * n_envs;
  if (t >= A) return;
  const int e = t / n_agents, ai = t - e * n_agents;
  if (!mask[e]) return;
  const size_t M = (size_t)st.m, gi = (size_t)e * st.n + agents[ai];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    hq[(size_t)a * A + t] = a < st.dims ? st.q[a * M + gi] : 0u;
    himg[(size_t)a * A + t] = a < st.dims ? st.img[a * M + gi] : 0;
  }
}

}  // namespace swarm
