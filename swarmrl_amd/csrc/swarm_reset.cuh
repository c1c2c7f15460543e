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

__global__ __launch_bounds__(256) void k_place_envs(const Derived* __restrict__ d, DevState st,
                                                    ResetArgs a) {
  const int N = st.n;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)a.n_listed * N) return;
  const int k = (int)(t / N), i = (int)(t - (long)k * N);
  const int env = a.envs[k];
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
    c.y = (uint32_t)a.ordinal;
    c.z = (uint32_t)(a.ordinal >> 32);
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

}  // namespace swarm
