// swarm_langevin.cuh -- the Langevin thermostat (2-D, periodic box, spheres
// with isotropic friction) and the coupling to a gridded flow field.
//
// Replaces what EspressoMD does for MDParams(thermostat_type="langevin"):
// integrator.set_vv() with thermostat.set_langevin (espresso.py:1171-1190) and
// the FlowField constraint of add_flowfield (espresso.py:940-993).  Inertial
// dynamics with a per-particle mass and rotational inertia: the velocities
// (DevState::vel, DevState::omega) are integrator state here, they carry from
// run to run.
//
// An engine under this thermostat (swarm_engine_set_langevin) runs every
// sub-step and the overlap removal on k_langevin_run, one workgroup per env, a
// path of block_env_run (swarm_env_block.cuh): PlainEnvPath's potential and
// walls, the flow lookup beside the potential's, and a step of its own with
// the env's velocities in the LDS tail (v_x[N], v_y[N], omega[N]).
//
// The step is ONE fp32 operation sequence ("Langevin step" and
// "Flow field"); tests/csrc/langevin_oracle.c restates it line by line.
#pragma once

#include "swarm_integrator.cuh"

namespace swarm {

// Philox stream tag of the thermostat's noise: one block per (particle,
// sub-step), counter (id, step lo, step hi, kLangevinTag).  Apart from the
// Brownian groups (kGroupTag + 0..2) and the velocity draw (tag 1).
constexpr uint32_t kLangevinTag = 0x20u;

// Per-engine constants of the Langevin path (device memory).  Host:
// swarm_engine_set_langevin, swarm_engine_set_flow_field; fp64, rounded once.
struct LangevinArgs {
  float dt_m[kMaxSpecies], dt_i[kMaxSpecies];  // dt / m, dt / I
  float gam[kMaxSpecies];                      // gamma_t + gamma_flow
  float gam_r[kMaxSpecies];
  // sqrt(24 kT gamma / dt): the uniform noise's amplitude (0 without noise)
  float sig_t[kMaxSpecies], sig_r[kMaxSpecies];
  float dt_sx[2];  // dt / sx: a velocity in fixed-point units per sub-step
  float dt;
  // the flow field; flow null: none.  One record of 32 bytes per cell
  //   rec[i0x][i0y] = {ux00, ux10, ux01, ux11, uy00, uy10, uy01, uy11},
  //   u_ab = u[(i0x + a) mod n0][(i0y + b) mod n1],
  // built by the host: two 16-byte loads per lookup and no i1 arithmetic
  const float* flow;
  int32_t fn[2];
  float gflow;
};

// The flow velocity at box fractions (qx, qy): the potential's cell and weight
// (pot_axis), per component
//   a = u00 + tx (u10 - u00),  b = u01 + tx (u11 - u01),  u = a + ty (b - a).
__device__ __forceinline__ void flow_sample2(const float* __restrict__ rec, uint32_t nx,
                                             uint32_t ny, uint32_t qx, uint32_t qy, float* ux,
                                             float* uy) {
  const PotAxis x = pot_axis(qx, nx), y = pot_axis(qy, ny);
  const float4* c = reinterpret_cast<const float4*>(rec) + 2 * ((size_t)x.i0 * ny + y.i0);
  const float4 cx = c[0], cy = c[1];
  const float ax = cx.x + x.t * (cx.y - cx.x), bx = cx.z + x.t * (cx.w - cx.z);
  *ux = ax + y.t * (bx - ax);
  const float ay = cy.x + x.t * (cy.y - cy.x), by = cy.z + x.t * (cy.w - cy.z);
  *uy = ay + y.t * (by - ay);
}

// U - 1/2 from a Philox word: U = (word >> 8) 2^-24, the difference exact.
__device__ __forceinline__ float centred_uniform(uint32_t w) {
  return (float)(w >> 8) * 5.9604644775390625e-08f - 0.5f;
}

// One Langevin sub-step of one particle from its force sum (ax, ay; 2^-24
// units, pairs and walls) and the external force (fex, fey: constant force,
// potential and gamma_flow u).  v: the particle's (v_x, v_y, omega), updated.
// an_swim as in bd_step.  Sequence: DESIGN.md §3.
__device__ __forceinline__ void langevin_step(const LangevinArgs* __restrict__ lv, int sp,
                                              bool noisy, PState& p, float v[3], int64_t ax,
                                              int64_t ay, float fs, float tz, float fex, float fey,
                                              uint32_t k0, uint32_t k1, uint32_t id, uint64_t step,
                                              uint32_t an_swim) {
  float sn, cs;
  sincos_turn(an_swim, &sn, &cs);
  float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
  if (noisy) {
    u32x4 c;
    c.x = id;
    c.y = (uint32_t)step;
    c.z = (uint32_t)(step >> 32);
    c.w = kLangevinTag;
    const u32x4 r = philox4x32_10(c, k0, k1);
    n0 = centred_uniform(r.x);
    n1 = centred_uniform(r.y);
    n2 = centred_uniform(r.z);
  }
  const float c1x = fex + fs * cs, c1y = fey + fs * sn;
  const float fx = __builtin_fmaf(i64_to_f32(ax), 5.9604644775390625e-08f, c1x);
  const float fy = __builtin_fmaf(i64_to_f32(ay), 5.9604644775390625e-08f, c1y);
  const float gam = lv->gam[sp], sg = lv->sig_t[sp], dtm = lv->dt_m[sp];
  // F = f - (gamma_t + gamma_flow) v + sig (U - 1/2);  v += (dt / m) F
  const float Fx = __builtin_fmaf(sg, n0, __builtin_fmaf(-gam, v[0], fx));
  const float Fy = __builtin_fmaf(sg, n1, __builtin_fmaf(-gam, v[1], fy));
  const float Tq = __builtin_fmaf(lv->sig_r[sp], n2, __builtin_fmaf(-lv->gam_r[sp], v[2], tz));
  v[0] = __builtin_fmaf(dtm, Fx, v[0]);
  v[1] = __builtin_fmaf(dtm, Fy, v[1]);
  v[2] = __builtin_fmaf(lv->dt_i[sp], Tq, v[2]);
  advance(p.qx, p.ix, f2i32_sat(v[0] * lv->dt_sx[0]));
  advance(p.qy, p.iy, f2i32_sat(v[1] * lv->dt_sx[1]));
  const float dth = v[2] * lv->dt;
  p.an = p.an + (uint32_t)f2i32_sat(dth * kAngInvScale);
}

// block_env_run under the Langevin thermostat: the plain colloid's potential
// and walls, the flow's drag beside the potential's force, and the inertial
// step on the velocities in the LDS tail.  The overlap removal is sd_step,
// with the flow at v = 0; it leaves the velocities alone.
struct LangevinEnvPath : PlainEnvPath {
  static constexpr bool kStamps = false;
  const LangevinArgs* __restrict__ lv;
  __device__ __forceinline__ void field(const EnvRun& r, const PState& p, float& fex,
                                        float& fey) const {
    PlainEnvPath::field(r, p, fex, fey);
    if (lv->flow) {
      float ux, uy;
      flow_sample2(lv->flow, (uint32_t)lv->fn[0], (uint32_t)lv->fn[1], p.qx, p.qy, &ux, &uy);
      fex = fex + lv->gflow * ux;
      fey = fey + lv->gflow * uy;
    }
  }
  template <class L>
  __device__ __forceinline__ bool step(const EnvRun& r, const L& l, int s, bool,
                                       const EnvParticle& q, PState& p, float2, EnvAcc& a,
                                       int& any) const {
    if (r.d->n_walls) {
      int64_t az = 0;
      wall_forces<2>(r.d, q.sik, (float)p.qx * r.sx0, (float)p.qy * r.sx1, 0.0f, a.ax, a.ay, az,
                     r.st.wall_viol);
    }
    if (r.sd_mode) {
      any |= sd_step(load_pconst(r.d, q.sik), p, a.ax, a.ay, q.fs, q.tz, q.fex, q.fey, r.g, r.md)
                 ? 1
                 : 0;
      return true;
    }
    float* vt = reinterpret_cast<float*>(l.tail);
    const int N = r.st.n;
    float v[3] = {vt[q.i], vt[N + q.i], vt[2 * N + q.i]};
    langevin_step(lv, q.sik, r.d->noisy != 0, p, v, a.ax, a.ay, q.fs, q.tz, q.fex, q.fey, r.k0,
                  r.k1, (uint32_t)q.i, r.step0 + (uint64_t)s, q.first ? r.prv.ang[q.gi] : p.an);
    vt[q.i] = v[0];
    vt[N + q.i] = v[1];
    vt[2 * N + q.i] = v[2];
    return true;
  }
};

// Langevin-engine launch: n_steps sub-steps (or SD steps) of every env, one
// 1024-thread workgroup per env (k_global's contract: reuse_forces slots,
// device step counter).  The velocities are read into the LDS tail before the
// first sub-step and written back after the last.
__global__ __launch_bounds__(1024) void k_langevin_run(
    const Derived* __restrict__ d, DevState st, const LangevinArgs* __restrict__ lv, int n_steps,
    uint64_t* __restrict__ step_ctr, uint32_t* __restrict__ arrive, int lx, int ly, int sd_mode,
    float g, float md) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ PairTables pt;
  stage_pair_tables(d, &pt);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  int32_t* lsq = cnt + (1 << (lx + ly)) + 1;
  const uint64_t step0 = sd_mode ? 0ull : *step_ctr;
  const int par = window_parity(step_ctr);
  const int N = st.n;
  const size_t M = (size_t)st.m, base = (size_t)blockIdx.x * N;
  float* vt = reinterpret_cast<float*>(env_lds<false>(lsq, N).tail);
  if (!sd_mode) {  // (block_env_run's first barrier orders these before the first step)
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      vt[i] = st.vel[base + i];
      vt[N + i] = st.vel[M + base + i];
      vt[2 * N + i] = st.omega[base + i];
    }
  }
  block_env_run(d, st, blockIdx.x, n_steps, step0, lx, ly, sd_mode != 0, g, md, cnt, wave_sums,
                lsq, &pt, par, LangevinEnvPath{{}, lv});
  if (!sd_mode) {  // (block_env_run's last barrier follows the last step)
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      st.vel[base + i] = vt[i];
      st.vel[M + base + i] = vt[N + i];
      st.vel[2 * M + base + i] = 0.0f;
      st.omega[base + i] = vt[2 * N + i];
    }
  }
  save_forces_env(st, blockIdx.x, sd_mode ? par : par ^ 1);
  if (!sd_mode) advance_counter(step_ctr, arrive, step0, n_steps);
}

}  // namespace swarm
