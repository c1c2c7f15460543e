// swarm_ellipsoid.cuh -- ellipsoidal colloids (2-D, periodic box): Gay-Berne
// pairs and anisotropic friction.
//
// Replaces what EspressoMD does for aspect_ratio != 1 and three-component
// frictions: _setup_interactions' switch of every pair from WCA to Gay-Berne
// (swarmrl/engine/espresso.py:802-832) and the per-axis gamma / gamma_rot of
// add_colloid_on_point (espresso.py:420-436).  The 2-D body frame is the
// reference's (espresso.py:427-449): body z the director, body y the in-plane
// normal, body x lab z, so gamma_par = gamma_translation[2], gamma_perp =
// gamma_translation[1], and the rotation about lab z keeps gamma_rotation[0]
// (Derived::rot_dt).
//
// A torque per pair and a step in the body frame: neither fits the cluster
// windows, so an engine with ellipsoids (swarm_engine_set_ellipsoids) runs
// every sub-step and the overlap removal on k_ellipsoid_run, one workgroup
// per env, a path of block_env_run (swarm_env_block.cuh): state and the
// per-sub-step counting sort in LDS, every particle walks the 3 x 3 cells,
// forces and the z-torque summed in int64 at 2^-24 (independent of visiting
// order).  kGB = false (aspect ratio 1, per-axis friction): pair_force (WCA)
// unchanged and only the new step.
//
// The pair term and the step are each ONE fp32 operation sequence (DESIGN.md
// §3, "Gay-Berne pair" and "Body-frame step"); tests/csrc/ellipsoid_oracle.c
// restates both line by line.
#pragma once

#include "swarm_integrator.cuh"

namespace swarm {

// Per-engine constants of the ellipsoid path (device memory; the pair tables
// are staged in LDS).  Host: swarm_engine_set_ellipsoids.
struct EllArgs {
  float chi, hchi, chi2;  // (k^2 - 1) / (k^2 + 1), chi / 2, chi^2
  float eps4;             // 4 epsilon0
  // body-frame mobilities per species: dt / gamma, sqrt(2 kT dt / gamma)
  // (0 without noise) and 1 / gamma, along (par) and across (perp) the director
  float mob_par[kMaxSpecies], mob_perp[kMaxSpecies];
  float sig_par[kMaxSpecies], sig_perp[kMaxSpecies];
  float inv_gpar[kMaxSpecies], inv_gperp[kMaxSpecies];
  // per species pair: sigma0 = (r_i + r_j) 2^(-1/6), 1 / sigma0, the cutoff
  // 2 (r_i + r_j) max(k, 1 / k) and its square
  float sig0[kMaxSpecies * kMaxSpecies], isig0[kMaxSpecies * kMaxSpecies];
  float rcut[kMaxSpecies * kMaxSpecies], rcut2[kMaxSpecies * kMaxSpecies];
};

struct EllPairTables {
  float sig0[kMaxSpecies * kMaxSpecies], isig0[kMaxSpecies * kMaxSpecies];
  float rcut[kMaxSpecies * kMaxSpecies], rcut2[kMaxSpecies * kMaxSpecies];
};

// Static LDS of k_ellipsoid_run<true>: both pair tables and 256 bytes of the
// helpers' own (the build's resource report states the total, 6400).
constexpr size_t kEllStaticLds = sizeof(PairTables) + sizeof(EllPairTables) + 256;

// Gay-Berne force and z-torque on i from j (r = x_j - x_i, u_i = (ci, si),
// u_j = (cj, sj)) with k2 = 1, nu = 1, mu = 2, shifted at the cutoff, added in
// 2^-24 fixed point.  Returns true for a deep overlap (X >= 1.25 or
// |r| - sigma + sigma0 <= 0), which contributes the values at X = 1.25.
//   g  = 1 - (chi/2) [(a+b)^2 / (1 + chi c) + (a-b)^2 / (1 - chi c)]
//   sigma = sigma0 / sqrt(g),  eps = eps0 / sqrt(1 - chi^2 c^2)
//   X  = sigma0 / (|r| - sigma + sigma0),  Xc the same at r_cut
//   U  = 4 eps [X^12 - X^6 - Xc^12 + Xc^6]
// The caller has tested 0 < r2 < r_cut^2.  Sequence: DESIGN.md §3.
__device__ __forceinline__ bool gb_pair(const EllArgs* __restrict__ ea, float sig0, float isig0,
                                        float rcut, float r2, float rx, float ry, float ci,
                                        float si, float cj, float sj, int64_t& ax, int64_t& ay,
                                        int64_t& at) {
  const float chi = ea->chi, hchi = ea->hchi;
  const float r = sqrt_rn(r2);
  const float ir = 1.0f / r;
  const float hx = rx * ir, hy = ry * ir;
  const float a = __builtin_fmaf(hx, ci, hy * si);
  const float b = __builtin_fmaf(hx, cj, hy * sj);
  const float c = __builtin_fmaf(ci, cj, si * sj);
  const float P = a + b, M = a - b;
  const float xc = chi * c;
  const float Dp = 1.0f + xc, Dm = 1.0f - xc;
  const float p = P / Dp, m = M / Dm;
  const float t = __builtin_fmaf(P, p, M * m);
  const float g = __builtin_fmaf(-hchi, t, 1.0f);
  const float isg = 1.0f / sqrt_rn(g);
  const float sig = sig0 * isg;
  const float ise = 1.0f / sqrt_rn(Dp * Dm);
  const float e4 = ea->eps4 * ise;
  const float den = (r - sig) + sig0;
  const float denc = (rcut - sig) + sig0;
  float X = sig0 / den;
  const bool deep = !(den > 0.0f) || !(X < 1.25f);
  X = deep ? 1.25f : X;
  const float Xc = sig0 / denc;
  const float X3 = (X * X) * X, Xc3 = (Xc * Xc) * Xc;
  const float X6 = X3 * X3, Xc6 = Xc3 * Xc3;
  const float u6 = __builtin_fmaf(X6, X6, -X6), uc6 = __builtin_fmaf(Xc6, Xc6, -Xc6);
  const float U = e4 * (u6 - uc6);
  const float ei = e4 * isig0;
  // W = -dU/d|r| = (4 eps / sigma0) X^7 (12 X^6 - 6); Wc the same at r_cut
  const float w = (ei * (X6 * X)) * __builtin_fmaf(12.0f, X6, -6.0f);
  const float wc = (ei * (Xc6 * Xc)) * __builtin_fmaf(12.0f, Xc6, -6.0f);
  // dU/dg = -(W - Wc) sigma / (2 g)
  const float G = -((w - wc) * ((0.5f * sig) * (isg * isg)));
  const float pm = p + m, pd = p - m;
  const float Aa = G * (-chi * pm);  // dU/da
  const float Ab = G * (-chi * pd);  // dU/db
  // dU/dc = dU/dg (chi^2 / 2)(p^2 - m^2) + U chi^2 c / (1 - chi^2 c^2)
  const float Ac = __builtin_fmaf(G, (hchi * chi) * (pm * pd), U * ((ea->chi2 * c) * (ise * ise)));
  // F_i = dU/dr = -W rhat + [Aa (u_i - a rhat) + Ab (u_j - b rhat)] / |r|
  const float k = __builtin_fmaf(Aa, a, Ab * b);
  const float rad = __builtin_fmaf(-k, ir, -w);
  const float tx = __builtin_fmaf(Aa, ci, Ab * cj), ty = __builtin_fmaf(Aa, si, Ab * sj);
  const float fx = __builtin_fmaf(rad, hx, tx * ir), fy = __builtin_fmaf(rad, hy, ty * ir);
  // T_i = -(u_i x dU/du_i)_z,  dU/du_i = Aa rhat + Ac u_j
  const float cr1 = __builtin_fmaf(ci, hy, -(si * hx)), cr2 = __builtin_fmaf(ci, sj, -(si * cj));
  const float tq = -__builtin_fmaf(Aa, cr1, Ac * cr2);
  ax += fix_scaled(fx * 16777216.0f);
  ay += fix_scaled(fy * 16777216.0f);
  at += fix_scaled(tq * 16777216.0f);
  return deep;
}

// One Brownian sub-step in the body frame from the force sum (ax, ay) and the
// torque sum at (2^-24 units).  (sn, cs): the director at the start of the
// sub-step; an_swim as in bd_step.  Sequence: DESIGN.md §3.
__device__ __forceinline__ void ell_step(const EllArgs* __restrict__ ea, int sp, const PConst& c,
                                         PState& p, int64_t ax, int64_t ay, int64_t at, float fs,
                                         float tz, float fex, float fey, uint32_t k0, uint32_t k1,
                                         uint32_t id, uint64_t step, bool last, float* vx,
                                         float* vy, float* w, uint32_t an_swim, bool swim_own,
                                         float sn, float cs) {
  float ss = sn, sc = cs;
  if (!swim_own) sincos_turn(an_swim, &ss, &sc);
  float g[3] = {0.0f, 0.0f, 0.0f};
  if (c.noisy) step_normals(k0, k1, id, step, g);
  const float c1x = fex + fs * sc, c1y = fey + fs * ss;
  const float fx = __builtin_fmaf(i64_to_f32(ax), 5.9604644775390625e-08f, c1x);
  const float fy = __builtin_fmaf(i64_to_f32(ay), 5.9604644775390625e-08f, c1y);
  const float tq = __builtin_fmaf(i64_to_f32(at), 5.9604644775390625e-08f, tz);
  const float fpar = __builtin_fmaf(fx, cs, fy * sn);
  const float fperp = __builtin_fmaf(fy, cs, -(fx * sn));
  const float sgp = c.noisy ? ea->sig_par[sp] : 0.0f, sgq = c.noisy ? ea->sig_perp[sp] : 0.0f;
  const float dpar = __builtin_fmaf(fpar, ea->mob_par[sp], sgp * g[0]);
  const float dperp = __builtin_fmaf(fperp, ea->mob_perp[sp], sgq * g[1]);
  const float dx = __builtin_fmaf(cs, dpar, -(sn * dperp));
  const float dy = __builtin_fmaf(sn, dpar, cs * dperp);
  float dth = tq * c.rot_dt;
  dth = dth + c.sigr * g[2];
  advance(p.qx, p.ix, f2i32_sat(dx * c.inv_sx0));
  advance(p.qy, p.iy, f2i32_sat(dy * c.inv_sx1));
  p.an = p.an + (uint32_t)f2i32_sat(dth * kAngInvScale);
  if (last) {
    const float vpar = fpar * ea->inv_gpar[sp], vperp = fperp * ea->inv_gperp[sp];
    float v0 = __builtin_fmaf(cs, vpar, -(sn * vperp));
    float v1 = __builtin_fmaf(sn, vpar, cs * vperp);
    float om = tq * c.inv_gr;
    if (c.noisy) {
      float gv[3];
      normals3(k0, k1, id, step, 1u, gv);
      v0 = v0 + c.sig_v * gv[0];
      v1 = v1 + c.sig_v * gv[1];
      om = om + c.sig_w * gv[2];
    }
    *vx = v0;
    *vy = v1;
    *w = om;
  }
}

// block_env_run for ellipsoids: the directors travel with the sorted
// positions, the pair term is Gay-Berne's (kGB) with its torque, and the step
// is the body frame's.
template <bool kGB>
struct EllEnvPath : EnvPathBase {
  static constexpr bool kDirs = true;
  const EllArgs* __restrict__ ea;
  const EllPairTables* gt;
  __device__ __forceinline__ void pair(const EnvRun& r, int pk, float rx, float ry, float2 ui,
                                       const float2* uj, EnvAcc& a) const {
    if (kGB) {
      const float r2 = __builtin_fmaf(rx, rx, ry * ry);
      if (!(r2 < gt->rcut2[pk] && r2 > 0.0f)) return;
      a.deep += gb_pair(ea, gt->sig0[pk], gt->isig0[pk], gt->rcut[pk], r2, rx, ry, ui.x, ui.y,
                        uj->x, uj->y, a.ax, a.ay, a.at)
                    ? 1
                    : 0;
    } else {
      EnvPathBase::pair(r, pk, rx, ry, ui, uj, a);
    }
  }
  template <class L>
  __device__ __forceinline__ bool step(const EnvRun& r, const L&, int s, bool last,
                                       const EnvParticle& q, PState& p, float2 ui, EnvAcc& a,
                                       int& any) const {
    // (counted in the sub-steps only: an overlapping start is what the
    // overlap removal is for)
    if (kGB && a.deep && !r.sd_mode) atomicAdd(r.st.wall_viol, (unsigned long long)a.deep);
    const PConst pc = load_pconst(r.d, q.sik);
    if (r.sd_mode) {
      const float tq = __builtin_fmaf(i64_to_f32(a.at), 5.9604644775390625e-08f, q.tz);
      any |= sd_step(pc, p, a.ax, a.ay, q.fs, tq, q.fex, q.fey, r.g, r.md) ? 1 : 0;
    } else {
      float vx, vy, w;
      ell_step(ea, q.sik, pc, p, a.ax, a.ay, a.at, q.fs, q.tz, q.fex, q.fey, r.k0, r.k1,
               (uint32_t)q.i, r.step0 + (uint64_t)s, last, &vx, &vy, &w,
               q.first ? r.prv.ang[q.gi] : p.an, !q.first, ui.y, ui.x);
      if (last) env_store_vel(r, q.gi, vx, vy, w);
    }
    return true;
  }
};

// Ellipsoid-engine launch: n_steps sub-steps (or SD steps) of every env, one
// 1024-thread workgroup per env (k_global's contract: reuse_forces slots,
// device step counter).
template <bool kGB>
__global__ __launch_bounds__(1024) void k_ellipsoid_run(
    const Derived* __restrict__ d, DevState st, const EllArgs* __restrict__ ea, int n_steps,
    uint64_t* __restrict__ step_ctr, uint32_t* __restrict__ arrive, int lx, int ly, int sd_mode,
    float g, float md) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ PairTables pt;
  __shared__ EllPairTables gt;
  if (kGB) {
    for (int k = threadIdx.x; k < kMaxSpecies * kMaxSpecies; k += blockDim.x) {
      gt.sig0[k] = ea->sig0[k];
      gt.isig0[k] = ea->isig0[k];
      gt.rcut[k] = ea->rcut[k];
      gt.rcut2[k] = ea->rcut2[k];
    }
  }
  stage_pair_tables(d, &pt);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  const uint64_t step0 = sd_mode ? 0ull : *step_ctr;
  const int par = window_parity(step_ctr);
  block_env_run(d, st, blockIdx.x, n_steps, step0, lx, ly, sd_mode != 0, g, md, cnt, wave_sums,
                cnt + (1 << (lx + ly)) + 1, &pt, par, EllEnvPath<kGB>{{}, ea, &gt});
  save_forces_env(st, blockIdx.x, sd_mode ? par : par ^ 1);
  if (!sd_mode) advance_counter(step_ctr, arrive, step0, n_steps);
}

}  // namespace swarm
