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
// per env, modelled on block_global_run_lds / k_rod_run: state and the
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

// Dynamic LDS of k_ellipsoid_run in 4-byte words: wave sums, cell counts,
// (8-byte aligned) the sorted positions and directors (uint2, float2), the
// sorted ids and the particle state (q, img, ang).
__host__ __device__ inline size_t ell_lds_words(int n, int ncell) {
  return 16 + (size_t)ncell + 1 + 1 + 10 * (size_t)n;
}

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

// All sub-steps (or steepest-descent steps) of env e by one workgroup.
template <bool kGB>
__device__ __forceinline__ void block_ellipsoid_run(
    const Derived* __restrict__ d, const DevState& st, const EllArgs* __restrict__ ea, int e,
    int n_steps, uint64_t step0, int lx, int ly, bool sd_mode, float g, float md, int32_t* cnt,
    int32_t* wave_sums, int32_t* lsq, const PairTables* pt, const EllPairTables* gt, int rp) {
  const PrevSlot prv = prev_slot(st, rp);  // reuse_forces: sub-step 0 reads slot rp
  const int T = blockDim.x, tid = threadIdx.x, N = st.n;
  const size_t M = (size_t)st.m, base = (size_t)e * N;
  const int ncell = 1 << (lx + ly);
  const int ncx = 1 << lx, ncy = 1 << ly;
  const int loy = ncy >= 3 ? -1 : 0, hiy = ncy >= 3 ? 1 : ncy - 1;
  const uint32_t k0 = d->key0, k1 = d->key1 ^ (uint32_t)e;
  const float sx0 = d->sx[0], sx1 = d->sx[1];
  const float eps24 = d->eps24;
  uint2* sq = reinterpret_cast<uint2*>(lsq + ((reinterpret_cast<uintptr_t>(lsq) >> 2) & 1));
  float2* sdir = reinterpret_cast<float2*>(sq + N);
  int32_t* sid = reinterpret_cast<int32_t*>(sdir + N);
  uint32_t* lqx = reinterpret_cast<uint32_t*>(sid + N);
  uint32_t* lqy = lqx + N;
  int32_t* lix = reinterpret_cast<int32_t*>(lqy + N);
  int32_t* liy = lix + N;
  uint32_t* lan = reinterpret_cast<uint32_t*>(liy + N);
  for (int i = tid; i < N; i += T) {
    const size_t gi = base + i;
    lqx[i] = st.q[gi];
    lqy[i] = st.q[M + gi];
    lix[i] = st.img[gi];
    liy[i] = st.img[M + gi];
    lan[i] = st.ang[gi];
  }
  __syncthreads();
  for (int s = 0; s < n_steps; ++s) {
    for (int c = tid; c <= ncell; c += T) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += T) atomicAdd(&cnt[cell_index(lqx[i], lqy[i], lx, ly)], 1);
    __syncthreads();
    block_exclusive_scan(cnt, ncell, wave_sums);
    __syncthreads();
    for (int i = tid; i < N; i += T) {
      const uint32_t qx = lqx[i], qy = lqy[i];
      const int pos = atomicAdd(&cnt[cell_index(qx, qy, lx, ly)], 1);
      float sn, cs;
      sincos_turn(lan[i], &sn, &cs);  // the sub-step's directors, once per particle
      sq[pos] = make_uint2(qx, qy);
      sdir[pos] = make_float2(cs, sn);
      sid[pos] = i | ((int)st.species[i] << 24);
    }
    __syncthreads();  // cell c now spans [c ? cnt[c-1] : 0, cnt[c])
    const bool last = s == n_steps - 1;
    int any = 0;
    for (int ps = tid; ps < N; ps += T) {
      const int pki = sid[ps];
      const int i = pki & 0xffffff, sik = pki >> 24;
      const size_t gi = base + i;
      PState pp = {lqx[i], lqy[i], lan[i], lix[i], liy[i]};
      const float2 ui = sdir[ps];
      int64_t ax = 0, ay = 0, at = 0;
      int deep = 0;
      const int c0 = cell_index(pp.qx, pp.qy, lx, ly);
      const int cx = c0 & (ncx - 1), cy = c0 >> lx;
      const int xa = ncx >= 3 ? max(cx - 1, 0) : 0;
      const int xb = ncx >= 3 ? min(cx + 1, ncx - 1) : ncx - 1;
      const int xw = ncx >= 3 ? (cx == 0 ? ncx - 1 : (cx == ncx - 1 ? 0 : -1)) : -1;
      for (int oy = loy; oy <= hiy; ++oy) {
        const int row = ((cy + oy + ncy) & (ncy - 1)) << lx;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
          if (part == 1 && xw < 0) continue;
          const int c_lo = row | (part == 0 ? xa : xw), c_hi = row | (part == 0 ? xb : xw);
          const int jb = c_lo ? cnt[c_lo - 1] : 0, je = cnt[c_hi];
          for (int jj = jb; jj < je; ++jj) {
            if (jj == ps) continue;
            const uint2 qj = sq[jj];
            const float rx = (float)(int32_t)(qj.x - pp.qx) * sx0;
            const float ry = (float)(int32_t)(qj.y - pp.qy) * sx1;
            const int pk = sik * kMaxSpecies + (sid[jj] >> 24);
            if (kGB) {
              const float r2 = __builtin_fmaf(rx, rx, ry * ry);
              if (!(r2 < gt->rcut2[pk] && r2 > 0.0f)) continue;
              const float2 uj = sdir[jj];
              deep += gb_pair(ea, gt->sig0[pk], gt->isig0[pk], gt->rcut[pk], r2, rx, ry, ui.x,
                              ui.y, uj.x, uj.y, ax, ay, at)
                          ? 1
                          : 0;
            } else {
              pair_force(pt->cut2[pk], pt->sig6[pk], eps24, rx, ry, ax, ay);
            }
          }
        }
      }
      // (counted in the sub-steps only: an overlapping start is what the
      // overlap removal is for)
      if (kGB && deep && !sd_mode) atomicAdd(st.wall_viol, (unsigned long long)deep);
      const bool first = st.reuse && s == 0 && !sd_mode;  // reuse_forces: previous run's
      const float fs = first ? prv.f[gi] : st.f_swim[gi];
      const float tz = first ? prv.tz[gi] : st.torque_z[gi];
      const float fex = st.f_ext[gi], fey = st.f_ext[M + gi];
      const PConst pc = load_pconst(d, sik);
      if (sd_mode) {
        const float tq = __builtin_fmaf(i64_to_f32(at), 5.9604644775390625e-08f, tz);
        any |= sd_step(pc, pp, ax, ay, fs, tq, fex, fey, g, md) ? 1 : 0;
      } else {
        float vx, vy, w;
        ell_step(ea, sik, pc, pp, ax, ay, at, fs, tz, fex, fey, k0, k1, (uint32_t)i,
                 step0 + (uint64_t)s, last, &vx, &vy, &w, first ? prv.ang[gi] : pp.an, !first,
                 ui.y, ui.x);
        if (last) {
          st.vel[gi] = vx;
          st.vel[M + gi] = vy;
          st.vel[2 * M + gi] = 0.0f;
          st.omega[gi] = w;
        }
      }
      lqx[i] = pp.qx;  // the sort of the next sub-step reads them after a barrier
      lqy[i] = pp.qy;
      lix[i] = pp.ix;
      liy[i] = pp.iy;
      lan[i] = pp.an;
    }
    if (sd_mode) {
      if (!__syncthreads_or(any)) break;
    } else {
      __syncthreads();
    }
  }
  __syncthreads();
  for (int i = tid; i < N; i += T) {
    const size_t gi = base + i;
    st.q[gi] = lqx[i];
    st.q[M + gi] = lqy[i];
    st.img[gi] = lix[i];
    st.img[M + gi] = liy[i];
    st.ang[gi] = lan[i];
  }
}

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
  block_ellipsoid_run<kGB>(d, st, ea, blockIdx.x, n_steps, step0, lx, ly, sd_mode != 0, g, md,
                           cnt, wave_sums, cnt + (1 << (lx + ly)) + 1, &pt, &gt, par);
  save_forces_env(st, blockIdx.x, sd_mode ? par : par ^ 1);
  if (!sd_mode) advance_counter(step_ctr, arrive, step0, n_steps);
}

}  // namespace swarm
