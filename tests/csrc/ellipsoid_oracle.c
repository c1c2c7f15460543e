/*
 * ellipsoid_oracle.c -- CPU restatement of the ellipsoid path (swarmrl_amd/
 * csrc/swarm_ellipsoid.cuh), TEST INFRASTRUCTURE ONLY.
 *
 * One translation unit with the CPU oracle: its static helpers (derive,
 * wca_pair, pair_disp, advance, f2i32, f2i32_sat, fix_scaled) and exported
 * device-math restatements (or_sincos_turn, or_step_normals, or_normals3) are
 * used unchanged.  Pair search is O(n^2): the sums are exact int64, so the
 * GPU's cell lists give the same bits.  Compiled with -ffp-contract=off:
 * every fp32 operation below is rounded on its own, fused only where fmaf is
 * written ("Gay-Berne pair" and "Body-frame step").
 *
 * Sub-step (2-D, periodic):
 *   1. every particle sums over all partners within the pair's cutoff the
 *      Gay-Berne force and z-torque (aspect ratio != 1) or the WCA force
 *      (aspect ratio 1), in int64 at 2^-24;
 *   2. f = F 2^-24 + f_ext + f_swim d (d: the swim director, with
 *      reuse_forces at sub-step 0 the previous run's), split along and across
 *      the director at the start of the sub-step, each part with its own
 *      mobility and noise, rotated back and added per axis;
 *   3. dtheta = (t_action + T 2^-24) rot_dt + sig_r g2.
 */
#include "../../oracle/swarm_oracle.c"

typedef struct {
  float chi, hchi, chi2, eps4;
  float mob_par[SWARM_MAX_SPECIES], mob_perp[SWARM_MAX_SPECIES];
  float sig_par[SWARM_MAX_SPECIES], sig_perp[SWARM_MAX_SPECIES];
  float inv_gpar[SWARM_MAX_SPECIES], inv_gperp[SWARM_MAX_SPECIES];
  float sig0[SWARM_MAX_SPECIES][SWARM_MAX_SPECIES], isig0[SWARM_MAX_SPECIES][SWARM_MAX_SPECIES];
  float rcut[SWARM_MAX_SPECIES][SWARM_MAX_SPECIES], rcut2[SWARM_MAX_SPECIES][SWARM_MAX_SPECIES];
  int gb;
} ell_t;

/* swarm_engine_set_ellipsoids' derivation: fp64, rounded once */
static void ell_derive(const swarm_params_t *p, const swarm_ellipsoids_t *e, ell_t *a) {
  memset(a, 0, sizeof(*a));
  const double k = e->aspect_ratio;
  const double chi = (k * k - 1.0) / (k * k + 1.0);
  const double wide = 2.0 * (k > 1.0 / k ? k : 1.0 / k);
  a->gb = k != 1.0;
  a->chi = (float)chi;
  a->hchi = (float)(0.5 * chi);
  a->chi2 = (float)(chi * chi);
  a->eps4 = (float)(4.0 * p->wca_epsilon);
  const double kT = p->kT, dt = p->time_step;
  for (int s = 0; s < p->n_species; ++s) {
    const double ga = e->gamma_par[s], gq = e->gamma_perp[s];
    a->mob_par[s] = (float)(dt / ga);
    a->mob_perp[s] = (float)(dt / gq);
    a->sig_par[s] = (float)sqrt(2.0 * kT * dt / ga);
    a->sig_perp[s] = (float)sqrt(2.0 * kT * dt / gq);
    a->inv_gpar[s] = (float)(1.0 / ga);
    a->inv_gperp[s] = (float)(1.0 / gq);
    for (int t = 0; t < p->n_species; ++t) {
      const double rs = p->radius[s] + p->radius[t];
      const double s0 = rs * pow(2.0, -1.0 / 6.0), rc = wide * rs;
      a->sig0[s][t] = (float)s0;
      a->isig0[s][t] = s0 > 0.0 ? (float)(1.0 / s0) : 0.0f;
      a->rcut[s][t] = (float)rc;
      a->rcut2[s][t] = (float)(rc * rc);
    }
  }
}

/* gb_pair of swarm_ellipsoid.cuh: force (f[0], f[1]) and z-torque f[2] on i
 * before the fixed-point conversion; returns 1 for a deep overlap.  The
 * caller has tested 0 < r2 < rcut2. */
static int gb_pair(const ell_t *ea, float sig0, float isig0, float rcut, float r2, float rx,
                   float ry, float ci, float si, float cj, float sj, float f[3]) {
  const float chi = ea->chi, hchi = ea->hchi;
  const float r = sqrtf(r2);
  const float ir = 1.0f / r;
  const float hx = rx * ir, hy = ry * ir;
  const float a = fmaf(hx, ci, hy * si);
  const float b = fmaf(hx, cj, hy * sj);
  const float c = fmaf(ci, cj, si * sj);
  const float P = a + b, M = a - b;
  const float xc = chi * c;
  const float Dp = 1.0f + xc, Dm = 1.0f - xc;
  const float p = P / Dp, m = M / Dm;
  const float t = fmaf(P, p, M * m);
  const float g = fmaf(-hchi, t, 1.0f);
  const float isg = 1.0f / sqrtf(g);
  const float sig = sig0 * isg;
  const float ise = 1.0f / sqrtf(Dp * Dm);
  const float e4 = ea->eps4 * ise;
  const float den = (r - sig) + sig0;
  const float denc = (rcut - sig) + sig0;
  float X = sig0 / den;
  const int deep = !(den > 0.0f) || !(X < 1.25f);
  X = deep ? 1.25f : X;
  const float Xc = sig0 / denc;
  const float X3 = (X * X) * X, Xc3 = (Xc * Xc) * Xc;
  const float X6 = X3 * X3, Xc6 = Xc3 * Xc3;
  const float u6 = fmaf(X6, X6, -X6), uc6 = fmaf(Xc6, Xc6, -Xc6);
  const float U = e4 * (u6 - uc6);
  const float ei = e4 * isig0;
  const float w = (ei * (X6 * X)) * fmaf(12.0f, X6, -6.0f);
  const float wc = (ei * (Xc6 * Xc)) * fmaf(12.0f, Xc6, -6.0f);
  const float G = -((w - wc) * ((0.5f * sig) * (isg * isg)));
  const float pm = p + m, pd = p - m;
  const float Aa = G * (-chi * pm);
  const float Ab = G * (-chi * pd);
  const float Ac = fmaf(G, (hchi * chi) * (pm * pd), U * ((ea->chi2 * c) * (ise * ise)));
  const float k = fmaf(Aa, a, Ab * b);
  const float rad = fmaf(-k, ir, -w);
  const float tx = fmaf(Aa, ci, Ab * cj), ty = fmaf(Aa, si, Ab * sj);
  f[0] = fmaf(rad, hx, tx * ir);
  f[1] = fmaf(rad, hy, ty * ir);
  const float cr1 = fmaf(ci, hy, -(si * hx)), cr2 = fmaf(ci, sj, -(si * cj));
  f[2] = -fmaf(Aa, cr1, Ac * cr2);
  return deep;
}

/* The fp32 pair term for given geometry (species 0, 0): out[3] = F_x, F_y,
 * T_z on i, *deep the overlap flag; returns 0 out of range. */
int or_ell_pair(const swarm_params_t *p, const swarm_ellipsoids_t *e, float rx, float ry,
                float ci, float si, float cj, float sj, float *out, int *deep) {
  ell_t a;
  ell_derive(p, e, &a);
  out[0] = out[1] = out[2] = 0.0f;
  *deep = 0;
  const float r2 = fmaf(rx, rx, ry * ry);
  if (!(r2 < a.rcut2[0][0] && r2 > 0.0f))
    return 0;
  *deep = gb_pair(&a, a.sig0[0][0], a.isig0[0][0], a.rcut[0][0], r2, rx, ry, ci, si, cj, sj,
                  out);
  return 1;
}

/* forces and torques of one (sub-)step: acc[3][n] (x, y, torque), 2^-24;
 * stats (NULL allowed): [0] += ordered pairs in range, [1] += those with a
 * non-zero torque, [2] += deep overlaps */
static void ell_forces(const swarm_params_t *p, const derived_t *d, const ell_t *ea, int n,
                       const uint32_t *q, const int32_t *img, const uint32_t *ang,
                       const uint8_t *species, int64_t *acc, int64_t *stats, int count_deep) {
  memset(acc, 0, sizeof(int64_t) * 3 * (size_t)n);
  float *cs = (float *)malloc(sizeof(float) * 2 * (size_t)n), *sn = cs + n;
  for (int i = 0; i < n; ++i)
    or_sincos_turn(ang[i], &sn[i], &cs[i]);
  int64_t s0 = 0, s1 = 0, s2 = 0;
#ifdef _OPENMP
#pragma omp parallel for schedule(static) reduction(+ : s0, s1, s2) if (n >= 256)
#endif
  for (int i = 0; i < n; ++i) {
    const int si = species[i];
    for (int j = 0; j < n; ++j) {
      if (j == i)
        continue;
      const int sj = species[j];
      const float rx = pair_disp(p, d, q, img, n, 0, i, j);
      const float ry = pair_disp(p, d, q, img, n, 1, i, j);
      const float r2 = fmaf(rx, rx, ry * ry);
      if (!ea->gb) {
        wca_pair(d, si, sj, rx, ry, &acc[i], &acc[n + i]);
        s0 += r2 < d->cut2[si][sj] && r2 > 0.0f;
        continue;
      }
      if (!(r2 < ea->rcut2[si][sj] && r2 > 0.0f))
        continue;
      float f[3];
      const int deep = gb_pair(ea, ea->sig0[si][sj], ea->isig0[si][sj], ea->rcut[si][sj], r2, rx,
                               ry, cs[i], sn[i], cs[j], sn[j], f);
      const int64_t tq = fix_scaled(f[2] * 16777216.0f);
      acc[i] += fix_scaled(f[0] * 16777216.0f);
      acc[n + i] += fix_scaled(f[1] * 16777216.0f);
      acc[2 * n + i] += tq;
      s0 += 1;
      s1 += tq != 0;
      s2 += count_deep && deep;
    }
  }
  if (stats) {
    stats[0] += s0;
    stats[1] += s1;
    stats[2] += s2;
  }
  free(cs);
}

/*
 * n_steps BD sub-steps of ONE env of ellipsoids.  Arrays as or_bd_run_walls;
 * f_swim0 / torque0 / ang0: reuse_forces (NULL: the current ones).  stats
 * (NULL allowed): see ell_forces, summed over the sub-steps.
 */
int or_ell_bd_run(const swarm_params_t *p, const swarm_ellipsoids_t *e, int n, uint32_t *q,
                  int32_t *img, uint32_t *ang, const uint8_t *species, const float *f_swim,
                  const float *torque_z, const float *f_ext, uint64_t step0, int n_steps,
                  uint32_t env, float *vel, float *omega, const float *f_swim0,
                  const float *torque0, const uint32_t *ang0, int64_t *stats) {
  if (p->n_dims != 2 || !p->periodic)
    return SWARM_EINVAL;
  derived_t d;
  derive(p, &d);
  ell_t ea;
  ell_derive(p, e, &ea);
  const int noisy = p->kT > 0.0;
  int64_t *acc = (int64_t *)malloc(sizeof(int64_t) * 3 * (size_t)n);
  for (int s = 0; s < n_steps; ++s) {
    const uint64_t step = step0 + (uint64_t)s;
    const int last = s == n_steps - 1, first = s == 0;
    ell_forces(p, &d, &ea, n, q, img, ang, species, acc, stats, 1);
    for (int i = 0; i < n; ++i) {
      const int sp = species[i];
      const float fs = first && f_swim0 ? f_swim0[i] : f_swim[i];
      const float tz = first && torque0 ? torque0[i] : torque_z[i];
      const float fex = f_ext ? f_ext[i] : 0.0f, fey = f_ext ? f_ext[n + i] : 0.0f;
      float sn, cs, ss, sc;
      or_sincos_turn(ang[i], &sn, &cs);
      or_sincos_turn(first && ang0 ? ang0[i] : ang[i], &ss, &sc);
      float g[3] = {0.0f, 0.0f, 0.0f};
      if (noisy)
        or_step_normals(p->seed, env, (uint32_t)i, step, g);
      const float c1x = fex + fs * sc, c1y = fey + fs * ss;
      const float fx = fmaf((float)acc[i], 5.9604644775390625e-08f, c1x);
      const float fy = fmaf((float)acc[n + i], 5.9604644775390625e-08f, c1y);
      const float tq = fmaf((float)acc[2 * n + i], 5.9604644775390625e-08f, tz);
      const float fpar = fmaf(fx, cs, fy * sn);
      const float fperp = fmaf(fy, cs, -(fx * sn));
      const float sgp = noisy ? ea.sig_par[sp] : 0.0f, sgq = noisy ? ea.sig_perp[sp] : 0.0f;
      const float dpar = fmaf(fpar, ea.mob_par[sp], sgp * g[0]);
      const float dperp = fmaf(fperp, ea.mob_perp[sp], sgq * g[1]);
      const float dx = fmaf(cs, dpar, -(sn * dperp));
      const float dy = fmaf(sn, dpar, cs * dperp);
      float dth = tq * d.rot_dt[sp];
      dth = dth + (noisy ? d.sig_r[sp] : 0.0f) * g[2];
      advance(&q[i], &img[i], f2i32_sat(dx * d.inv_sx[0]));
      advance(&q[n + i], &img[n + i], f2i32_sat(dy * d.inv_sx[1]));
      ang[i] = ang[i] + (uint32_t)f2i32_sat(dth * ANG_INV_SCALE);
      if (last) {
        const float vpar = fpar * ea.inv_gpar[sp], vperp = fperp * ea.inv_gperp[sp];
        float vx = fmaf(cs, vpar, -(sn * vperp));
        float vy = fmaf(sn, vpar, cs * vperp);
        float w = tq * d.inv_gr[sp];
        if (noisy) {
          float gv[3];
          or_normals3(p->seed, env, (uint32_t)i, step, 1u, gv);
          vx = vx + d.sig_v[sp] * gv[0];
          vy = vy + d.sig_v[sp] * gv[1];
          w = w + d.sig_w[sp] * gv[2];
        }
        if (vel) {
          vel[i] = vx;
          vel[n + i] = vy;
          vel[2 * n + i] = 0.0f;
        }
        if (omega)
          omega[i] = w;
      }
    }
  }
  free(acc);
  return SWARM_OK;
}

/* Steepest descent (or_sd_run_walls' step) with the Gay-Berne force and
 * torque.  Returns the number of steps executed (stops once no particle
 * feels a force or torque). */
int or_ell_sd_run(const swarm_params_t *p, const swarm_ellipsoids_t *e, int n, uint32_t *q,
                  int32_t *img, uint32_t *ang, const uint8_t *species, const float *f_swim,
                  const float *torque_z, const float *f_ext, int n_steps, double gamma,
                  double max_disp) {
  derived_t d;
  derive(p, &d);
  ell_t ea;
  ell_derive(p, e, &ea);
  const float g = (float)gamma, md = (float)max_disp;
  int64_t *acc = (int64_t *)malloc(sizeof(int64_t) * 3 * (size_t)n);
  int s;
  for (s = 0; s < n_steps; ++s) {
    ell_forces(p, &d, &ea, n, q, img, ang, species, acc, NULL, 0);
    int any = 0;
    for (int i = 0; i < n; ++i) {
      float sn, cs;
      or_sincos_turn(ang[i], &sn, &cs);
      float fx = (float)acc[i] * 5.9604644775390625e-08f;
      float fy = (float)acc[n + i] * 5.9604644775390625e-08f;
      fx = fx + (f_ext ? f_ext[i] : 0.0f);
      fy = fy + (f_ext ? f_ext[n + i] : 0.0f);
      fx = fx + f_swim[i] * cs;
      fy = fy + f_swim[i] * sn;
      const float tz = fmaf((float)acc[2 * n + i], 5.9604644775390625e-08f, torque_z[i]);
      if (fx != 0.0f || fy != 0.0f || tz != 0.0f)
        any = 1;
      float px = fminf(fmaxf(g * fx, -md), md);
      float py = fminf(fmaxf(g * fy, -md), md);
      float pa = fminf(fmaxf(g * tz, -md), md);
      advance(&q[i], &img[i], f2i32(px * d.inv_sx[0]));
      advance(&q[n + i], &img[n + i], f2i32(py * d.inv_sx[1]));
      ang[i] = ang[i] + (uint32_t)f2i32(pa * ANG_INV_SCALE);
    }
    if (!any)
      break;
  }
  free(acc);
  return s;
}
