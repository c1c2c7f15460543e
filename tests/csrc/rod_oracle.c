/*
 * rod_oracle.c -- CPU restatement of the rod path (swarmrl_amd/csrc/
 * swarm_rod.cuh), TEST INFRASTRUCTURE ONLY.
 *
 * One translation unit with the CPU oracle: its static helpers (derive,
 * wca_pair, pair_disp, advance, f2i32, f2i32_sat) and exported device-math
 * restatements (or_sincos_turn, or_step_normals, or_normals3) are used
 * unchanged, so the colloids' sub-step is or_bd_run_walls' sequence line by
 * line.  Pair search is O(n^2): the sums are exact int64, so the GPU's cell
 * lists give the same bits.
 *
 * Sub-step (2-D, periodic, one rod = particles [first, first + n)):
 *   1. forces: a colloid sums WCA over every partner; a rod particle over
 *      the colloids only (rod-rod pairs skipped);
 *   2. F = sum_b A_b, S = sum_b m_b A_b (int64, 2^-24 units; m_b the signed
 *      slot, centre 0);
 *   3. tau = (delta (u_x S_y - u_y S_x)) 2^-24 in fp32, u = sincos_turn of
 *      the centre's angle at the start of the sub-step;
 *   4. colloids: the BD sub-step of or_bd_run_walls (reuse_forces at 0);
 *   5. centre: the same sub-step from (F, swim 0, ext 0, tau), noise stream
 *      of its particle index; fixed: q/img restored, v = 0;
 *   6. beads: from the centre's new state, per axis
 *      dq = f2i32_sat(((m delta) cos|sin) inv_sx), ang = centre's; on the last
 *      sub-step v_b = v_c + omega x r_b, omega_b = omega_c.
 */
#include "../../oracle/swarm_oracle.c"

static int rod_slot(int b) {
  if (b == 0)
    return 0;
  int k = b - 1;
  return (k & 1 ? -1 : 1) * (k / 2 + 1);
}

static void rod_place(const swarm_rod_t *rod, const derived_t *d, int n, uint32_t *q,
                      int32_t *img, uint32_t *ang, int b, float *rx, float *ry) {
  const int c = rod->first, i = rod->first + b;
  const float delta = (float)rod->delta;
  float sn, cs;
  or_sincos_turn(ang[c], &sn, &cs);
  const float lever = (float)rod_slot(b) * delta;
  *rx = lever * cs;
  *ry = lever * sn;
  q[i] = q[c];
  img[i] = img[c];
  q[n + i] = q[n + c];
  img[n + i] = img[n + c];
  advance(&q[i], &img[i], f2i32_sat(*rx * d->inv_sx[0]));
  advance(&q[n + i], &img[n + i], f2i32_sat(*ry * d->inv_sx[1]));
  ang[i] = ang[c];
}

/* The beads onto the centre's line (the engine does this once, when the rod
 * is set). */
int or_rod_snap(const swarm_params_t *p, int n, uint32_t *q, int32_t *img, uint32_t *ang,
                const swarm_rod_t *rod) {
  derived_t d;
  derive(p, &d);
  float rx, ry;
  for (int b = 1; b < rod->n; ++b)
    rod_place(rod, &d, n, q, img, ang, b, &rx, &ry);
  return SWARM_OK;
}

/* forces of one (sub-)step; sigma (NULL allowed): sum of the rod's forces on
 * the colloids; contacts (NULL allowed): += colloid-rod pairs in range */
static void rod_forces(const swarm_params_t *p, const derived_t *d, int n, const uint32_t *q,
                       const int32_t *img, const uint8_t *species, const swarm_rod_t *rod,
                       int64_t *acc, int64_t *sigma, int64_t *contacts) {
  const int r0 = rod->first, r1 = rod->first + rod->n;
  memset(acc, 0, sizeof(int64_t) * 2 * (size_t)n);
  if (sigma)
    sigma[0] = sigma[1] = 0;
  for (int i = 0; i < n; ++i) {
    const int i_rod = i >= r0 && i < r1;
    for (int j = 0; j < n; ++j) {
      if (j == i)
        continue;
      const int j_rod = j >= r0 && j < r1;
      if (i_rod && j_rod)
        continue;
      float rx = pair_disp(p, d, q, img, n, 0, i, j);
      float ry = pair_disp(p, d, q, img, n, 1, i, j);
      int64_t tx = 0, ty = 0;
      wca_pair(d, species[i], species[j], rx, ry, &tx, &ty);
      acc[i] += tx;
      acc[n + i] += ty;
      if (!i_rod && j_rod) {
        float r2 = fmaf(rx, rx, ry * ry);
        if (r2 < d->cut2[species[i]][species[j]] && r2 > 0.0f && contacts)
          ++*contacts;
        if (sigma) {
          sigma[0] += tx;
          sigma[1] += ty;
        }
      }
    }
  }
}

/* One BD sub-step of particle i from its force sum (or_bd_run_walls' body). */
static void bd_particle(const swarm_params_t *p, const derived_t *d, int n, uint32_t *q,
                        int32_t *img, uint32_t *ang, int i, int sp, int64_t ax, int64_t ay,
                        float fs, float tz, float fex, float fey, uint32_t an_swim,
                        uint64_t step, uint32_t env, int last, float *vx_o, float *vy_o,
                        float *w_o) {
  const int noisy = p->kT > 0.0;
  float sn, cs;
  or_sincos_turn(an_swim, &sn, &cs);
  float g[3] = {0.0f, 0.0f, 0.0f};
  float dth = tz * d->rot_dt[sp];
  if (noisy) {
    or_step_normals(p->seed, env, (uint32_t)i, step, g);
    dth = dth + d->sig_r[sp] * g[2];
  }
  const float c1x = fex + fs * cs;
  const float c1y = fey + fs * sn;
  float fx = fmaf((float)ax, 5.9604644775390625e-08f, c1x);
  float fy = fmaf((float)ay, 5.9604644775390625e-08f, c1y);
  const float mobx = d->mob_dt[sp] * d->inv_sx[0], moby = d->mob_dt[sp] * d->inv_sx[1];
  const float sigx = noisy ? d->sig_t[sp] * d->inv_sx[0] : 0.0f;
  const float sigy = noisy ? d->sig_t[sp] * d->inv_sx[1] : 0.0f;
  advance(&q[i], &img[i], f2i32_sat(fmaf(fx, mobx, sigx * g[0])));
  advance(&q[n + i], &img[n + i], f2i32_sat(fmaf(fy, moby, sigy * g[1])));
  ang[i] = ang[i] + (uint32_t)f2i32_sat(dth * ANG_INV_SCALE);
  if (last) {
    float vx = fx * d->inv_gt[sp], vy = fy * d->inv_gt[sp];
    float w = tz * d->inv_gr[sp];
    if (noisy) {
      float gv[3];
      or_normals3(p->seed, env, (uint32_t)i, step, 1u, gv);
      vx = vx + d->sig_v[sp] * gv[0];
      vy = vy + d->sig_v[sp] * gv[1];
      w = w + d->sig_w[sp] * gv[2];
    }
    *vx_o = vx;
    *vy_o = vy;
    *w_o = w;
  }
}

/*
 * n_steps BD sub-steps of ONE env with a rod.  Arrays as or_bd_run_walls;
 * f_swim0 / torque0 / ang0: reuse_forces (NULL: the current ones).
 * Optional outputs (NULL allowed): sums[4] = F_x, F_y, S_x, S_y and *tau of
 * the LAST sub-step, sigma[2] = the last sub-step's sum of the rod's forces
 * on the colloids, *contacts += colloid-rod pairs in range over all
 * sub-steps.
 */
int or_rod_bd_run(const swarm_params_t *p, int n, uint32_t *q, int32_t *img, uint32_t *ang,
                  const uint8_t *species, const float *f_swim, const float *torque_z,
                  const float *f_ext, uint64_t step0, int n_steps, uint32_t env, float *vel,
                  float *omega, const swarm_rod_t *rod, const float *f_swim0,
                  const float *torque0, const uint32_t *ang0, int64_t *sums, float *tau_out,
                  int64_t *sigma, int64_t *contacts) {
  if (p->n_dims != 2 || !p->periodic || rod->n < 1 || rod->first < 0 || rod->first + rod->n > n)
    return SWARM_EINVAL;
  derived_t d;
  derive(p, &d);
  const int r0 = rod->first, r1 = rod->first + rod->n;
  const float delta = (float)rod->delta;
  int64_t *acc = (int64_t *)malloc(sizeof(int64_t) * 2 * (size_t)n);
  for (int s = 0; s < n_steps; ++s) {
    const uint64_t step = step0 + (uint64_t)s;
    const int last = s == n_steps - 1;
    rod_forces(p, &d, n, q, img, species, rod, acc, sigma, contacts);
    int64_t F[2] = {0, 0}, S[2] = {0, 0};
    for (int b = 0; b < rod->n; ++b) {
      const int64_t m = rod_slot(b);
      F[0] += acc[r0 + b];
      F[1] += acc[n + r0 + b];
      S[0] += m * acc[r0 + b];
      S[1] += m * acc[n + r0 + b];
    }
    float sn, cs;
    or_sincos_turn(ang[r0], &sn, &cs);
    const float t1 = cs * (float)S[1], t2 = sn * (float)S[0];
    const float cr = t1 - t2;
    const float tau = (delta * cr) * 5.9604644775390625e-08f;
    if (sums) {
      sums[0] = F[0];
      sums[1] = F[1];
      sums[2] = S[0];
      sums[3] = S[1];
    }
    if (tau_out)
      *tau_out = tau;
    float vx = 0.0f, vy = 0.0f, w = 0.0f;
    for (int i = 0; i < n; ++i) {
      if (i >= r0 && i < r1)
        continue;
      const int first = s == 0;
      const float fs = first && f_swim0 ? f_swim0[i] : f_swim[i];
      const float tz = first && torque0 ? torque0[i] : torque_z[i];
      bd_particle(p, &d, n, q, img, ang, i, species[i], acc[i], acc[n + i], fs, tz,
                  f_ext ? f_ext[i] : 0.0f, f_ext ? f_ext[n + i] : 0.0f,
                  first && ang0 ? ang0[i] : ang[i], step, env, last, &vx, &vy, &w);
      if (last && vel) {
        vel[i] = vx;
        vel[n + i] = vy;
        vel[2 * n + i] = 0.0f;
      }
      if (last && omega)
        omega[i] = w;
    }
    /* the centre */
    const uint32_t oq[2] = {q[r0], q[n + r0]};
    const int32_t oi[2] = {img[r0], img[n + r0]};
    vx = vy = w = 0.0f;
    bd_particle(p, &d, n, q, img, ang, r0, species[r0], F[0], F[1], 0.0f, tau, 0.0f, 0.0f,
                ang[r0], step, env, last, &vx, &vy, &w);
    if (rod->fixed) {
      q[r0] = oq[0];
      q[n + r0] = oq[1];
      img[r0] = oi[0];
      img[n + r0] = oi[1];
      vx = 0.0f;
      vy = 0.0f;
    }
    if (last && vel) {
      vel[r0] = vx;
      vel[n + r0] = vy;
      vel[2 * n + r0] = 0.0f;
    }
    if (last && omega)
      omega[r0] = w;
    /* the beads */
    for (int b = 1; b < rod->n; ++b) {
      float rx, ry;
      rod_place(rod, &d, n, q, img, ang, b, &rx, &ry);
      if (last && vel) {
        vel[r0 + b] = vx - w * ry;
        vel[n + r0 + b] = vy + w * rx;
        vel[2 * n + r0 + b] = 0.0f;
      }
      if (last && omega)
        omega[r0 + b] = w;
    }
  }
  free(acc);
  return SWARM_OK;
}

/* Steepest descent with a rod: or_sd_run_walls' step for the colloids (the
 * rod's particles push them), the rod itself does not move.  Returns the
 * number of steps executed (stops once no colloid feels a force). */
int or_rod_sd_run(const swarm_params_t *p, int n, uint32_t *q, int32_t *img, uint32_t *ang,
                  const uint8_t *species, const float *f_swim, const float *torque_z,
                  const float *f_ext, int n_steps, double gamma, double max_disp,
                  const swarm_rod_t *rod) {
  derived_t d;
  derive(p, &d);
  const int r0 = rod->first, r1 = rod->first + rod->n;
  const float g = (float)gamma, md = (float)max_disp;
  int64_t *acc = (int64_t *)malloc(sizeof(int64_t) * 2 * (size_t)n);
  int s;
  for (s = 0; s < n_steps; ++s) {
    rod_forces(p, &d, n, q, img, species, rod, acc, NULL, NULL);
    int any = 0;
    for (int i = 0; i < n; ++i) {
      if (i >= r0 && i < r1)
        continue;
      float sn, cs;
      or_sincos_turn(ang[i], &sn, &cs);
      float fx = (float)acc[i] * 5.9604644775390625e-08f;
      float fy = (float)acc[n + i] * 5.9604644775390625e-08f;
      fx = fx + (f_ext ? f_ext[i] : 0.0f);
      fy = fy + (f_ext ? f_ext[n + i] : 0.0f);
      fx = fx + f_swim[i] * cs;
      fy = fy + f_swim[i] * sn;
      float tz = torque_z[i];
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
