// swarm_rod.cuh -- a rigid rod among the colloids (2-D, periodic box).
//
// Replaces EspressoMD.add_rod's centre particle + VIRTUAL_SITES_RELATIVE
// beads (swarmrl/engine/espresso.py:546-665) and the reward of RotateRod
// (swarmrl/tasks/object_movement/rod_rotation.py,
// swarmrl/utils/colloid_utils.py:29-117).
//
// The rod is rn consecutive particles [first, first + rn) of every env: the
// centre, then rn - 1 beads; bead k sits in signed slot
//   m_k = (-1)^k (k / 2 + 1)      at      centre + m_k delta u,
// u the centre's director.  A rigid body needs, per sub-step, the sum of all
// of its contacts -- a reduction the cluster windows cannot provide -- so an
// engine with a rod runs every sub-step on k_rod_run, one workgroup per env:
// a path of block_env_run (swarm_env_block.cuh), the LDS-resident global
// path's per-sub-step cell sort, pair_force / bd_step / sd_step and int64 sums.
// Per sub-step the rod adds
//   F = sum_b A_b,  S = sum_b m_b A_b          (int64, 2^-24 units, LDS atomics:
//                                               independent of contact order)
//   tau = delta (u_x S_y - u_y S_x) 2^-24      (fp32; u at the sub-step's start)
// then the centre takes one bd_step from (F, tau) with its own noise stream,
// and every bead is re-placed from the centre's new state.  Rod-rod pairs are
// skipped (internal forces of a rigid body).
#pragma once

#include "swarm_integrator.cuh"

namespace swarm {

// swarm_rod_t on the device
struct RodArgs {
  int32_t first, n;
  float delta;
  int32_t fixed;
};

constexpr int kRodMaxParticles = 255;  // rod particles (centre + beads)
constexpr int kRodMaxEnv = 4096;       // particles per env of a rod engine (LDS-resident state)

// signed slot of rod particle b (0: the centre)
__host__ __device__ inline int rod_slot(int b) {
  if (b == 0) return 0;
  const int k = b - 1;
  return (k & 1 ? -1 : 1) * (k / 2 + 1);
}

// What k_rod_run keeps after the particle state (EnvLds::tail, the last
// argument of env_lds_words), in 4-byte words: the plain layout's spare word,
// two for the alignment to 8 bytes, the rod's four int64 sums and the centre's
// velocities (v_x, v_y, omega and a pad).
constexpr size_t kRodTailWords = 1 + 2 + 8 + 4;

// Bead b (1 <= b < rn) from the centre's state: per axis
//   dq = f2i32_sat(((m delta) cos|sin) inv_sx)
// added to the centre's (q, img); r: the lever (m delta) (cos, sin).
__device__ __forceinline__ void rod_place(const RodArgs& rod, int b, uint32_t cqx, uint32_t cqy,
                                          int32_t cix, int32_t ciy, float sn, float cs,
                                          float inv_sx0, float inv_sx1, PState& p, float* rx,
                                          float* ry) {
  const float lever = (float)rod_slot(b) * rod.delta;
  *rx = lever * cs;
  *ry = lever * sn;
  p.qx = cqx;
  p.qy = cqy;
  p.ix = cix;
  p.iy = ciy;
  advance(p.qx, p.ix, f2i32_sat(*rx * inv_sx0));
  advance(p.qy, p.iy, f2i32_sat(*ry * inv_sx1));
}

// block_env_run with a rod: rod-rod pairs are skipped, a rod particle only
// adds its pair sum to the rod's, and after the colloids' step the centre
// takes its own and the beads follow it.
struct RodEnvPath : EnvPathBase {
  RodArgs rod;
  float inv_sx0, inv_sx1;
  // the rod's sums (F_x, F_y, S_x, S_y); after them the centre's (v_x, v_y, omega)
  template <class L>
  __device__ __forceinline__ unsigned long long* sums(const L& l) const {
    return reinterpret_cast<unsigned long long*>(
        l.tail + ((reinterpret_cast<uintptr_t>(l.tail) >> 2) & 1));
  }
  __device__ __forceinline__ bool in_rod(int i) const {
    return i >= rod.first && i < rod.first + rod.n;
  }
  template <class L>
  __device__ __forceinline__ void begin_step(const L& l) const {
    if (threadIdx.x < 4) sums(l)[threadIdx.x] = 0ull;
  }
  // rod-rod: internal to the rigid body
  __device__ __forceinline__ bool skip(int i, int j) const { return in_rod(i) && in_rod(j); }
  template <class L>
  __device__ __forceinline__ bool step(const EnvRun& r, const L& l, int s, bool last,
                                       const EnvParticle& q, PState& p, float2, EnvAcc& a,
                                       int& any) const {
    if (!in_rod(q.i)) {
      env_colloid_step(r, s, last, q, p, a.ax, a.ay, any);
      return true;
    }
    // the rod moves as one body (and not at all in the overlap removal): its
    // particles only add to the sums
    if (!r.sd_mode && (a.ax != 0 || a.ay != 0)) {
      unsigned long long* acc = sums(l);
      const int64_t m = (int64_t)rod_slot(q.i - rod.first);
      atomicAdd(&acc[0], (unsigned long long)a.ax);
      atomicAdd(&acc[1], (unsigned long long)a.ay);
      atomicAdd(&acc[2], (unsigned long long)(m * a.ax));
      atomicAdd(&acc[3], (unsigned long long)(m * a.ay));
    }
    return false;
  }
  // (the sub-step's barrier: the rod's sums are complete)
  template <class L>
  __device__ __forceinline__ void end_step(const EnvRun& r, const L& l, int s, bool last) const {
    const int T = blockDim.x, tid = threadIdx.x, r0 = rod.first;
    const size_t base = r.base;
    const DevState& st = r.st;
    unsigned long long* acc = sums(l);
    float* cv = reinterpret_cast<float*>(acc + 4);
    if (tid == 0) {  // the centre: one bd_step from (F, tau), its own noise stream
      PState pc_ = {l.qx[r0], l.qy[r0], l.an[r0], l.ix[r0], l.iy[r0]};
      const PState old = pc_;
      float sn, cs;
      sincos_turn(pc_.an, &sn, &cs);
      const float Sx = i64_to_f32((int64_t)acc[2]), Sy = i64_to_f32((int64_t)acc[3]);
      const float t1 = cs * Sy, t2 = sn * Sx;
      const float cr = t1 - t2;
      const float tau = (rod.delta * cr) * 5.9604644775390625e-08f;
      const PConst pc = load_pconst(r.d, (int)st.species[r0]);
      float vx = 0.0f, vy = 0.0f, w = 0.0f;
      bd_step(pc, pc_, (int64_t)acc[0], (int64_t)acc[1], 0.0f, tau, 0.0f, 0.0f, r.k0, r.k1,
              (uint32_t)r0, r.step0 + (uint64_t)s, last, &vx, &vy, &w, pc_.an);
      if (rod.fixed) {  // no translation and no translational velocity
        pc_.qx = old.qx;
        pc_.qy = old.qy;
        pc_.ix = old.ix;
        pc_.iy = old.iy;
        vx = 0.0f;
        vy = 0.0f;
      }
      l.qx[r0] = pc_.qx;
      l.qy[r0] = pc_.qy;
      l.ix[r0] = pc_.ix;
      l.iy[r0] = pc_.iy;
      l.an[r0] = pc_.an;
      if (last) {
        cv[0] = vx;
        cv[1] = vy;
        cv[2] = w;
        env_store_vel(r, base + r0, vx, vy, w);
      }
    }
    __syncthreads();  // the centre's new state
    for (int b = 1 + tid; b < rod.n; b += T) {
      float sn, cs, rx, ry;
      sincos_turn(l.an[r0], &sn, &cs);
      PState pb;
      rod_place(rod, b, l.qx[r0], l.qy[r0], l.ix[r0], l.iy[r0], sn, cs, inv_sx0, inv_sx1, pb, &rx,
                &ry);
      const int i = r0 + b;
      l.qx[i] = pb.qx;
      l.qy[i] = pb.qy;
      l.ix[i] = pb.ix;
      l.iy[i] = pb.iy;
      l.an[i] = l.an[r0];
      if (last) {  // v_b = v_c + omega x r_b
        const float w = cv[2];
        env_store_vel(r, base + i, cv[0] - w * ry, cv[1] + w * rx, w);
      }
    }
    // (no barrier here: the next sub-step zeroes cnt and the sums, which
    // nobody reads any more, and meets a barrier before it reads positions)
  }
};

// Rod-engine launch: n_steps sub-steps (or SD steps) of every env, one
// 1024-thread workgroup per env (k_global's contract: reuse_forces slots,
// device step counter).
__global__ __launch_bounds__(1024) void k_rod_run(const Derived* __restrict__ d, DevState st,
                                                  RodArgs rod, int n_steps,
                                                  uint64_t* __restrict__ step_ctr,
                                                  uint32_t* __restrict__ arrive, int lx, int ly,
                                                  int sd_mode, float g, float md) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ PairTables pt;
  stage_pair_tables(d, &pt);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  const uint64_t step0 = sd_mode ? 0ull : *step_ctr;
  const int par = window_parity(step_ctr);
  block_env_run(d, st, blockIdx.x, n_steps, step0, lx, ly, sd_mode != 0, g, md, cnt, wave_sums,
                cnt + (1 << (lx + ly)) + 1, &pt, par,
                RodEnvPath{{}, rod, d->inv_sx[0], d->inv_sx[1]});
  save_forces_env(st, blockIdx.x, sd_mode ? par : par ^ 1);
  if (!sd_mode) advance_counter(step_ctr, arrive, step0, n_steps);
}

// The beads of every env onto the centre's line (once, when the rod is set
// or a new fp64 state is uploaded): one thread per (env, bead).
__global__ __launch_bounds__(256) void k_rod_snap(const Derived* __restrict__ d, DevState st,
                                                  RodArgs rod, int n_envs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int nb = rod.n - 1;
  if (t >= n_envs * nb) return;
  const int e = t / nb, b = 1 + t % nb;
  const size_t M = (size_t)st.m, gc = (size_t)e * st.n + rod.first, gi = gc + b;
  float sn, cs, rx, ry;
  sincos_turn(st.ang[gc], &sn, &cs);
  PState p;
  rod_place(rod, b, st.q[gc], st.q[M + gc], st.img[gc], st.img[M + gc], sn, cs, d->inv_sx[0],
            d->inv_sx[1], p, &rx, &ry);
  st.q[gi] = p.qx;
  st.q[M + gi] = p.qy;
  st.img[gi] = p.ix;
  st.img[M + gi] = p.iy;
  st.ang[gi] = st.ang[gc];
  // (both reuse_forces slots: the orientation of the last force calculation)
  st.ang_prev[gi] = st.ang[gc];
  st.ang_prev[M + gi] = st.ang[gc];
}

// w_i of k_rod_reward for the colloid at global index gi
__device__ __forceinline__ double rod_weight(const DevState& st, const RodArgs& rod, size_t gc,
                                             size_t gi, double L0, double L1, double ux,
                                             double uy) {
  const size_t M = (size_t)st.m;
  const double xi = ((double)st.img[gi] + (double)st.q[gi] / 4294967296.0) * L0;
  const double yi = ((double)st.img[M + gi] + (double)st.q[M + gi] / 4294967296.0) * L1;
  double fx = 0.0, fy = 0.0;
  for (int b = 0; b < rod.n; ++b) {
    const size_t gb = gc + b;
    const double rx = ((double)st.img[gb] + (double)st.q[gb] / 4294967296.0) * L0 - xi;
    const double ry = ((double)st.img[M + gb] + (double)st.q[M + gb] / 4294967296.0) * L1 - yi;
    const double r2 = rx * rx + ry * ry;
    const double r4 = r2 * r2;
    const double r14 = r4 * r4 * r4 * r2;
    const double c = -12.0 / r14;
    fx += c * rx;
    fy += c * ry;
  }
  return fabs(ux * fy - uy * fx) + 1e-8;
}

// RotateRod's reward (rod_rotation.py:87-219, colloid_utils.py:29-117) for
// every env, one workgroup per env, in fp64:
//   step  = wrapped (centre angle - historic angle) 360 / 2^32   [degrees]
//   pushed into the env's history ring [H]; mean over its filled entries
//   w_i   = |u x sum_b f_ib| + 1e-8,  f_ib = grad(1 / |r|^12) = -12 r / |r|^14,
//           r = r_b - r_i (xy of the unwrapped positions, no minimum image),
//           u the director
//   out[e][a] = scale mean w_a / sum_a w_a      (partition = 0: scale mean / A)
// hist_ang [E], ring [E][H] and count [E] are the task's device state.
__global__ __launch_bounds__(256) void k_rod_reward(DevState st, RodArgs rod,
                                                    const double* __restrict__ box,
                                                    const int32_t* __restrict__ agent_idx,
                                                    int n_agents, uint32_t* __restrict__ hist_ang,
                                                    double* __restrict__ ring,
                                                    int32_t* __restrict__ count, int history,
                                                    double scale, int partition,
                                                    float* __restrict__ out) {
  __shared__ double red[256];
  __shared__ double s_mean;
  const int e = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const size_t base = (size_t)e * st.n, gc = base + rod.first;
  const uint32_t ang = st.ang[gc];
  if (tid == 0) {
    const int32_t dang = (int32_t)(ang - hist_ang[e]);
    const double step = (double)dang * (360.0 / 4294967296.0);
    const int c = count[e];
    double* r = ring + (size_t)e * history;
    r[c % history] = step;
    const int filled = min(c + 1, history);
    double sum = 0.0;
    for (int k = 0; k < filled; ++k) sum += r[k];
    s_mean = sum / (double)filled;
    // (the count stays below 2 H so that it never overflows)
    count[e] = c + 1 >= 2 * history ? c + 1 - history : c + 1;
    hist_ang[e] = ang;
  }
  const double L0 = box[0], L1 = box[1];
  const double th = (double)ang * (6.283185307179586476925 / 4294967296.0);
  const double ux = cos(th), uy = sin(th);
  double wsum = 0.0;
  if (partition) {
    for (int a = tid; a < n_agents; a += T) {
      wsum += rod_weight(st, rod, gc, base + agent_idx[a], L0, L1, ux, uy);
    }
  }
  red[tid] = wsum;
  __syncthreads();
  for (int h = T / 2; h > 0; h >>= 1) {  // fixed order: the same bits on every run
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const double total = red[0];
  const double reward = scale * s_mean;
  for (int a = tid; a < n_agents; a += T) {
    double part;
    if (partition) {
      // the colloid's own weight again (not kept: any number of agents per thread)
      part = rod_weight(st, rod, gc, base + agent_idx[a], L0, L1, ux, uy) / total;
    } else {
      part = 1.0 / (double)n_agents;
    }
    out[(size_t)e * n_agents + a] = (float)(reward * part);
  }
}

}  // namespace swarm
