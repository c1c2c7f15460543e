// swarm_env_block.cuh -- one workgroup per env, the env's state resident in
// LDS: the sub-step loop that k_global, the re-run inside k_check, k_rod_run,
// k_ellipsoid_run and k_langevin_run share.  Per sub-step a counting sort into cells of side
// >= the cutoff, then every particle, in sorted order, sums its pairs over the
// 3 x 3 cells (int64 at 2^-24: independent of visiting order) and is advanced.
// Periodic 2-D boxes of up to kGlobalCH * 1024 particles.
//
// What differs between the kernels is a path: a small struct of
// __forceinline__ hooks (EnvPathBase has the plain colloid's).  PlainEnvPath
// (walls, potential) follows the body in swarm_integrator.cuh, RodEnvPath is
// in swarm_rod.cuh, EllEnvPath in swarm_ellipsoid.cuh and LangevinEnvPath in
// swarm_langevin.cuh.
//
// Part of swarm_integrator.cuh (included there, after sd_step and bd_step):
// not a header to include on its own.
#pragma once

namespace swarm {

#ifdef SWARM_PHASE_TIMING
__device__ unsigned long long g_global_phase[4];  // cycles: sort, forces+step, steps
#endif

// The LDS after cnt[ncell + 1] (swarm_sizes.h:env_lds_words), 8-byte aligned.
template <bool kDirs>
struct EnvLds {
  uint2* sq;     // positions in sorted order
  float2* dir;   // kDirs: the sub-step's directors (cos, sin) in sorted order
  int32_t* sid;  // sorted order: particle index | species << 24
  // particle state by particle index (the forces, velocities and species
  // are re-read from global memory, L1-resident, where used)
  uint32_t *qx, *qy;
  int32_t *ix, *iy;
  uint32_t* an;
  int32_t* tail;  // after an[N]: what a path keeps of its own
};

template <bool kDirs>
__device__ __forceinline__ EnvLds<kDirs> env_lds(int32_t* lsq, int N) {
  EnvLds<kDirs> l;
  l.sq = reinterpret_cast<uint2*>(lsq + ((reinterpret_cast<uintptr_t>(lsq) >> 2) & 1));
  l.dir = reinterpret_cast<float2*>(l.sq + N);
  l.sid = reinterpret_cast<int32_t*>(l.dir + (kDirs ? N : 0));
  l.qx = reinterpret_cast<uint32_t*>(l.sid + N);
  l.qy = l.qx + N;
  l.ix = reinterpret_cast<int32_t*>(l.qy + N);
  l.iy = l.ix + N;
  l.an = reinterpret_cast<uint32_t*>(l.iy + N);
  l.tail = reinterpret_cast<int32_t*>(l.an + N);
  return l;
}

// What is fixed over a run.
struct EnvRun {
  const Derived* __restrict__ d;
  const DevState& st;
  const PairTables* pt;
  PrevSlot prv;  // reuse_forces: sub-step 0 reads this slot
  size_t M, base;
  uint32_t k0, k1;
  uint64_t step0;
  float sx0, sx1, eps24;
  bool sd_mode;
  float g, md;  // steepest descent: step factor and the largest displacement
};

// One particle of one sub-step: its index, species, global index and the
// forces it swims with (first: the previous run's, reuse_forces).
struct EnvParticle {
  int i, sik;
  size_t gi;
  bool first;
  float fs, tz, fex, fey;
};

// A particle's pair sums: force, z-torque and the deep overlaps met (the
// last two for paths whose pair term has them).
struct EnvAcc {
  int64_t ax = 0, ay = 0, at = 0;
  int deep = 0;
};

__device__ __forceinline__ void env_store_vel(const EnvRun& r, size_t gi, float vx, float vy,
                                              float w) {
  r.st.vel[gi] = vx;
  r.st.vel[r.M + gi] = vy;
  r.st.vel[2 * r.M + gi] = 0.0f;
  r.st.omega[gi] = w;
}

// A free colloid's step: sd_step, or bd_step and the velocities on the last
// sub-step.
__device__ __forceinline__ void env_colloid_step(const EnvRun& r, int s, bool last,
                                                 const EnvParticle& q, PState& p, int64_t ax,
                                                 int64_t ay, int& any) {
  const PConst pc = load_pconst(r.d, q.sik);
  if (r.sd_mode) {
    any |= sd_step(pc, p, ax, ay, q.fs, q.tz, q.fex, q.fey, r.g, r.md) ? 1 : 0;
  } else {
    float vx, vy, w;
    bd_step(pc, p, ax, ay, q.fs, q.tz, q.fex, q.fey, r.k0, r.k1, (uint32_t)q.i,
            r.step0 + (uint64_t)s, last, &vx, &vy, &w, q.first ? r.prv.ang[q.gi] : p.an);
    if (last) env_store_vel(r, q.gi, vx, vy, w);
  }
}

// The plain colloid's hooks; a path overrides what it does differently.
struct EnvPathBase {
  static constexpr bool kDirs = false;    // stage the directors with the sorted positions
  static constexpr bool kStamps = false;  // SWARM_PHASE_TIMING: fill g_global_phase
  // beside the zeroing of the cell counts (a barrier follows)
  template <class L>
  __device__ __forceinline__ void begin_step(const L&) const {}
  // pairs that do not interact (i != j)
  __device__ __forceinline__ bool skip(int, int) const { return false; }
  // added to the external force before the pair sums
  __device__ __forceinline__ void field(const EnvRun&, const PState&, float&, float&) const {}
  // i's term from j at r = x_j - x_i; ui, *uj: their directors (kDirs)
  __device__ __forceinline__ void pair(const EnvRun& r, int pk, float rx, float ry, float2,
                                       const float2*, EnvAcc& a) const {
    pair_force(r.pt->cut2[pk], r.pt->sig6[pk], r.eps24, rx, ry, a.ax, a.ay);
  }
  // The particle's step from its sums; true: p goes back to LDS.
  template <class L>
  __device__ __forceinline__ bool step(const EnvRun& r, const L&, int s, bool last,
                                       const EnvParticle& q, PState& p, float2, EnvAcc& a,
                                       int& any) const {
    env_colloid_step(r, s, last, q, p, a.ax, a.ay, any);
    return true;
  }
  // after the sub-step's barrier (not in steepest descent)
  template <class L>
  __device__ __forceinline__ void end_step(const EnvRun&, const L&, int, bool) const {}
};

// All sub-steps (or steepest-descent steps) of env e by one workgroup.
// lsq: the LDS after cnt[ncell + 1].
template <class Path>
__device__ __forceinline__ void block_env_run(const Derived* __restrict__ d, const DevState& st,
                                              int e, int n_steps, uint64_t step0, int lx, int ly,
                                              bool sd_mode, float g, float md, int32_t* cnt,
                                              int32_t* wave_sums, int32_t* lsq,
                                              const PairTables* pt, int rp, const Path& path) {
  constexpr bool kDirs = Path::kDirs;
  const int T = blockDim.x, tid = threadIdx.x, N = st.n;
  const size_t M = (size_t)st.m, base = (size_t)e * N;
  const int ncell = 1 << (lx + ly);
  const int ncx = 1 << lx, ncy = 1 << ly;
  const int loy = ncy >= 3 ? -1 : 0, hiy = ncy >= 3 ? 1 : ncy - 1;
  const EnvRun r = {d,        st,       pt,       prev_slot(st, rp), M,       base, d->key0,
                    d->key1 ^ (uint32_t)e, step0, d->sx[0], d->sx[1], d->eps24, sd_mode, g, md};
  const EnvLds<kDirs> l = env_lds<kDirs>(lsq, N);
  for (int i = tid; i < N; i += T) {
    const size_t gi = base + i;
    l.qx[i] = st.q[gi];
    l.qy[i] = st.q[M + gi];
    l.ix[i] = st.img[gi];
    l.iy[i] = st.img[M + gi];
    l.an[i] = st.ang[gi];
  }
  __syncthreads();
#ifdef SWARM_PHASE_TIMING
  uint64_t t_sort = 0, t_force = 0, tA = 0;
#endif
  for (int s = 0; s < n_steps; ++s) {
#ifdef SWARM_PHASE_TIMING
    if (Path::kStamps && tid == 0) tA = __builtin_amdgcn_s_memtime();
#endif
    for (int c = tid; c <= ncell; c += T) cnt[c] = 0;
    path.begin_step(l);
    __syncthreads();
    for (int i = tid; i < N; i += T) atomicAdd(&cnt[cell_index(l.qx[i], l.qy[i], lx, ly)], 1);
    __syncthreads();
    block_exclusive_scan(cnt, ncell, wave_sums);
    __syncthreads();
    for (int i = tid; i < N; i += T) {
      const uint32_t qx = l.qx[i], qy = l.qy[i];
      const int pos = atomicAdd(&cnt[cell_index(qx, qy, lx, ly)], 1);
      l.sq[pos] = make_uint2(qx, qy);
      if (kDirs) {  // the sub-step's directors, once per particle
        float sn, cs;
        sincos_turn(l.an[i], &sn, &cs);
        l.dir[pos] = make_float2(cs, sn);
      }
      l.sid[pos] = i | ((int)st.species[i] << 24);
    }
    __syncthreads();  // cell c now spans [c ? cnt[c-1] : 0, cnt[c])
#ifdef SWARM_PHASE_TIMING
    if (Path::kStamps && tid == 0) {
      const uint64_t t = __builtin_amdgcn_s_memtime();
      t_sort += t - tA;
      tA = t;
    }
#endif
    const bool last = s == n_steps - 1;
    int any = 0;
    // sorted order: the lanes of a wave take neighbouring particles, so their
    // candidate ranges (a stencil row = one contiguous sorted range, plus a
    // wrap range at the grid edge) are alike and the loops stay converged
    for (int ps = tid; ps < N; ps += T) {
      const int pki = l.sid[ps];
      EnvParticle q;
      q.i = pki & 0xffffff, q.sik = pki >> 24;
      const int i = q.i;
      q.gi = base + i;
      PState pp = {l.qx[i], l.qy[i], l.an[i], l.ix[i], l.iy[i]};
      q.first = st.reuse && s == 0 && !sd_mode;  // reuse_forces: previous run's
      q.fs = q.first ? r.prv.f[q.gi] : st.f_swim[q.gi];
      q.tz = q.first ? r.prv.tz[q.gi] : st.torque_z[q.gi];
      q.fex = st.f_ext[q.gi], q.fey = st.f_ext[M + q.gi];
      path.field(r, pp, q.fex, q.fey);  // (the loads land while the pair sums run)
      const float2 ui = kDirs ? l.dir[ps] : make_float2(0.0f, 0.0f);
      EnvAcc acc;
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
            const int pj = l.sid[jj];
            const int j = pj & 0xffffff;
            if (j == i || path.skip(i, j)) continue;
            const uint2 qj = l.sq[jj];
            const float rx = (float)(int32_t)(qj.x - pp.qx) * r.sx0;
            const float ry = (float)(int32_t)(qj.y - pp.qy) * r.sx1;
            const int pk = q.sik * kMaxSpecies + (pj >> 24);
            path.pair(r, pk, rx, ry, ui, kDirs ? l.dir + jj : nullptr, acc);
          }
        }
      }
      if (path.step(r, l, s, last, q, pp, ui, acc, any)) {
        l.qx[i] = pp.qx;  // the sort of the next sub-step reads qx/qy after a barrier
        l.qy[i] = pp.qy;
        l.ix[i] = pp.ix;
        l.iy[i] = pp.iy;
        l.an[i] = pp.an;
      }
    }
#ifdef SWARM_PHASE_TIMING
    if (Path::kStamps) {
      __syncthreads();
      if (tid == 0) t_force += __builtin_amdgcn_s_memtime() - tA;
    }
#endif
    if (sd_mode) {
      if (!__syncthreads_or(any)) break;
    } else {
      __syncthreads();
      path.end_step(r, l, s, last);
    }
  }
#ifdef SWARM_PHASE_TIMING
  if (Path::kStamps && tid == 0) {
    g_global_phase[0] = t_sort;
    g_global_phase[1] = t_force;
    g_global_phase[2] = (uint64_t)n_steps;
  }
#endif
  __syncthreads();
  for (int i = tid; i < N; i += T) {
    const size_t gi = base + i;
    st.q[gi] = l.qx[i];
    st.q[M + gi] = l.qy[i];
    st.img[gi] = l.ix[i];
    st.img[M + gi] = l.iy[i];
    st.ang[gi] = l.an[i];
  }
}

}  // namespace swarm
