// swarm_observe.cuh -- the observable and reward kernels of the engine:
//
//   k_grid_build        per-env cell list in global memory
//   k_vision*           SubdividedVisionCones over cell-sorted records, with the
//                       rollout policy as a tail (k_vision_policy*)
//   k_vgrid_sort, k_vision_pairs, k_vision_policy_cbuild, k_policy_cbuild
//                       the same with a stage of the deferred cluster build
//                       riding along as extra workgroups
//   k_neighbor_reduce, k_pair_dist   fp64 neighbour sums, pairwise distances
//   k_field             ConcentrationField / GradientSensing distances
//   k_field_vgrid_sort  the reward launch carrying the build sort, the next
//                       vision grid and (kCheck) the last window's check
//   k_pairs             neighbour pairs (parity helper)
//   k_traj_write, k_traj_bump   the trajectory ring
//
// Device code only; the launches are in swarm_engine_host.cuh and
// swarm_engine.hip.  Included after the integrator and policy headers, whose
// bodies the fused kernels call (swarm_integrator.cuh: build_sort_body,
// build_pairs_body, cluster_build_env, check bodies; swarm_policy.cuh:
// MlpArgs, policy_body).  The kernels stay in the anonymous namespace: the
// profiles and tools name them so.
#pragma once

#include <cstdint>

#include "../../include/swarmrl_amd.h"
#include "swarm_device.cuh"
#include "swarm_integrator.cuh"
#include "swarm_policy.cuh"

namespace {

using swarm::Derived;
using swarm::DevState;
using swarm::Scratch;
using swarm::cell_index;
using swarm::block_exclusive_scan;

constexpr int kMaxSpecies = SWARM_MAX_SPECIES;

// Cell-sorted 32-byte record of one particle for the observables, read as
// two 16-byte loads: {qx, qy, ix, iy}, {radius bits, particle, type slot, 0}.
struct VisionSorted {
  uint4* rec;          // [E * N][2]
  int32_t* agent_row;  // [N] row of a particle in the agent list, -1 if none
};

// ------------------------------------------------- global per-env grid
// Counting sort of every env into cells (side >= cutoff), written to global
// memory: start[E][ncell+1], sorted particle index order[E][N].
__global__ __launch_bounds__(1024) void k_grid_build(DevState st, int lx, int ly,
                                                     int32_t* __restrict__ start,
                                                     int32_t* __restrict__ order) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int e = blockIdx.x, T = blockDim.x, tid = threadIdx.x, N = st.n;
  const int ncell = 1 << (lx + ly);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  for (int c = tid; c <= ncell; c += T) cnt[c] = 0;
  __syncthreads();
  const size_t M = (size_t)st.m;
  for (int i = tid; i < N; i += T) {
    const size_t g = (size_t)e * N + i;
    atomicAdd(&cnt[cell_index(st.q[g], st.q[M + g], lx, ly)], 1);
  }
  __syncthreads();
  block_exclusive_scan(cnt, ncell, wave_sums);
  __syncthreads();
  int32_t* so = start + (size_t)e * (ncell + 1);
  for (int c = tid; c <= ncell; c += T) so[c] = cnt[c];
  __syncthreads();
  for (int i = tid; i < N; i += T) {
    const size_t g = (size_t)e * N + i;
    const int pos = atomicAdd(&cnt[cell_index(st.q[g], st.q[M + g], lx, ly)], 1);
    order[(size_t)e * N + pos] = i;
  }
}

// Vision records (cell-sorted, 2 x uint4 per colloid):
//   {q_x, q_y, img_x, img_y}, {radius bits, id | (type slot + 1) << 24, angle, 0}
// (type slot -1: a type the observable does not detect).  The angle rides
// along so an agent's director needs no dependent load.
__device__ __forceinline__ uint32_t vision_id_word(int i, int ti) {
  return (uint32_t)i | ((uint32_t)(ti + 1) << 24);
}
__device__ __forceinline__ int vision_rec_id(uint32_t w) { return (int)(w & 0xffffffu); }
__device__ __forceinline__ int vision_rec_type(uint32_t w) { return (int)(w >> 24) - 1; }

// Vision grid: counting sort of every env into cells of side >= vision range,
// writing cell-sorted records so a candidate cell is one contiguous run; the
// env-0 workgroup also inverts the agent list (agent_row).
// The vision-cone launch arguments (one struct, so fused launches carry it).
struct VisionArgs {
  swarm_vision_params_t vp;
  int lx, ly;
  const float* radii;
  const int32_t* types;
  const int32_t* agents;
  int n_agents;
  int32_t* start;
  VisionSorted vs;
  float* out;
  int n_envs;
  int staged;  // 1: the records are scattered into LDS, then written in order
  unsigned long long* rstamp;  // role stamps of the launch (profiling), or null
};

// Body for the workgroup of env e (k_vision_grid, or k_vgrid_sort).
__device__ __forceinline__ void vision_grid_body(const DevState& st, const VisionArgs& va, int e,
                                                 unsigned char* smem) {
  const swarm_vision_params_t& vp = va.vp;
  const int lx = va.lx, ly = va.ly;
  const float* __restrict__ radii = va.radii;
  const int32_t* __restrict__ types = va.types;
  const int32_t* __restrict__ agents = va.agents;
  const int n_agents = va.n_agents;
  int32_t* __restrict__ start = va.start;
  const VisionSorted& vs = va.vs;
  const int T = blockDim.x, tid = threadIdx.x, N = st.n;
  const int ncell = 1 << (lx + ly);
  int32_t* wave_sums = reinterpret_cast<int32_t*>(smem);
  int32_t* cnt = wave_sums + 16;
  for (int c = tid; c <= ncell; c += T) cnt[c] = 0;
  if (e == 0)
    for (int i = tid; i < N; i += T) vs.agent_row[i] = -1;
  __syncthreads();
  if (e == 0) {  // agents' rows: their ids loaded together (one memory latency)
    constexpr int kA = 8;
    for (int a0 = tid; a0 < n_agents; a0 += kA * T) {
      int ag[kA];
#pragma unroll
      for (int u = 0; u < kA; ++u) ag[u] = a0 + u * T < n_agents ? agents[a0 + u * T] : -1;
#pragma unroll
      for (int u = 0; u < kA; ++u)
        if ((unsigned)ag[u] < (unsigned)N) vs.agent_row[ag[u]] = a0 + u * T;
    }
  }
  const size_t M = (size_t)st.m, base = (size_t)e * N;
  int32_t* so = start + (size_t)e * (ncell + 1);
  constexpr int kPer = 8;  // colloids per thread kept in registers (N <= 8 T)
  if (N <= kPer * T) {
    // every colloid's record fields are loaded once, up front, so their
    // latency overlaps the count and the scan
    uint4 r0[kPer], r1[kPer];
    int cell[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int i = tid + k * T;
      if (i < N) {
        const size_t g = base + i;
        const uint32_t qx = st.q[g], qy = st.q[M + g];
        const int tj = types[i];
        int ti = -1;
        for (int tt = 0; tt < vp.n_types; ++tt)
          if (vp.detected_types[tt] == tj) ti = tt;
        r0[k] = make_uint4(qx, qy, (uint32_t)st.img[g], (uint32_t)st.img[M + g]);
        r1[k] = make_uint4(__float_as_uint(radii[i]), vision_id_word(i, ti), st.ang[g], 0u);
        cell[k] = cell_index(qx, qy, lx, ly);
        atomicAdd(&cnt[cell[k]], 1);
      }
    }
    __syncthreads();
    block_exclusive_scan(cnt, ncell, wave_sums);
    __syncthreads();
    for (int c = tid; c <= ncell; c += T) so[c] = cnt[c];
    __syncthreads();
    if (va.staged) {
      // scatter into LDS (16-byte aligned after the counts), then write the
      // records in order: coalesced stores instead of 2 N scattered ones
      uint4* lrec = reinterpret_cast<uint4*>(
          smem + (((16 + (size_t)ncell + 1) * 4 + 15) & ~(size_t)15));
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        if (tid + k * T < N) {
          const int pos = atomicAdd(&cnt[cell[k]], 1);
          lrec[2 * pos] = r0[k];
          lrec[2 * pos + 1] = r1[k];
        }
      }
      __syncthreads();
      uint4* grec = vs.rec + 2 * base;
      for (int p = tid; p < 2 * N; p += T) grec[p] = lrec[p];
      return;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (tid + k * T < N) {
        const size_t pos = base + atomicAdd(&cnt[cell[k]], 1);
        vs.rec[2 * pos] = r0[k];
        vs.rec[2 * pos + 1] = r1[k];
      }
    }
    return;
  }
  for (int i = tid; i < N; i += T)
    atomicAdd(&cnt[cell_index(st.q[base + i], st.q[M + base + i], lx, ly)], 1);
  __syncthreads();
  block_exclusive_scan(cnt, ncell, wave_sums);
  __syncthreads();
  for (int c = tid; c <= ncell; c += T) so[c] = cnt[c];
  __syncthreads();
  for (int i = tid; i < N; i += T) {
    const size_t g = base + i;
    const uint32_t qx = st.q[g], qy = st.q[M + g];
    const size_t pos = base + atomicAdd(&cnt[cell_index(qx, qy, lx, ly)], 1);
    const int tj = types[i];
    int ti = -1;
    for (int tt = 0; tt < vp.n_types; ++tt)
      if (vp.detected_types[tt] == tj) ti = tt;
    vs.rec[2 * pos] = make_uint4(qx, qy, (uint32_t)st.img[g], (uint32_t)st.img[M + g]);
    vs.rec[2 * pos + 1] = make_uint4(__float_as_uint(radii[i]), vision_id_word(i, ti), st.ang[g], 0u);
  }
}

__global__ __launch_bounds__(1024) void k_vision_grid(DevState st, VisionArgs va) {
  extern __shared__ __align__(16) unsigned char smem[];
  vision_grid_body(st, va, blockIdx.x, smem);
}

// ---------------------------------------------------------- vision cone
// One group of G lanes per cell-sorted particle (neighbouring groups share
// candidate cells, so their record loads coalesce); groups of particles
// that are not agents exit.  The candidates of the 3x3 cell stencil form one
// flat index range that the G lanes split.  Two phases, so that the lanes of
// a wave stay converged: a cheap range test over the candidates appends the
// hits to a per-lane list in LDS, and the cone arithmetic (sqrt, divisions,
// acos) then runs over the hits only, four at a time; a full list is drained
// early.  Each lane keeps NB bins (>= n_cones * n_types) of 2^-32
// fixed-point amplitude in registers, and the group adds them with
// xor-shuffles.  Integer sums make the result independent of G, of the
// visiting order and of the phase split.
constexpr int kVisionHits = 16;  // per-lane hit list (LDS, [kVisionHits][256])

struct VisionLane {
  uint32_t qxi, qyi;
  int32_t ixi, iyi;
  int i;
  float mx, my, sx0, sx1, R;
};

// The in-range test of one candidate record (shared by both phases).
// kAny: vision_range may reach half the box or more (the all-records scan):
// every unwrapped separation is converted from int64.
template <bool kAny = false>
__device__ __forceinline__ bool vision_offsets(const VisionLane& L, const uint4& c0, float* dx,
                                               float* dy) {
  const int64_t dqx = ((int64_t)((int32_t)c0.z - L.ixi) * (int64_t)4294967296LL) +
                      ((int64_t)c0.x - (int64_t)L.qxi);
  const int64_t dqy = ((int64_t)((int32_t)c0.w - L.iyi) * (int64_t)4294967296LL) +
                      ((int64_t)c0.y - (int64_t)L.qyi);
  if (kAny) {
    *dx = (float)dqx * L.sx0;
    *dy = (float)dqy * L.sx1;
  } else {
    // unwrapped separations beyond half a box are never within range
    // (vision_range < L/2): skip them and convert the rest from int32, whose
    // conversion is a single exact-rounding instruction.
    if (dqx < -2147483647LL || dqx > 2147483647LL || dqy < -2147483647LL ||
        dqy > 2147483647LL)
      return false;
    *dx = (float)(int32_t)dqx * L.sx0;
    *dy = (float)(int32_t)dqy * L.sx1;
  }
  const float dist2 = *dx * *dx + *dy * *dy;
  // conservative pre-test on dist^2 (the exact test is on the fp32 sqrt)
  return dist2 < L.R * L.R * 1.0001f && dist2 != 0.0f;
}

// Cheap pre-test for the candidate scan: the minimum-image separation (int32
// wrap of the fraction difference) in range.  A candidate that passes
// vision_offsets passes this one (its unwrapped separation fits int32 and so
// equals the wrapped one); vision_hit re-tests the listed ones exactly.
__device__ __forceinline__ bool vision_near(const VisionLane& L, const uint4& c0) {
  const float dx = (float)(int32_t)(c0.x - L.qxi) * L.sx0;
  const float dy = (float)(int32_t)(c0.y - L.qyi) * L.sx1;
  const float dist2 = dx * dx + dy * dy;
  return dist2 < L.R * L.R * 1.0001f && dist2 != 0.0f;
}

template <int NB, bool kAny = false>
__device__ __forceinline__ void vision_hit(const VisionLane& L, const swarm_vision_params_t& vp,
                                           const uint4& c0, const uint4& c1, int64_t* acc) {
  float dx, dy;
  if (!vision_offsets<kAny>(L, c0, &dx, &dy)) return;
  const int ti = vision_rec_type(c1.y);
  if (ti < 0 || vision_rec_id(c1.y) == L.i) return;
  // (dist^2 >= sx0^2 ~ 1e-14: positive and normal, no special cases)
  const float dist = swarm::sqrt_pos(dx * dx + dy * dy);
  if (!(dist < L.R)) return;
  float amp = (2.0f * __uint_as_float(c1.x)) / dist;
  amp = fminf(1.0f, amp);
  const float ux = dx / dist, uy = dy / dist;
  float dot = ux * L.mx + uy * L.my;
  dot = fminf(fmaxf(dot, -1.0f), 1.0f);
  float an = swarm::acosf_fixed(dot);
  const float orth = ux * (-L.my) + uy * L.mx;
  if (orth < 0.0f) an = -an;
  const int64_t fixed = __float2ll_rn(amp * 4294967296.0f);
  int bin = -1;
  for (int k = 0; k < vp.n_cones; ++k)
    if (vp.rims[k] < an && an < vp.rims[k + 1]) bin = k * vp.n_types + ti;
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] += (b == bin) ? fixed : 0;
}

// Cone arithmetic over a lane's listed hits, records fetched four at a time.
template <int NB, bool kAny = false, int BS = 256>
__device__ __forceinline__ void vision_drain(const VisionLane& L, const swarm_vision_params_t& vp,
                                             const uint4* __restrict__ rec, size_t base,
                                             const uint32_t (*hits)[BS], int nh, int64_t* acc) {
  for (int k0 = 0; __any(k0 < nh); k0 += 4) {  // over the active lanes' longest list
    uint4 c0[4], c1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (k0 + u < nh) {
        const size_t jj = base + hits[k0 + u][threadIdx.x];
        c0[u] = rec[2 * jj];
        c1[u] = rec[2 * jj + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k0 + u < nh) vision_hit<NB, kAny>(L, vp, c0[u], c1[u], acc);
  }
}

// The same over the G lanes' lists of a group together: the group's hits,
// concatenated in lane order, are dealt round-robin to its lanes, so a lane
// evaluates ceil(total / G) of them instead of its own list's length (the
// wave runs as long as its longest: ~6 hits of Poisson(2) lists against ~4
// of the balanced ones at E = 64).  Integer bin sums: the same result.
// Whole groups are active together (they share one agent).
template <int NB, int G, bool kAny = false, int BS = 256>
__device__ __forceinline__ void vision_drain_group(const VisionLane& L,
                                                   const swarm_vision_params_t& vp,
                                                   const uint4* __restrict__ rec, size_t base,
                                                   const uint32_t (*hits)[BS], int nh,
                                                   int64_t* acc) {
  // the other lanes' list entries are read below: keep the compiler from
  // moving those LDS reads above this lane's writes (one wave's LDS
  // operations complete in order)
  __asm__ volatile("" ::: "memory");
  const int sub = threadIdx.x & (G - 1);
  const int lane0 = (threadIdx.x & 63) - sub;  // the group's first lane in the wave
  const int tid0 = threadIdx.x - sub;
  int cnt[G];
  int total = 0;
#pragma unroll
  for (int l = 0; l < G; ++l) {
    cnt[l] = __shfl(nh, lane0 + l, 64);
    total += cnt[l];
  }
  for (int h0 = sub; __any(h0 < total); h0 += 4 * G) {
    uint4 c0[4], c1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int h = h0 + u * G;
      if (h < total) {
        int owner = 0, k = h, pre = 0;
#pragma unroll
        for (int l = 0; l < G; ++l) {
          const bool in = h >= pre && h < pre + cnt[l];
          owner = in ? l : owner;
          k = in ? h - pre : k;
          pre += cnt[l];
        }
        const size_t jj = base + hits[k][tid0 + owner];
        c0[u] = rec[2 * jj];
        c1[u] = rec[2 * jj + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (h0 + u * G < total) vision_hit<NB, kAny>(L, vp, c0[u], c1[u], acc);
  }
}

// What a vision group does with its agent's summed bins (every lane of the
// group holds them): FeatureTail writes the observable row; PolicyTail
// (swarm_vision_policy) also runs the actor MLP and the sampling on them.
// pre() runs as soon as the agent's row is known (its loads overlap the
// candidate scan), done() after the group's reduction.
struct FeatureTail {
  using Pre = int;
  __device__ Pre pre(const VisionArgs&, int, int) const { return 0; }
  template <int NB, int G>
  __device__ void done(const VisionArgs& va, int e, int row, int sub, const int64_t (&acc)[NB],
                       Pre) const {
    if (sub != 0) return;
    const int nb = va.vp.n_cones * va.vp.n_types;
    float* o = va.out + ((size_t)e * va.n_agents + row) * nb;
#pragma unroll
    for (int k = 0; k < NB; ++k)
      if (k < nb) o[k] = (float)acc[k] * 2.3283064365386963e-10f;
  }
};

// The observable row, then the rollout policy of the same agent (flat agent
// a = e * n_agents + row, as swarm_policy_mlp_sample sees the flattened
// observable): the actor MLP over the group's G lanes, weights read in place
// (mlp_group_logits_direct), and lane 0 samples with the agent's own call
// counter state[a] (one group handles an agent per launch, so it reads and
// advances it alone: no block barrier, no atomic).
template <int D, int K>
struct PolicyTail {
  swarm::MlpArgs m;
  const float* sw = nullptr;  // the weights staged in LDS (stage_mlp_rows), or read in place
  using Pre = unsigned long long;
  __device__ Pre pre(const VisionArgs& va, int e, int row) const {
    return m.state[(size_t)e * va.n_agents + row];
  }
  template <int NB, int G>
  __device__ void done(const VisionArgs& va, int e, int row, int sub, const int64_t (&acc)[NB],
                       Pre ctr) const {
    static_assert(NB <= D, "the fused policy takes the bins as its features");
    const int nb = va.vp.n_cones * va.vp.n_types;
    const int a = e * va.n_agents + row;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < NB; ++k)
      if (k < nb) x[k] = (float)acc[k] * 2.3283064365386963e-10f;
    if (sub == 0) {
      float* o = va.out + (size_t)a * nb;
#pragma unroll
      for (int k = 0; k < D; ++k)
        if (k < nb) o[k] = x[k];
    }
    float lg[K];
    if (sw)
      swarm::mlp_group_logits<G, D, K>(m, sw, x, sub, lg);
    else
      swarm::mlp_group_logits_direct<G, D, K>(m, x, sub, lg);
    if (sub == 0) {
      swarm::policy_emit<K>(m, a, lg, ctr);
      m.state[a] = ctr + 1ull;
    }
  }
};

// kAll: vision_range >= half the box (the reference has no range limit,
// subdivided_vision_cones.py:116-121): every record of the env is a
// candidate, tested on its unwrapped (int64) separation.
// xcd_bpe > 0: blocks placed on XCDs by env (swarm::xcd_env_block, xcd_bpe
// blocks per env), so the records an env's agents read stay in one L2.
// Body for block vb (k_vision, or a workgroup of k_vision_pairs /
// k_vision_cbuild); hits: the block's [kVisionHits][BS] LDS hit lists
// (blockDim BS).
template <int NB, int G, bool kAll = false, int BS = 256, class Tail = FeatureTail>
__device__ __forceinline__ void vision_body(const DevState& st, const Derived* __restrict__ d,
                                            const VisionArgs& va, int vb, int xcd_bpe,
                                            uint32_t (*hits)[BS], const Tail& tail = Tail{}) {
  const swarm_vision_params_t& vp = va.vp;
  const int lx = va.lx, ly = va.ly;
  const int32_t* __restrict__ start = va.start;
  const VisionSorted& vs = va.vs;
  const int n_envs = va.n_envs;
  const int N = st.n;
  const int sub = threadIdx.x & (G - 1);
  int e, ps;
  if (xcd_bpe > 0) {
    int lb;
    if (!swarm::xcd_env_block(vb, xcd_bpe, n_envs, &e, &lb)) return;
    ps = (lb * (int)blockDim.x + (int)threadIdx.x) / G;
    if (ps >= N) return;  // whole groups only (G divides 64)
  } else {
    const int grp = (vb * (int)blockDim.x + (int)threadIdx.x) / G;
    if (grp >= n_envs * N) return;
    e = grp / N;
    ps = grp - e * N;
  }
  const size_t base = (size_t)e * N;
  const uint4 own0 = vs.rec[2 * (base + ps)];
  const uint4 own1 = vs.rec[2 * (base + ps) + 1];
  VisionLane L;
  L.i = vision_rec_id(own1.y);
  const int row = vs.agent_row[L.i];
  // (the candidate ranges below load beside agent_row: both wait on the own
  // record only; a non-agent group leaves after them)
  L.qxi = own0.x;
  L.qyi = own0.y;
  L.ixi = (int32_t)own0.z;
  L.iyi = (int32_t)own0.w;
  float sn, cs;
  swarm::sincos_turn(own1.z, &sn, &cs);
  const float nm = swarm::sqrt_pos(cs * cs + sn * sn);  // ~1
  L.mx = cs / nm;
  L.my = sn / nm;
  L.sx0 = d->sx[0];
  L.sx1 = d->sx[1];
  L.R = vp.vision_range;
  int64_t acc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0;
  const int ncell = 1 << (lx + ly);
  const int ncx = 1 << lx, ncy = 1 << ly;
  const int loy = ncy >= 3 ? -1 : 0, hiy = ncy >= 3 ? 1 : ncy - 1;
  const int cc0 = cell_index(L.qxi, L.qyi, lx, ly);
  const int cx = cc0 & (ncx - 1), cy = cc0 >> lx;
  const int32_t* so = start + (size_t)e * (ncell + 1);
  int nh = 0;
  // the 3x3 candidate cells as one flat index range [0, total): a stencil
  // row (cells x-1..x+1) is one contiguous sorted range, plus one wrap cell
  // at the grid edge -- six ranges, their 12 bounds loaded together; then
  // candidates four at a time per lane (their record loads in flight
  // together), a lane taking f = sub, sub + G, ...; record index j = f +
  // off[r] of the range r holding f
  const int xa = ncx >= 3 ? max(cx - 1, 0) : 0;
  const int xb = ncx >= 3 ? min(cx + 1, ncx - 1) : ncx - 1;
  const int xw = ncx >= 3 ? (cx == 0 ? ncx - 1 : (cx == ncx - 1 ? 0 : -1)) : -1;
  int off[6], pre[7];
  pre[0] = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int oy = loy + (r >> 1), part = r & 1;
    int jb = 0, je = 0;
    if (kAll) {  // one range: all records
      je = r == 0 ? N : 0;
    } else if (oy <= hiy && (part == 0 || xw >= 0)) {
      const int row = ((cy + oy + ncy) & (ncy - 1)) << lx;
      jb = so[row | (part == 0 ? xa : xw)];
      je = so[(row | (part == 0 ? xb : xw)) + 1];
    }
    off[r] = jb - pre[r];
    pre[r + 1] = pre[r] + (je - jb);
  }
  if (row < 0) return;
  const typename Tail::Pre tail_pre = tail.pre(va, e, row);
  const int total = pre[6];
  // kVF candidates per lane in flight per round
  constexpr int kVF = 4;
  // (group-uniform trip count: a drain below always finds whole groups)
  for (int f00 = 0; f00 < total; f00 += kVF * G) {
    const int f0 = f00 + sub;
    uint4 c0[kVF];
    int jj[kVF];
#pragma unroll
    for (int u = 0; u < kVF; ++u) {
      const int f = f0 + u * G;
      int o = off[0];
#pragma unroll
      for (int r = 1; r < 6; ++r) o = f >= pre[r] ? off[r] : o;
      const int j = f + o;
      jj[u] = j;
      if (f < total) c0[u] = vs.rec[2 * (base + j)];
    }
#pragma unroll
    for (int u = 0; u < kVF; ++u) {
      float ddx, ddy;
      if (f0 + u * G < total &&
          (kAll ? vision_offsets<true>(L, c0[u], &ddx, &ddy) : vision_near(L, c0[u])))
        hits[nh++][threadIdx.x] = jj[u];
    }
    if (__any(nh > kVisionHits - kVF)) {  // no room for kVF more: drain every lane's
      if (G <= 8)
        vision_drain_group<NB, G, kAll>(L, vp, vs.rec, base, hits, nh, acc);
      else
        vision_drain<NB, kAll>(L, vp, vs.rec, base, hits, nh, acc);
      nh = 0;
    }
  }
  if (G <= 8)
    vision_drain_group<NB, G, kAll>(L, vp, vs.rec, base, hits, nh, acc);
  else
    vision_drain<NB, kAll>(L, vp, vs.rec, base, hits, nh, acc);
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)acc[b], off, 64);
      const int32_t hi = __shfl_xor((int)(acc[b] >> 32), off, 64);
      acc[b] += (int64_t)(((uint64_t)(uint32_t)hi << 32) | lo);
    }
  }
  swarm::role_mark(va.rstamp, swarm::kMarkConeReduced);
  tail.template done<NB, G>(va, e, row, sub, acc, tail_pre);
}

template <int NB, int G, bool kAll = false>
__global__ __launch_bounds__(256) void k_vision(DevState st, const Derived* __restrict__ d,
                                                VisionArgs va, int xcd_bpe) {
  __shared__ uint32_t hits[kVisionHits][256];
  vision_body<NB, G, kAll>(st, d, va, blockIdx.x, xcd_bpe, hits);
}

// The vision cone and the rollout policy of its agents in one launch
// (swarm_engine_vision_policy): each agent's group computes its bins, writes
// the observable row and runs the MLP + sampling on them (PolicyTail).
template <int NB, int G, int D, int K>
__global__ __launch_bounds__(256) void k_vision_policy(DevState st, const Derived* __restrict__ d,
                                                       VisionArgs va, swarm::MlpArgs m,
                                                       int xcd_bpe) {
  __shared__ uint32_t hits[kVisionHits][256];
  const PolicyTail<D, K> tail{m};
  vision_body<NB, G, false, 256, PolicyTail<D, K>>(st, d, va, blockIdx.x, xcd_bpe, hits, tail);
}

// ------------------------------------------- build stages riding along
// Latency-bound engines (swarm_engine_defer_build): the next window's
// cluster decomposition does not fork onto a second stream; its three
// stages ride along in the slice's observable and policy launches instead,
// as extra workgroups of the same kernels (no graph fork/join edges, no
// launch of their own):
//   k_vgrid_sort     the vision grid's env workgroups + k_build_sort's
//   k_vision_pairs   the vision cone's blocks + k_build_pairs's
//   k_policy_cbuild  the policy's blocks (1024 threads) + k_cluster_build's
// Each stage needs the previous one complete, which the launch order on
// the engine stream guarantees.  The build's workgroups take the first block
// indices of each launch: the build chain (sort -> pairs -> cluster build)
// is the longer one, so its workgroups are dealt out first.
// Block index of a fused launch whose first `nfirst` roles are the build's
// (dealt out first).
__device__ __forceinline__ int fused_block(int nfirst) {
  (void)nfirst;
  return (int)blockIdx.x;
}

// The l1_pairs pair-search role of the slice's first launch: n_fb blocks
// per env of blockDim threads after the sort and grid workgroups
// (swarm::pair_filter_body; ctl: the device control block, whose window
// counter names this window's build sort).  smem: the launch's dynamic LDS,
// at least l1_role_lds_bytes() (the fallback cell search's tables).
using swarm::l1_role_lds_bytes;
__device__ __forceinline__ void l1_pairs_role(const Derived* __restrict__ d, const DevState& st,
                                              const Scratch& sc, int lxb, int lyb, int fb, int n_fb,
                                              const uint64_t* ctl, unsigned char* smem) {
  float* nb2 = reinterpret_cast<float*>(smem);
  int32_t* uf = reinterpret_cast<int32_t*>(smem) + kMaxSpecies * kMaxSpecies;
  swarm::role_begin(sc, swarm::kRolePairs);
  swarm::pair_filter_body(d, st, sc, lxb, lyb, fb % n_fb, fb / n_fb, ctl[swarm::kCtlWin] + 1ull,
                          nb2, uf);
  swarm::role_end(sc, swarm::kRolePairs);
}

template <int CH>
__global__ __launch_bounds__(1024) void k_vgrid_sort(DevState st, VisionArgs va, Scratch sc,
                                                     int lxb, int lyb, const Derived* __restrict__ d,
                                                     int n_fb, const uint64_t* __restrict__ ctl) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = fused_block(va.n_envs);
  const int E = va.n_envs;
  if (b >= 2 * E) {  // l1_pairs: the pair search beside the sort (n_fb > 0)
    l1_pairs_role(d, st, sc, lxb, lyb, b - 2 * E, n_fb, ctl, smem);
    return;
  }
  const int role = b < E ? swarm::kRoleSort : swarm::kRoleVgrid;
  swarm::role_begin(sc, role);
  if (b < E)
    swarm::build_sort_body<CH>(st, sc, lxb, lyb, b, smem, n_fb > 0 ? ctl[swarm::kCtlWin] + 1ull : 0ull);
  else
    vision_grid_body(st, va, b - E, smem);
  swarm::role_end(sc, role);
}

// The pair blocks come first: theirs is the longer chain (the cluster build
// waits on it), so they are dealt out before the cone blocks.
template <int NB, int G, bool kLocal>
__global__ __launch_bounds__(256) void k_vision_pairs(DevState st, const Derived* __restrict__ d,
                                                      VisionArgs va, int n_pblocks, Scratch sc,
                                                      int lxb, int lyb, int pair_bx) {
  __shared__ uint32_t hits[kVisionHits][256];
  __shared__ float nb2[swarm::kMaxSpecies * swarm::kMaxSpecies];
  __shared__ int32_t uf[2 * 256];
  const int b = fused_block(n_pblocks);
  const int role = b < n_pblocks ? swarm::kRolePairs : swarm::kRoleCone;
  swarm::role_begin(sc, role);
  if (b < n_pblocks) {
    swarm::build_pairs_body<kLocal>(d, st, sc, lxb, lyb, b % pair_bx, b / pair_bx, nb2, uf);
  } else {
    vision_body<NB, G, false>(st, d, va, b - n_pblocks, 0, hits);
  }
  swarm::role_end(sc, role);
}

// The same with the fused rollout policy on the cone side (PolicyTail): the
// pair blocks first, then the cone + MLP + sampling blocks.
template <int NB, int G, bool kLocal, int D, int K>
__global__ __launch_bounds__(256) void k_vision_policy_pairs(DevState st,
                                                             const Derived* __restrict__ d,
                                                             VisionArgs va, swarm::MlpArgs m,
                                                             int n_pblocks, Scratch sc, int lxb,
                                                             int lyb, int pair_bx) {
  __shared__ uint32_t hits[kVisionHits][256];
  __shared__ float nb2[swarm::kMaxSpecies * swarm::kMaxSpecies];
  __shared__ int32_t uf[2 * 256];
  const int b = fused_block(n_pblocks);
  const int role = b < n_pblocks ? swarm::kRolePairs : swarm::kRoleCone;
  swarm::role_begin(sc, role);
  if (b < n_pblocks) {
    swarm::build_pairs_body<kLocal>(d, st, sc, lxb, lyb, b % pair_bx, b / pair_bx, nb2, uf);
  } else {
    const PolicyTail<D, K> tail{m};
    vision_body<NB, G, false, 256, PolicyTail<D, K>>(st, d, va, b - n_pblocks, 0, hits, tail);
  }
  swarm::role_end(sc, role);
}

// l1_pairs slices: the pair list is ready when the cone runs, so the
// cluster build rides beside the cone + MLP + sampling (1024-thread blocks:
// the build's workgroup per env first, then the cone's, whose hit lists
// share the build's dynamic LDS).
template <int NB, int G, int D, int K>
__global__ __launch_bounds__(1024) void k_vision_policy_cbuild(DevState st,
                                                               const Derived* __restrict__ d,
                                                               VisionArgs va, swarm::MlpArgs m,
                                                               Scratch sc) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = fused_block(va.n_envs);
  const int role = b < va.n_envs ? swarm::kRoleCbuild : swarm::kRoleCone;
  swarm::role_begin(sc, role);
  if (b < va.n_envs) {
    swarm::cluster_build_env<false, true, false>(st, sc, b, smem, sc.gnpairs[b]);
  } else {
    auto* hits = reinterpret_cast<uint32_t(*)[1024]>(smem);
    // the actor's rows into LDS behind the hit lists before any group starts
    // (the groups' tails then read them at LDS latency, not L2's)
    float* sw = reinterpret_cast<float*>(smem + (size_t)kVisionHits * 1024 * sizeof(uint32_t));
    swarm::stage_mlp_rows<D, K>(m, sw);
    __syncthreads();
    const PolicyTail<D, K> tail{m, sw};
    vision_body<NB, G, false, 1024, PolicyTail<D, K>>(st, d, va, b - va.n_envs, 0, hits, tail);
  }
  swarm::role_end(sc, role);
}

template <int G, int D, int K>
__global__ __launch_bounds__(1024) void k_policy_cbuild(swarm::MlpArgs m, int n_envs,
                                                        DevState st, Scratch sc) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = fused_block(n_envs);
  const int role = b < n_envs ? swarm::kRoleCbuild : swarm::kRoleMlp;
  swarm::role_begin(sc, role);
  if (b < n_envs) {
    if (sc.local_uf)
      swarm::cluster_build_env<false, true, true>(st, sc, b, smem, sc.gnpairs[b]);
    else
      swarm::cluster_build_env<false, true, false>(st, sc, b, smem, sc.gnpairs[b]);
  } else {
    swarm::policy_body<G, D, K>(m, b - n_envs, reinterpret_cast<float*>(smem));
  }
  swarm::role_end(sc, role);
}

// ------------------------------------------- neighbour reductions (fp64)
// For the classical neighbour-rule agents (bechinger_models.py:156-171
// get_colloids_in_vision; lymburn_model.py:113-125): per agent i and every
// candidate j != i whose type bit is set in cand_mask, with d = x_j - x_i,
// |d| < range and (half_angle >= 0) acos(d/|d| . dir_i) < half_angle:
//   out[0] = count, out[1] = sum 1/(2 pi |d|), out[2..4] = sum d,
//   out[5] = sum |d|^2, out[6..8] = sum dir_j, out[9..11] = sum v_j.
// fp64 like the reference's numpy; candidates staged in LDS tiles.
constexpr int kNbOut = 12;

__global__ __launch_bounds__(256) void k_neighbor_reduce(
    const double* __restrict__ pos, const double* __restrict__ dir, const double* __restrict__ vel,
    const int32_t* __restrict__ types, int n, const int32_t* __restrict__ agents, int n_agents,
    uint32_t cand_mask, double range, double half_angle, double* __restrict__ out) {
  __shared__ double tp[256][3], td[256][3], tv[256][3];
  __shared__ int32_t tid_[256];
  const int e = blockIdx.y;
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = a < n_agents;
  const size_t base = (size_t)e * n;
  int i = -1;
  double xi[3] = {0.0, 0.0, 0.0}, mi[3] = {0.0, 0.0, 0.0};
  if (valid) {
    i = agents[a];
    for (int k = 0; k < 3; ++k) {
      xi[k] = pos[(base + i) * 3 + k];
      mi[k] = dir[(base + i) * 3 + k];
    }
  }
  double acc[kNbOut];
#pragma unroll
  for (int k = 0; k < kNbOut; ++k) acc[k] = 0.0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + (int)threadIdx.x;
    __syncthreads();
    if (j < n) {
      const bool ok = (cand_mask >> (types[j] & 31)) & 1u;
      tid_[threadIdx.x] = ok ? j : -1;
      for (int k = 0; k < 3; ++k) {
        tp[threadIdx.x][k] = pos[(base + j) * 3 + k];
        td[threadIdx.x][k] = dir[(base + j) * 3 + k];
        tv[threadIdx.x][k] = vel ? vel[(base + j) * 3 + k] : 0.0;
      }
    } else {
      tid_[threadIdx.x] = -1;
    }
    __syncthreads();
    if (!valid) continue;
    const int cn = min(256, n - j0);
    for (int c = 0; c < cn; ++c) {
      const int jj = tid_[c];
      if (jj < 0 || jj == i) continue;
      const double dx = tp[c][0] - xi[0], dy = tp[c][1] - xi[1], dz = tp[c][2] - xi[2];
      const double d2 = dx * dx + dy * dy + dz * dz;
      const double dn = sqrt(d2);
      if (!(dn < range)) continue;
      if (half_angle >= 0.0) {
        const double dot = (dx / dn) * mi[0] + (dy / dn) * mi[1] + (dz / dn) * mi[2];
        if (!(acos(dot) < half_angle)) continue;
      }
      acc[0] += 1.0;
      acc[1] += 1.0 / (2.0 * 3.14159265358979323846 * dn);
      acc[2] += dx;
      acc[3] += dy;
      acc[4] += dz;
      acc[5] += d2;
      acc[6] += td[c][0];
      acc[7] += td[c][1];
      acc[8] += td[c][2];
      acc[9] += tv[c][0];
      acc[10] += tv[c][1];
      acc[11] += tv[c][2];
    }
  }
  if (valid) {
    double* o = out + ((size_t)e * n_agents + a) * kNbOut;
#pragma unroll
    for (int k = 0; k < kNbOut; ++k) o[k] = acc[k];
  }
}

// ------------------------------------------------ pairwise field distances
// For ParticleSensing / SpeciesSearch (particle_sensing.py:95-121,
// species_search.py:97-130): d = || fp32(x_j) - fp32(x_i) || / L per agent
// i and sensed colloid j (unwrapped positions, no minimum image), written
// [E][mc][A] for sensed columns m0 .. m0 + mc - 1.  The sensed positions of
// the block's column tile are staged in LDS once and read by all agents.
__global__ __launch_bounds__(256) void k_pair_dist(DevState st, const double* __restrict__ box,
                                                   const int32_t* __restrict__ agents,
                                                   int n_agents,
                                                   const int32_t* __restrict__ sensed, int m0,
                                                   int mc, float b0, float b1, float b2,
                                                   float* __restrict__ out) {
  __shared__ float tile[256][3];
  const int e = blockIdx.z;
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = st.n;
  const size_t M = (size_t)st.m, base = (size_t)e * N;
  const double inv32 = 1.0 / 4294967296.0;
  float xi[3] = {0.0f, 0.0f, 0.0f};
  if (a < n_agents) {
    const size_t gi = base + agents[a];
    for (int k = 0; k < st.dims; ++k)
      xi[k] = (float)(((double)st.img[k * M + gi] + (double)st.q[k * M + gi] * inv32) * box[k]);
  }
  const int c0 = blockIdx.y * 256;
  const int cn = min(256, mc - c0);
  if (threadIdx.x < cn) {
    const size_t gj = base + sensed[m0 + c0 + threadIdx.x];
    tile[threadIdx.x][2] = 0.0f;
    for (int k = 0; k < st.dims; ++k)
      tile[threadIdx.x][k] =
          (float)(((double)st.img[k * M + gj] + (double)st.q[k * M + gj] * inv32) * box[k]);
  }
  __syncthreads();
  if (a >= n_agents) return;
  const size_t A = (size_t)n_agents;
  float* o = out + ((size_t)e * mc + c0) * A + a;
  for (int c = 0; c < cn; ++c) {
    const float dx = (tile[c][0] - xi[0]) / b0;
    const float dy = (tile[c][1] - xi[1]) / b1;
    const float dz = (tile[c][2] - xi[2]) / b2;
    o[(size_t)c * A] = swarm::sqrt_rn(dx * dx + dy * dy + dz * dz);
  }
}

// ------------------------------------------------------- field distance
struct FieldArgs {
  const double* box;
  const int32_t* agents;
  int n_agents;
  double s0, s1, s2;  // source
  double b0, b1, b2;  // box scale
  uint32_t* hq;
  int32_t* himg;
  float* d_cur;
  float* d_prev;
  int update, init_only, n_envs;
  int mode;  // 0: distances; 1: scale (f(d_cur) - f(d_prev)), f(d) = fa + fb d; 2: same, clipped at 0
  float fa, fb, fscale;
  float* out;
};

// Agent slot t (env-major) of k_field, or of a workgroup of k_field_vgrid_sort:
// everything the slot stores, computed first (field_compute) so that a
// workgroup that runs beside the window's check can hold its stores back
// (field_store) until the check's verdict.
struct FieldVal {
  float a, b;       // mode 0: d_cur, d_prev; else a: the transformed value
  uint32_t hq[3];   // the history update
  int32_t himg[3];
  bool live;
};
__device__ __forceinline__ FieldVal field_compute(const DevState& st, const FieldArgs& f, int t) {
  FieldVal v{};
  const int A = f.n_agents * f.n_envs;
  v.live = t < A;
  if (!v.live) return v;
  const int e = t / f.n_agents, ai = t - e * f.n_agents;
  const int N = st.n;
  const size_t M = (size_t)st.m;
  const size_t gi = (size_t)e * N + f.agents[ai];
  const double inv32 = 1.0 / 4294967296.0;
  if (!f.init_only) {
    const double src[3] = {f.s0 / f.b0, f.s1 / f.b1, f.s2 / f.b2};
    const double bs[3] = {f.b0, f.b1, f.b2};
    float cur[3], prev[3];
    for (int a = 0; a < 3; ++a) {
      double pc, hp;
      if (a < st.dims) {
        pc = ((double)st.img[a * M + gi] + (double)st.q[a * M + gi] * inv32) * f.box[a] / bs[a];
        hp = ((double)f.himg[(size_t)a * A + t] + (double)f.hq[(size_t)a * A + t] * inv32) *
             f.box[a] / bs[a];
      } else {
        pc = 0.0 / bs[a];
        hp = 0.0 / bs[a];
      }
      cur[a] = (float)(src[a] - pc);
      prev[a] = (float)(src[a] - hp);
    }
    const float dc = swarm::sqrt_rn(cur[0] * cur[0] + cur[1] * cur[1] + cur[2] * cur[2]);
    const float dp = swarm::sqrt_rn(prev[0] * prev[0] + prev[1] * prev[1] + prev[2] * prev[2]);
    if (f.mode == 0) {
      v.a = dc;
      v.b = dp;
    } else {
      // affine decay f(d) = fa + fb * d; value = scale * (f(d_cur) - f(d_prev))
      // (concentration_field.py:102-104); mode 2 clips at 0
      // (gradient_sensing.py:117-118; NaN propagates as in torch.clamp)
      const float fc = f.fa + f.fb * dc;
      const float fp = f.fa + f.fb * dp;
      float w = f.fscale * (fc - fp);
      if (f.mode == 2) w = w < 0.0f ? 0.0f : w;
      v.a = w;
    }
  }
  if (f.update || f.init_only) {
    for (int a = 0; a < 3; ++a) {
      v.hq[a] = a < st.dims ? st.q[a * M + gi] : 0u;
      v.himg[a] = a < st.dims ? st.img[a * M + gi] : 0;
    }
  }
  return v;
}
__device__ __forceinline__ void field_store(const FieldArgs& f, int t, const FieldVal& v) {
  if (!v.live) return;
  const int A = f.n_agents * f.n_envs;
  if (!f.init_only) {
    if (f.mode == 0) {
      f.d_cur[t] = v.a;
      f.d_prev[t] = v.b;
    } else {
      f.out[t] = v.a;
    }
  }
  if (f.update || f.init_only) {
    for (int a = 0; a < 3; ++a) {
      f.hq[(size_t)a * A + t] = v.hq[a];
      f.himg[(size_t)a * A + t] = v.himg[a];
    }
  }
}
__device__ __forceinline__ void field_body(const DevState& st, const FieldArgs& f, int t) {
  field_store(f, t, field_compute(st, f, t));
}

__global__ __launch_bounds__(256) void k_field(DevState st, FieldArgs f) {
  field_body(st, f, blockIdx.x * blockDim.x + threadIdx.x);
}

// The reward launch of a slice whose observable is a persistent vision
// cone (swarm_vision_cone_persistent) and whose next build is deferred:
// the field's agents, the NEXT observable's vision grid (from the positions
// the reward sees, which the observable will see too) and build stage 1,
// so the observable launch only runs the cone (beside stage 2).
// l1_pairs (n_fb > 0): the next window's pair search rides here too,
// n_fb blocks per env after the grid workgroups (l1_pairs_role).
// with_grid = 0 (a field observable, l1_pairs): no vision grid, the reward
// carries the sort and the pair search only (its grid workgroups return).
// CheckArgs (kCheck launches): the window's pending check rides here as
// well, one workgroup per env with the lowest block indices of the launch
// (swarm::check_body with k_check's arguments), and no other workgroup
// waits for it before it starts ("The check in the
// reward launch").  Every role runs at once on the state the run kernel
// left, reading no word a workgroup of this launch writes (the tag of the
// finished sort is the env's window number, vtag, with bit 63 set: never a
// window counter + 1 of the other launches; the pair counters were reset by
// the run launch), and publishing nothing that cannot be recomputed: the
// sort holds its global writes back (the check reads the last sort's
// output), the pair search takes the lists as usable and writes scratch
// only, the field role keeps its results in registers.  Then each waits for
// the env's verdict:
//  - kVerdictOk (a relaxed store, no fence on either side): the window
//    stands and its lists are usable; the held stores go out.
//  - kVerdictRedo: the check is about to change the state (an exact re-run)
//    or has (big clusters, which its workgroup integrates before the test),
//    or the lists are unusable.  Every role workgroup releases what it wrote
//    and arrives; the check workgroup, which waits for the last arrival
//    before it re-runs, then resets the pair counters and releases
//    kVerdictGo; the roles acquire and do their work again the way they
//    would after k_check.
struct CheckArgs {
  int n_steps;
  uint64_t* step_ctr;
  uint32_t* arrive;
  int lx, ly, cell_lx, cell_ly;
};
constexpr uint64_t kRideTag = 1ull << 63;

// The check workgroup of env e.  n_roles: the other workgroups of the launch
// that touch env e (each arrives once after kVerdictRedo).
__device__ __forceinline__ void ride_check_role(const Derived* __restrict__ d, const DevState& st,
                                                const Scratch& sc, int e, int E, int n_roles,
                                                const CheckArgs& ck, unsigned char* smem) {
  const bool big = sc.big_n[e] != 0;
  int outcome = 0;  // index into cstats: 0 speculated, 1 big clusters, 2 lists unusable, 3 re-run
  auto hook = [&](bool rerun, bool lists_ok) {
    outcome = rerun ? 3 : big ? 1 : lists_ok ? 0 : 2;
    if (outcome == 0) {
      swarm::verdict_publish(sc, e, swarm::kVerdictOk, false);
    } else {
      swarm::verdict_publish(sc, e, swarm::kVerdictRedo, false);
      swarm::verdict_arrivals(sc, e, n_roles);
    }
  };
  swarm::check_body(d, st, sc, e, E, ck.n_steps, ck.step_ctr, ck.arrive, ck.lx, ck.ly, 0,
                    ck.cell_lx, ck.cell_ly, smem, false, hook);
  if (threadIdx.x == 0) atomicAdd(&sc.cstats[outcome], 1ull);
  if (outcome != 0) {
    if (threadIdx.x == 0) {  // what the roles that ran ahead left behind
      sc.gnpairs[e] = 0;
      sc.gnx[e] = 0;
      __hip_atomic_store(&sc.varrive[e], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    swarm::verdict_publish(sc, e, swarm::kVerdictGo, true);
  }
}

struct RideSortHold {
  static constexpr bool kActive = true;
  const Scratch& sc;
  int e;
  uint64_t vt;
  __device__ __forceinline__ bool operator()() const {
    return swarm::verdict_poll(sc, e, vt) == swarm::kVerdictOk;
  }
};

template <int CH, bool kCheck = false>
__global__ __launch_bounds__(1024) void k_field_vgrid_sort(FieldArgs f, int n_fblocks, DevState st,
                                                           VisionArgs va, Scratch sc, int lxb,
                                                           int lyb, const Derived* __restrict__ d,
                                                           int n_fb, const uint64_t* __restrict__ ctl,
                                                           int with_grid, CheckArgs ck) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int E = va.n_envs, npb = n_fb * E;
  int b = fused_block(2 * va.n_envs);
  if (kCheck) {
    if (b < E) {
      // the field blocks with an agent slot of env b
      const int nA = f.n_agents, T = (int)blockDim.x;
      const int nfield = ((b + 1) * nA - 1) / T - (b * nA) / T + 1;
      ride_check_role(d, st, sc, b, E, 1 + (with_grid ? 1 : 0) + n_fb + nfield, ck, smem);
      return;
    }
    b -= E;
  }
  if (b >= 2 * E && b < 2 * E + npb) {
    if (kCheck) {
      const int fb = b - 2 * E, e = fb / n_fb;
      float* nb2 = reinterpret_cast<float*>(smem);
      int32_t* uf = reinterpret_cast<int32_t*>(smem) + kMaxSpecies * kMaxSpecies;
      const uint64_t vt = sc.vtag[e];  // (loaded beside the body's first loads)
      swarm::role_begin(sc, swarm::kRolePairs);
      uint64_t early = 0ull;
      swarm::pair_filter_body(d, st, sc, lxb, lyb, fb % n_fb, e, vt | kRideTag, nb2, uf, true,
                              &early);
      if (swarm::verdict_poll(sc, e, vt, swarm::kVerdictOk, early) == swarm::kVerdictOk) {
        if (fb % n_fb == 0 && threadIdx.x == 0) atomicAdd(&sc.stats[0], 1ull);
      } else {
        swarm::verdict_redo(sc, e, vt);
        swarm::pair_filter_body(d, st, sc, lxb, lyb, fb % n_fb, e, vt | kRideTag, nb2, uf);
      }
      swarm::role_end(sc, swarm::kRolePairs);
      return;
    }
    l1_pairs_role(d, st, sc, lxb, lyb, b - 2 * E, n_fb, ctl, smem);
    return;
  }
  if (!with_grid && b >= E && b < 2 * E) return;
  const int role = b < E ? swarm::kRoleSort : b < 2 * E ? swarm::kRoleVgrid : swarm::kRoleField;
  const int ft0 = (b - 2 * E - npb) * (int)blockDim.x;  // field role: first agent slot
  if (kCheck) {
    if (b < 2 * E) {
      const int e = b < E ? b : b - E;
      const uint64_t vt = sc.vtag[e];
      swarm::role_begin(sc, role);
      bool done;
      if (b < E) {
        done = swarm::build_sort_body<CH, RideSortHold>(st, sc, lxb, lyb, e, smem, 0ull,
                                                        RideSortHold{sc, e, vt});
      } else {
        vision_grid_body(st, va, e, smem);
        done = swarm::verdict_poll(sc, e, vt) == swarm::kVerdictOk;
      }
      if (!done) {
        swarm::verdict_redo(sc, e, vt);
        if (b < E)
          swarm::build_sort_body<CH>(st, sc, lxb, lyb, e, smem, n_fb > 0 ? vt | kRideTag : 0ull);
        else
          vision_grid_body(st, va, e, smem);
      }
      swarm::role_end(sc, role);
      return;
    }
    // the field role: every env with an agent slot in this block
    const int A = f.n_agents * f.n_envs;
    const int e0 = min(ft0, A - 1) / f.n_agents;
    const int e1 = min(ft0 + (int)blockDim.x - 1, A - 1) / f.n_agents;
    swarm::role_begin(sc, role);
    FieldVal v = field_compute(st, f, ft0 + (int)threadIdx.x);
    bool redo = false;
    for (int e = e0; e <= e1; ++e)
      if (swarm::verdict_poll(sc, e, sc.vtag[e]) != swarm::kVerdictOk) redo = true;
    if (redo) {
      // every arrival first (nothing of this block is stored yet), then the
      // waits: the block waits for nothing while it owes an arrival
      __syncthreads();
      if (threadIdx.x == 0)
        for (int e = e0; e <= e1; ++e)
          if (swarm::verdict_poll(sc, e, sc.vtag[e]) != swarm::kVerdictOk)
            __hip_atomic_fetch_add(&sc.varrive[e], 1ull, __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      for (int e = e0; e <= e1; ++e)
        if (swarm::verdict_poll(sc, e, sc.vtag[e]) != swarm::kVerdictOk)
          swarm::verdict_acquire(sc, e, sc.vtag[e], swarm::kVerdictGo);
      v = field_compute(st, f, ft0 + (int)threadIdx.x);
    }
    field_store(f, ft0 + (int)threadIdx.x, v);
    swarm::role_end(sc, role);
    return;
  }
  swarm::role_begin(sc, role);
  if (b < E)
    swarm::build_sort_body<CH>(st, sc, lxb, lyb, b, smem, n_fb > 0 ? ctl[swarm::kCtlWin] + 1ull : 0ull);
  else if (b < 2 * E)
    vision_grid_body(st, va, b - E, smem);
  else
    field_body(st, f, ft0 + (int)threadIdx.x);
  swarm::role_end(sc, role);
}

// --------------------------------------------------------- pair listing
__global__ __launch_bounds__(256) void k_pairs(DevState st, const Derived* __restrict__ d,
                                               int env, float cut2, int lx, int ly,
                                               const int32_t* __restrict__ start,
                                               const int32_t* __restrict__ order,
                                               int32_t* __restrict__ pairs, int max_pairs,
                                               int32_t* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = st.n;
  if (i >= N) return;
  const size_t M = (size_t)st.m;
  const size_t gi = (size_t)env * N + i;
  const uint32_t qxi = st.q[gi], qyi = st.q[M + gi];
  const int ncell = 1 << (lx + ly);
  const int ncx = 1 << lx, ncy = 1 << ly;
  const int lox = ncx >= 3 ? -1 : 0, hix = ncx >= 3 ? 1 : ncx - 1;
  const int loy = ncy >= 3 ? -1 : 0, hiy = ncy >= 3 ? 1 : ncy - 1;
  const int cc0 = cell_index(qxi, qyi, lx, ly);
  const int cx = cc0 & (ncx - 1), cy = cc0 >> lx;
  const int32_t* so = start + (size_t)env * (ncell + 1);
  const int32_t* oo = order + (size_t)env * N;
  for (int oy = loy; oy <= hiy; ++oy) {
    const int y = (cy + oy + ncy) & (ncy - 1);
    for (int ox = lox; ox <= hix; ++ox) {
      const int x = (cx + ox + ncx) & (ncx - 1);
      const int cc = (y << lx) | x;
      for (int jj = so[cc]; jj < so[cc + 1]; ++jj) {
        const int j = oo[jj];
        if (j <= i) continue;
        const size_t gj = (size_t)env * N + j;
        // minimum image in a periodic box, else the unwrapped difference
        // (the grid search wraps either way: a pair within cutoff < L / 2 is
        // within it by the minimum image too)
        const bool per = d->periodic != 0;
        const float rx = swarm::pair_disp(st.q[gj], st.img[gj], qxi, st.img[gi], d->sx[0], per);
        const float ry = swarm::pair_disp(st.q[M + gj], st.img[M + gj], qyi, st.img[M + gi], d->sx[1], per);
        if (rx * rx + ry * ry < cut2) {
          const int slot = atomicAdd(count, 1);
          if (slot < max_pairs) {
            pairs[2 * slot] = i;
            pairs[2 * slot + 1] = j;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------- trajectory ring
// One trajectory entry of env `env` (espresso.py:1110-1130: the state at a
// write point) into slot count % cap of a host-pinned, device-mapped ring:
// the step counter, then q[D][N], img[D][N], ang[N] (2-D) or dir3[3][N]
// (3-D), vel[D][N].  The slot comes from a device counter, so captured
// graphs record into successive slots on every replay; k_traj_bump
// publishes the count after the entry is complete (stream order).
__global__ __launch_bounds__(256) void k_traj_write(DevState st, int env,
                                                    unsigned char* __restrict__ ring, int cap,
                                                    size_t entry_bytes,
                                                    const uint64_t* __restrict__ count,
                                                    const uint64_t* __restrict__ ctl) {
  const int N = st.n, D = st.dims;
  const size_t M = (size_t)st.m;
  const uint64_t slot = *count % (uint64_t)cap;
  unsigned char* ent = ring + 64 + slot * entry_bytes;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *reinterpret_cast<uint64_t*>(ent) = ctl[0];
  if (i >= N) return;
  const size_t gi = (size_t)env * N + i;
  uint32_t* w = reinterpret_cast<uint32_t*>(ent + 8);
  for (int a = 0; a < D; ++a) w[(size_t)a * N + i] = st.q[a * M + gi];
  w += (size_t)D * N;
  for (int a = 0; a < D; ++a) w[(size_t)a * N + i] = (uint32_t)st.img[a * M + gi];
  w += (size_t)D * N;
  if (D == 3) {
    float* f = reinterpret_cast<float*>(w);
    for (int a = 0; a < 3; ++a) f[(size_t)a * N + i] = st.dir3[a * M + gi];
    w += (size_t)3 * N;
  } else {
    w[i] = st.ang[gi];
    w += N;
  }
  float* v = reinterpret_cast<float*>(w);
  for (int a = 0; a < D; ++a) v[(size_t)a * N + i] = st.vel[a * M + gi];
}

__global__ void k_traj_bump(uint64_t* __restrict__ count, unsigned char* __restrict__ ring) {
  if (threadIdx.x == 0) {
    const uint64_t c = *count + 1;
    *count = c;
    __threadfence_system();
    *reinterpret_cast<volatile uint64_t*>(ring) = c;
  }
}

}  // namespace
