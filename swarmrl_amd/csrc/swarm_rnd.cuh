// swarm_rnd.cuh -- Random Network Distillation distance in one launch.
//
// The C5 workload's intrinsic reward (swarmrl/intrinsic_reward/
// random_network_distillation.py:126-143 with rnd_configs.py:17-38): per
// observation x, the fixed random target network and the trained predictor,
// both Dense(W) -> ReLU -> Dense(W) -> ReLU -> Dense(W), and the ZnNL
// OrderNDifference metric (sum_k |t_k - p_k|^order)^(1/order).  The torch
// forward of the two networks is six GEMMs and their epilogues (~20 small
// launches per slice, ~110 us at 16384 agents); here one thread per
// observation runs both networks from LDS-staged weights (torch Linear
// layouts, read in place) and reduces the metric.  fp32, checked against the
// torch networks within a stated tolerance (tests/test_gpu_rnd.py).
//
// Second half of the file: the predictor's training (k_rnd_targets,
// k_rnd_train; tests/test_gpu_rnd_train.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace swarm {

constexpr int kRndWidth = 32;   // rnd_configs.py:17-38 (Dense(32) x 3)
constexpr int kRndMaxIn = 16;

// The six parameter tensors of one network: w1, b1, w2, b2, w3, b3.
struct RndPtrs {
  const float* w[6];
};

// One network's weights in LDS: w1 [W][D], b1, and the square layers
// transposed (w2t[k][j] = w2[j][k]) so that one input k feeds a row of W
// outputs read as float4 broadcasts.
template <int D>
struct RndNet {
  float w1[kRndWidth][D];
  float b1[kRndWidth];
  float4 w2t[kRndWidth][kRndWidth / 4];
  float b2[kRndWidth];
  float4 w3t[kRndWidth][kRndWidth / 4];
  float b3[kRndWidth];
};

template <int D>
__device__ __forceinline__ void rnd_stage(RndNet<D>* net, const float* const* w, int d_in) {
  constexpr int W = kRndWidth;
  for (int k = threadIdx.x; k < W * D; k += blockDim.x) {
    const int j = k / D, i = k - j * D;
    net->w1[j][i] = i < d_in ? w[0][j * d_in + i] : 0.0f;
  }
  float* w2t = reinterpret_cast<float*>(net->w2t);
  float* w3t = reinterpret_cast<float*>(net->w3t);
  for (int k = threadIdx.x; k < W * W; k += blockDim.x) {
    const int j = k / W, i = k - j * W;  // torch w[j][i] (out j, in i)
    w2t[i * W + j] = w[2][k];
    w3t[i * W + j] = w[4][k];
  }
  for (int k = threadIdx.x; k < W; k += blockDim.x) {
    net->b1[k] = w[1][k];
    net->b2[k] = w[3][k];
    net->b3[k] = w[5][k];
  }
}

// a[j] = b[j] + sum_k wt[k][j] h[k] with h from the thread's LDS column
// (hb[k][tid]); k in order, one float4 row broadcast at a time.
__device__ __forceinline__ void rnd_square(const float4 (*wt)[kRndWidth / 4], const float* b,
                                           const float (*hb)[256], float* a) {
  constexpr int W = kRndWidth;
#pragma unroll
  for (int j = 0; j < W; ++j) a[j] = b[j];
#pragma unroll 2
  for (int k = 0; k < W; ++k) {
    const float hk = hb[k][threadIdx.x];
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      const float4 r = wt[k][q];
      a[4 * q + 0] = __builtin_fmaf(r.x, hk, a[4 * q + 0]);
      a[4 * q + 1] = __builtin_fmaf(r.y, hk, a[4 * q + 1]);
      a[4 * q + 2] = __builtin_fmaf(r.z, hk, a[4 * q + 2]);
      a[4 * q + 3] = __builtin_fmaf(r.w, hk, a[4 * q + 3]);
    }
  }
}

// Output layer of one network for one observation (x in registers).
template <int D>
__device__ __forceinline__ void rnd_forward(const RndNet<D>& net, const float* x,
                                            float (*hb)[256], float* out) {
  constexpr int W = kRndWidth;
  float a[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    float v = net.b1[j];
#pragma unroll
    for (int i = 0; i < D; ++i) v = __builtin_fmaf(net.w1[j][i], x[i], v);
    a[j] = v;
  }
#pragma unroll
  for (int j = 0; j < W; ++j) hb[j][threadIdx.x] = fmaxf(a[j], 0.0f);
  rnd_square(net.w2t, net.b2, hb, a);
#pragma unroll
  for (int j = 0; j < W; ++j) hb[j][threadIdx.x] = fmaxf(a[j], 0.0f);
  rnd_square(net.w3t, net.b3, hb, out);
}

// The metric of observation a (both networks from the block's LDS copies).
template <int D>
__device__ __forceinline__ float rnd_metric(const RndNet<D>& tnet, const RndNet<D>& pnet,
                                            const float* __restrict__ x, int a, int d_in,
                                            int order, float (*hb)[256]) {
  constexpr int W = kRndWidth;
  float xi[D];
#pragma unroll
  for (int i = 0; i < D; ++i) xi[i] = i < d_in ? x[(size_t)a * d_in + i] : 0.0f;
  float t[W], p[W];
  rnd_forward<D>(tnet, xi, hb, t);
  rnd_forward<D>(pnet, xi, hb, p);
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const float dlt = fabsf(t[j] - p[j]);
    acc += order == 2 ? dlt * dlt : powf(dlt, (float)order);
  }
  return order == 2 ? sqrtf(acc) : powf(acc, 1.0f / (float)order);
}

template <int D>
__global__ __launch_bounds__(256) void k_rnd_distance(const float* __restrict__ x, int n,
                                                      int d_in, RndPtrs tp, RndPtrs pp,
                                                      int order, float* __restrict__ out) {
  __shared__ RndNet<D> tnet, pnet;
  __shared__ float hb[kRndWidth][256];  // the thread's hidden activations (column tid)
  rnd_stage<D>(&tnet, tp.w, d_in);
  rnd_stage<D>(&pnet, pp.w, d_in);
  __syncthreads();
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;  // no barrier below
  out[a] = rnd_metric<D>(tnet, pnet, x, a, d_in, order, hb);
}

// The per-env intrinsic reward (random_network_distillation.py:126-143 on
// the device path: the mean metric of the env's latest observations,
// clipped) added to the task reward, in ONE launch instead of the metric
// kernel + torch's mean, clamp and add (five launches and a copy on C5's
// critical path).  Grid E x kb blocks of 256 threads, eight lanes per
// observation (32 a block): lane `sub` of a group computes outputs
// 4 sub .. 4 sub + 3 of every layer (each output's sum over its inputs in
// order, as rnd_forward), the group's hidden activations go through an LDS
// row (one wave's group: wave-scope ordering only), and the group adds its
// lanes' parts of the metric with xor-shuffles.  Each block writes its fp64
// partial sum (fixed order); the last block of an env (a ticket) adds the
// env's partials in a fixed tree, takes the mean, clips it and writes
// rewards[e][a] = base[e][a] + r_e (base null: r_e).  Deterministic: the
// same bits on every call and device.
constexpr int kRndLanes = 8;                      // lanes per observation
constexpr int kRndObsPerBlock = 256 / kRndLanes;  // 32
constexpr int kRndOut = kRndWidth / kRndLanes;    // outputs per lane and layer

// One network's weights in LDS, torch layouts (rows = outputs), the square
// layers' rows padded to kRndStride floats: lane `sub` of a group takes the
// outputs j = sub + 8 r, so the eight lanes of a group read rows 8 r .. 8 r
// + 7 together, which start 36 floats (= 36 banks mod 64) apart and cover
// disjoint bank quads -- no LDS bank conflict (unpadded rows 4 apart put all
// eight in one quad: an 8-way conflict on every float4 read).
constexpr int kRndStride = kRndWidth + 4;  // floats per padded row (16-B aligned)
template <int D>
struct RndRows {
  float w1[kRndWidth][D];
  float b1[kRndWidth];
  float4 w2[kRndWidth][kRndStride / 4];
  float b2[kRndWidth];
  float4 w3[kRndWidth][kRndStride / 4];
  float b3[kRndWidth];
};

// Both networks' weights into LDS (torch layouts, w1 zero-padded to D
// inputs).  Every load of the block's share of BOTH networks is issued
// before any LDS store: one memory latency (a load -> store -> load chain
// per loop trip took ~14 us per workgroup, SQ_WAIT_ANY 62 % of its wave
// cycles).  blockDim = 256.
template <int D>
__device__ __forceinline__ void rnd_stage_rows(RndRows<D>* tnet, RndRows<D>* pnet,
                                               const float* const* tw, const float* const* pw,
                                               int d_in) {
  constexpr int W = kRndWidth, T = 256;
  constexpr int N1 = (W * D + T - 1) / T, N2 = W * W / T;
  const int tid = threadIdx.x;
  RndRows<D>* nets[2] = {tnet, pnet};
  const float* const* ws[2] = {tw, pw};
  float v1[2][N1], v2[2][N2], v3[2][N2], bb[2][3];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const float* const* w = ws[n];
#pragma unroll
    for (int u = 0; u < N1; ++u) {
      const int k = tid + u * T, j = k / D, i = k - j * D;
      v1[n][u] = k < W * D && i < d_in ? w[0][j * d_in + i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < N2; ++u) {
      v2[n][u] = w[2][tid + u * T];
      v3[n][u] = w[4][tid + u * T];
    }
    if (tid < W) {
      bb[n][0] = w[1][tid];
      bb[n][1] = w[3][tid];
      bb[n][2] = w[5][tid];
    }
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    RndRows<D>* net = nets[n];
#pragma unroll
    for (int u = 0; u < N1; ++u) {
      const int k = tid + u * T;
      if (k < W * D) net->w1[k / D][k % D] = v1[n][u];
    }
    float* w2 = reinterpret_cast<float*>(net->w2);
    float* w3 = reinterpret_cast<float*>(net->w3);
#pragma unroll
    for (int u = 0; u < N2; ++u) {
      const int t = tid + u * T, j = t / W, c = t - j * W;
      w2[j * kRndStride + c] = v2[n][u];
      w3[j * kRndStride + c] = v3[n][u];
    }
    if (tid < W) {
      net->b1[tid] = bb[n][0];
      net->b2[tid] = bb[n][1];
      net->b3[tid] = bb[n][2];
    }
  }
}

// A square layer: the lane's outputs j = sub + 8 r, a[r] = b[j] + sum_k
// w[j][k] h[k] over the group's activations h (LDS row, float4 reads).
__device__ __forceinline__ void rnd_square_lanes(const float4 (*w)[kRndStride / 4], const float* b,
                                                 const float4* h, int sub, float* a) {
#pragma unroll
  for (int r = 0; r < kRndOut; ++r) a[r] = b[sub + kRndLanes * r];
#pragma unroll
  for (int q = 0; q < kRndWidth / 4; ++q) {
    const float4 hv = h[q];
#pragma unroll
    for (int r = 0; r < kRndOut; ++r) {
      const float4 wv = w[sub + kRndLanes * r][q];
      a[r] = __builtin_fmaf(wv.x, hv.x, a[r]);
      a[r] = __builtin_fmaf(wv.y, hv.y, a[r]);
      a[r] = __builtin_fmaf(wv.z, hv.z, a[r]);
      a[r] = __builtin_fmaf(wv.w, hv.w, a[r]);
    }
  }
}

// The lane's four outputs of one network for the group's observation x;
// row: the group's LDS activation row (kRndStride floats, float4-aligned).
template <int D>
__device__ __forceinline__ void rnd_forward_lanes(const RndRows<D>& net, const float* x, int sub,
                                                  float* row, float* out) {
  float a[kRndOut];
#pragma unroll
  for (int r = 0; r < kRndOut; ++r) {
    const int j = sub + kRndLanes * r;
    float v = net.b1[j];
#pragma unroll
    for (int i = 0; i < D; ++i) v = __builtin_fmaf(net.w1[j][i], x[i], v);
    a[r] = fmaxf(v, 0.0f);
  }
  auto publish = [&](const float* v) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the group's previous reads of the row are done
#pragma unroll
    for (int r = 0; r < kRndOut; ++r) row[sub + kRndLanes * r] = v[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const float4* h = reinterpret_cast<const float4*>(row);
  publish(a);
  rnd_square_lanes(net.w2, net.b2, h, sub, a);
#pragma unroll
  for (int r = 0; r < kRndOut; ++r) a[r] = fmaxf(a[r], 0.0f);
  publish(a);
  rnd_square_lanes(net.w3, net.b3, h, sub, out);
}

template <int D>
__global__ __launch_bounds__(256) void k_rnd_env(const float* __restrict__ x, int per_env,
                                                 int d_in, RndPtrs tp, RndPtrs pp, int order,
                                                 int clip, float lo, float hi,
                                                 const float* __restrict__ base,
                                                 float* __restrict__ metric,
                                                 float* __restrict__ env_reward,
                                                 float* __restrict__ rewards,
                                                 double* __restrict__ partial,
                                                 uint32_t* __restrict__ tickets) {
  static_assert(kRndOut == 4, "float4 activation rows");
  __shared__ RndRows<D> tnet, pnet;
  __shared__ __align__(16) float rows[kRndObsPerBlock][kRndStride];
  __shared__ double red[256];
  __shared__ int last;
  const int e = blockIdx.y, kb = gridDim.x, tid = threadIdx.x;
  const int sub = tid & (kRndLanes - 1), grp = tid / kRndLanes;
  rnd_stage_rows<D>(&tnet, &pnet, tp.w, pp.w, d_in);
  __syncthreads();
  // the block's groups of 32 observations (blockIdx.x, + gridDim.x, ...):
  // the networks are staged once per block, not once per 32 observations;
  // each group's metric sum in a fixed order per thread
  double own = 0.0;
  for (int k0 = blockIdx.x * kRndObsPerBlock; k0 < per_env; k0 += kb * kRndObsPerBlock) {
    const int k = k0 + grp;
    const bool valid = k < per_env;
    const size_t a = (size_t)e * per_env + (valid ? k : 0);
    float xi[D];
#pragma unroll
    for (int i = 0; i < D; ++i) xi[i] = i < d_in ? x[a * d_in + i] : 0.0f;
    float t[kRndOut], p[kRndOut];
    rnd_forward_lanes<D>(tnet, xi, sub, rows[grp], t);
    rnd_forward_lanes<D>(pnet, xi, sub, rows[grp], p);
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < kRndOut; ++r) {
      const float dlt = fabsf(t[r] - p[r]);
      acc += order == 2 ? dlt * dlt : powf(dlt, (float)order);
    }
#pragma unroll
    for (int o = 1; o < kRndLanes; o <<= 1) acc += __shfl_xor(acc, o, 64);
    const float m = order == 2 ? sqrtf(acc) : powf(acc, 1.0f / (float)order);
    if (valid && sub == 0) {
      metric[a] = m;
      own += (double)m;
    }
  }
  // the block's sum: fixed tree over its threads
  red[tid] = own;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  double* pe = partial + (size_t)e * kb;
  if (tid == 0) {
    // the partial by a returning agent-scope atomic, waited for before the
    // ticket counts it (no __threadfence: an agent-scope release writes the
    // L2 back, ~0.1 us per block and a stall for every kernel beside it --
    // this launch took 51 us beside C5's build instead of ~20)
    __hip_atomic_exchange(reinterpret_cast<unsigned long long*>(pe + blockIdx.x),
                          (unsigned long long)__double_as_longlong(red[0]), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);
    last = atomicAdd(&tickets[e], 1u) == (uint32_t)(kb - 1);
  }
  __syncthreads();
  if (!last) return;
  // the env's last block: its partials in a fixed tree (kb <= 256 x 16 per
  // thread), read by agent-scope atomic loads
  double v = 0.0;
  for (int b = tid; b < kb; b += 256)
    v += __hip_atomic_load(&pe[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  red[tid] = v;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  float r = (float)(red[0] / (double)per_env);
  if (clip) r = fminf(fmaxf(r, lo), hi);
  if (tid == 0) {
    env_reward[e] = r;
    tickets[e] = 0u;  // the next call's count (graph replays)
  }
  for (int q = tid; q < per_env; q += 256) {
    const size_t g = (size_t)e * per_env + q;
    rewards[g] = base ? base[g] + r : r;
  }
}

// ---------------------------------------------------------------------------
// Training the predictor (swarmrl/intrinsic_reward/
// random_network_distillation.py:102-123: ZnNL SimpleTraining.train_model
// with MeanPowerLoss(order) and optax.adam, restated in torch by
// RNDReward.update): per epoch one permutation of the n observations, cut
// into minibatches of B; per minibatch the predictor's forward, the loss
// mean(|pred - y|^order), its gradient and one Adam step.  The steps are a
// serial chain (each reads the weights the previous one wrote), so the
// kernels below do the one thing that helps: they keep the chain on chip.

// y[a][32] = target(x[a]) for every observation: one thread per observation,
// the target network staged in LDS, each output's sum in rnd_forward's order.
template <int D>
__global__ __launch_bounds__(256) void k_rnd_targets(const float* __restrict__ x, int n, int d_in,
                                                     RndPtrs tp, float* __restrict__ y) {
  constexpr int W = kRndWidth;
  __shared__ RndNet<D> tnet;
  __shared__ float hb[kRndWidth][256];
  rnd_stage<D>(&tnet, tp.w, d_in);
  __syncthreads();
  const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= (size_t)n) return;  // no barrier below
  float xi[D];
#pragma unroll
  for (int i = 0; i < D; ++i) xi[i] = i < d_in ? x[a * d_in + i] : 0.0f;
  float t[W];
  rnd_forward<D>(tnet, xi, hb, t);
  float4* o = reinterpret_cast<float4*>(y + a * W);
#pragma unroll
  for (int q = 0; q < W / 4; ++q)
    o[q] = make_float4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
}

// Minibatch steps [s0, s1) of one epoch in ONE workgroup of 256 threads.
//
// Resident for the whole launch: the predictor's six tensors in LDS (the
// square layers' rows padded to kRndStride = 36 floats as in k_rnd_env: the
// forward's float4 reads along the rows of 16 lanes and the backward's reads
// down a column are both free of bank conflicts; w1's rows padded to 17),
// and in the registers of the thread that owns each element the
// parameter and its two Adam moments (element e of a tensor belongs to
// thread e mod 256: at most 2 + 4 + 4 + 1 elements a thread).  They are read
// from torch's tensors at the start and written back in place, with the
// step counts, at the end.
//
// A step, R = ceil(B / 8) rows per thread (thread = row group g = tid / 32,
// unit l = tid % 32; rows b = g + 8 r):
//   1-3  forward, one output (b, l) per thread and row, k in order;
//        dP = dloss / dpred (zero for the rows past a short batch)
//   4    dz2 = (dP W3) [z2 > 0];  gW3 = dP^T h2, gb3;  Adam on w3, b3
//   5    dz1 = (dz2 W2) [z1 > 0]; gW2 = dz2^T h1, gb2; Adam on w2, b2
//   6    gW1 = dz1^T x, gb1;      Adam on w1, b1
// with one barrier after each.  Every sum over the batch runs b = 0, 1, ...
// in order and every sum over the units k = 0, 1, ... in order, in fp32
// fused multiply-adds; no atomics: the same bits on every run.  A layer's
// new weights go to LDS one phase after its Adam step, once no thread reads
// the old ones any more.
//
// The gather perm -> x[idx], y[idx] is off the chain: during step s the
// indices of step s + 2 and the rows of step s + 1 are in flight (the rows
// of x through a two-slot LDS ring, the thread's own targets y[idx[b]][l] in
// registers), issued at the top of the step and first touched at its end.
//
// Adam as swarm_ppo_epoch_step states it (torch's capturable Adam): step + 1,
// m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr / (1 - b1^step) *
// m / (sqrt(v) / sqrt(1 - b2^step) + eps), fp32; beta^step as exp2(step *
// log2 beta) and the two quotients as reciprocals (v_rcp_f32 / v_sqrt_f32,
// 1 ulp): a few ulp of a term that is lr times smaller than the parameter.
struct RndTrainArgs {
  float lr, beta1, beta2, eps;
  float log2_beta1, log2_beta2;
  float* param[6];
  float* m[6];
  float* v[6];
  float* step[6];
};

constexpr int kRndW1Stride = kRndMaxIn + 1;   // 17
constexpr int kRndMaxBatch = 64;

struct RndBias {
  float step_size, rsqrt_bc2;
};

__device__ __forceinline__ RndBias rnd_bias(const RndTrainArgs& a, float step) {
  const float bc1 = 1.0f - exp2f(step * a.log2_beta1);
  const float bc2 = 1.0f - exp2f(step * a.log2_beta2);
  RndBias r;
  r.step_size = a.lr * __builtin_amdgcn_rcpf(bc1);
  r.rsqrt_bc2 = __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(bc2));
  return r;
}

__device__ __forceinline__ void rnd_adam(const RndTrainArgs& a, const RndBias& bc, float g,
                                         float& p, float& m, float& v) {
  m = a.beta1 * m + (1.0f - a.beta1) * g;
  v = a.beta2 * v + (1.0f - a.beta2) * g * g;
  const float denom = __builtin_amdgcn_sqrtf(v) * bc.rsqrt_bc2 + a.eps;
  p = p - bc.step_size * (m * __builtin_amdgcn_rcpf(denom));
}

// |d|^(order - 1) for an integer order >= 1 by squaring (order 2: |d|).
__device__ __forceinline__ float rnd_powi(float a, int e) {
  float r = 1.0f;
  while (e > 0) {
    if (e & 1) r *= a;
    a *= a;
    e >>= 1;
  }
  return r;
}

// acc[r] += sum_k w[k] h[g + 8 r][k], k in order: the unit's weight row and
// the rows' activations as float4 reads (the activations a broadcast).
template <int R>
__device__ __forceinline__ void rnd_rows_dot(const float* wrow, const float (*h)[kRndWidth],
                                             int g, float* acc) {
#pragma unroll
  for (int q = 0; q < kRndWidth / 4; ++q) {
    const float4 wv = reinterpret_cast<const float4*>(wrow)[q];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 hv = reinterpret_cast<const float4*>(h[g + 8 * r])[q];
      acc[r] = __builtin_fmaf(wv.x, hv.x, acc[r]);
      acc[r] = __builtin_fmaf(wv.y, hv.y, acc[r]);
      acc[r] = __builtin_fmaf(wv.z, hv.z, acc[r]);
      acc[r] = __builtin_fmaf(wv.w, hv.w, acc[r]);
    }
  }
}

// acc[r] += sum_j d[g + 8 r][j] w[j][l], j in order: the unit's weight column
// (wcol = &w[0][l], rows kRndStride apart) and the rows' gradients as float4.
template <int R>
__device__ __forceinline__ void rnd_cols_dot(const float* wcol, const float (*d)[kRndWidth],
                                             int g, float* acc) {
#pragma unroll
  for (int q = 0; q < kRndWidth / 4; ++q) {
    const float w0 = wcol[(4 * q + 0) * kRndStride], w1 = wcol[(4 * q + 1) * kRndStride];
    const float w2 = wcol[(4 * q + 2) * kRndStride], w3 = wcol[(4 * q + 3) * kRndStride];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 dv = reinterpret_cast<const float4*>(d[g + 8 * r])[q];
      acc[r] = __builtin_fmaf(dv.x, w0, acc[r]);
      acc[r] = __builtin_fmaf(dv.y, w1, acc[r]);
      acc[r] = __builtin_fmaf(dv.z, w2, acc[r]);
      acc[r] = __builtin_fmaf(dv.w, w3, acc[r]);
    }
  }
}

// One wave per SIMD by construction (one workgroup of four waves): the whole
// register file is the wave's, so the R = 8 variant never spills to scratch.
template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_rnd_train(
    const float* __restrict__ x, const float* __restrict__ y, const long long* __restrict__ perm,
    int n, int d_in, int B, int order, int s0, int s1, RndTrainArgs a,
    float* __restrict__ loss_out) {
  constexpr int W = kRndWidth, NB = 8 * R, S1 = kRndW1Stride, S = kRndStride;
  __shared__ __align__(16) float w2s[W * S], w3s[W * S];
  __shared__ __align__(16) float h1[NB][W], h2[NB][W], dP[NB][W], dz2[NB][W], dz1[NB][W];
  __shared__ float w1s[W * S1], b1s[W], b2s[W], b3s[W];
  __shared__ float xs[2][NB][kRndMaxIn];
  float(*lbuf)[W] = dz1;  // the step's |d|^order terms (phases 3-4; dz1 lives in 5-6)
  const int tid = threadIdx.x, g = tid >> 5, l = tid & 31;

  // --- the thread's own elements: parameter and moments in registers
  float p1[2], m1[2], v1[2], p2[4], m2[4], v2[4], p3[4], m3[4], v3[4];
  float pb = 0.0f, mb = 0.0f, vb = 0.0f;
  int j1[2], i1[2];
  const int n1 = W * d_in;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = tid + 256 * u;
    const bool own = e < n1;
    j1[u] = own ? e / d_in : 0;
    i1[u] = own ? e - j1[u] * d_in : 0;
    p1[u] = own ? a.param[0][e] : 0.0f;
    m1[u] = own ? a.m[0][e] : 0.0f;
    v1[u] = own ? a.v[0][e] : 0.0f;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid + 256 * u;
    p2[u] = a.param[2][e];
    m2[u] = a.m[2][e];
    v2[u] = a.v[2][e];
    p3[u] = a.param[4][e];
    m3[u] = a.m[4][e];
    v3[u] = a.v[4][e];
  }
  const int bias = tid < 3 * W ? g : -1;  // 0: b1, 1: b2, 2: b3 (unit l)
  if (bias >= 0) {
    pb = a.param[2 * bias + 1][l];
    mb = a.m[2 * bias + 1][l];
    vb = a.v[2 * bias + 1][l];
  }
  // step counts (fp32, as torch keeps them): w1, w2, w3 and the thread's bias
  float st1 = *a.step[0], st2 = *a.step[2], st3 = *a.step[4];
  float stb = *a.step[bias >= 0 ? 2 * bias + 1 : 1];
  bool same = true;  // torch steps all six together: one bias correction a step
#pragma unroll
  for (int k = 1; k < 6; ++k) same = same && *a.step[k] == st1;

  for (int k = tid; k < W * S1; k += 256) w1s[k] = 0.0f;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (tid + 256 * u < n1) w1s[j1[u] * S1 + i1[u]] = p1[u];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    w2s[(g + 8 * u) * S + l] = p2[u];
    w3s[(g + 8 * u) * S + l] = p3[u];
  }
  if (bias == 0) b1s[l] = pb;
  if (bias == 1) b2s[l] = pb;
  if (bias == 2) b3s[l] = pb;

  // --- the gather pipeline
  auto load_idx = [&](int s, int* idx) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int b = g + 8 * r;
      const long long pos = (long long)s * B + b;
      long long v = 0;
      if (s < s1 && b < B && pos < (long long)n) v = perm[pos];
      v = v < 0 ? 0 : (v >= (long long)n ? (long long)n - 1 : v);  // never past x, y
      idx[r] = (int)v;
    }
  };
  auto gather = [&](int s, const int* idx, float* xr, float* yr) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int b = g + 8 * r;
      const bool valid = s < s1 && b < B && (long long)s * B + b < (long long)n;
      xr[r] = valid && l < d_in ? x[(size_t)idx[r] * d_in + l] : 0.0f;
      yr[r] = valid ? y[(size_t)idx[r] * W + l] : 0.0f;
    }
  };
  int idx_a[R], idx_b[R];
  float xn[R], yn[R], yc[R];
  load_idx(s0, idx_a);
  gather(s0, idx_a, xn, yc);
  load_idx(s0 + 1, idx_a);
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (l < kRndMaxIn) xs[0][g + 8 * r][l] = xn[r];
  __syncthreads();

  for (int s = s0; s < s1; ++s) {
    const int slot = (s - s0) & 1;
    const int rows = min(B, n - s * B);  // s B < n < 2^31
    load_idx(s + 2, idx_b);
    gather(s + 1, idx_a, xn, yn);
    const float (*xc)[kRndMaxIn] = xs[slot];

    // 1: z1 = W1 x + b1
    float z1[R], z2[R], acc[R];
    {
      const float bj = b1s[l];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = bj;
      for (int i = 0; i < d_in; ++i) {
        const float w = w1s[l * S1 + i];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(w, xc[g + 8 * r][i], acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        z1[r] = acc[r];
        h1[g + 8 * r][l] = fmaxf(acc[r], 0.0f);
      }
    }
    __syncthreads();
    // 2: z2 = W2 h1 + b2
    {
      const float bj = b2s[l];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = bj;
      rnd_rows_dot<R>(&w2s[l * S], h1, g, acc);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        z2[r] = acc[r];
        h2[g + 8 * r][l] = fmaxf(acc[r], 0.0f);
      }
    }
    __syncthreads();
    // 3: pred = W3 h2 + b3; dP = d/dpred mean(|pred - y|^order)
    {
      const float bj = b3s[l];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = bj;
      rnd_rows_dot<R>(&w3s[l * S], h2, g, acc);
      const float inv = 1.0f / (float)(rows * W);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float d = acc[r] - yc[r], ad = fabsf(d);
        const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        // order |d|^(order - 1) sign(d) / (rows W); order 1: sign(d), 0 at d == 0
        const float pw = order == 2 ? ad : rnd_powi(ad, order - 1);
        const bool valid = g + 8 * r < rows;
        dP[g + 8 * r][l] = valid ? (float)order * pw * sgn * inv : 0.0f;
        if (loss_out) lbuf[g + 8 * r][l] = valid ? pw * ad : 0.0f;
      }
    }
    __syncthreads();
    // the step's bias corrections (off the data's chain)
    st1 += 1.0f;
    st2 += 1.0f;
    st3 += 1.0f;
    stb += 1.0f;
    const RndBias c3 = rnd_bias(a, st3);
    const RndBias c2 = same ? c3 : rnd_bias(a, st2);
    const RndBias c1 = same ? c3 : rnd_bias(a, st1);
    const RndBias cb = same ? c3 : rnd_bias(a, stb);
    // 4: dz2 = (dP W3) [z2 > 0]; gW3 = dP^T h2; gb3
    {
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.0f;
      rnd_cols_dot<R>(&w3s[l], dP, g, acc);
#pragma unroll
      for (int r = 0; r < R; ++r) dz2[g + 8 * r][l] = z2[r] > 0.0f ? acc[r] : 0.0f;
      float gw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
      for (int b = 0; b < NB; ++b) {
        const float h = h2[b][l];
#pragma unroll
        for (int u = 0; u < 4; ++u) gw[u] = __builtin_fmaf(dP[b][g + 8 * u], h, gw[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) rnd_adam(a, c3, gw[u], p3[u], m3[u], v3[u]);
      if (bias == 2) {
        float gb = 0.0f;
#pragma unroll 8
        for (int b = 0; b < NB; ++b) gb += dP[b][l];
        rnd_adam(a, cb, gb, pb, mb, vb);
        b3s[l] = pb;  // read in phase 3 only
      }
      if (loss_out && tid < 64) {  // the loss: lane sums in order, then a fixed tree
        const float* e = &lbuf[0][0];
        float sum = 0.0f;
        for (int k = tid; k < NB * W; k += 64) sum += e[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (tid == 0) loss_out[s] = sum / (float)(rows * W);
      }
    }
    __syncthreads();
    // 5: dz1 = (dz2 W2) [z1 > 0]; gW2 = dz2^T h1; gb2
    {
#pragma unroll
      for (int u = 0; u < 4; ++u) w3s[(g + 8 * u) * S + l] = p3[u];  // not read before 3
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = 0.0f;
      rnd_cols_dot<R>(&w2s[l], dz2, g, acc);
#pragma unroll
      for (int r = 0; r < R; ++r) dz1[g + 8 * r][l] = z1[r] > 0.0f ? acc[r] : 0.0f;
      float gw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
      for (int b = 0; b < NB; ++b) {
        const float h = h1[b][l];
#pragma unroll
        for (int u = 0; u < 4; ++u) gw[u] = __builtin_fmaf(dz2[b][g + 8 * u], h, gw[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) rnd_adam(a, c2, gw[u], p2[u], m2[u], v2[u]);
      if (bias == 1) {
        float gb = 0.0f;
#pragma unroll 8
        for (int b = 0; b < NB; ++b) gb += dz2[b][l];
        rnd_adam(a, cb, gb, pb, mb, vb);
        b2s[l] = pb;  // read in phase 2 only
      }
    }
    __syncthreads();
    // 6: gW1 = dz1^T x; gb1; the next step's rows into the ring
    {
#pragma unroll
      for (int u = 0; u < 4; ++u) w2s[(g + 8 * u) * S + l] = p2[u];  // not read before 2
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (tid + 256 * u < n1) {
          float gw = 0.0f;
#pragma unroll 8
          for (int b = 0; b < NB; ++b) gw = __builtin_fmaf(dz1[b][j1[u]], xc[b][i1[u]], gw);
          rnd_adam(a, c1, gw, p1[u], m1[u], v1[u]);
          w1s[j1[u] * S1 + i1[u]] = p1[u];  // read in phase 1 only
        }
      }
      if (bias == 0) {
        float gb = 0.0f;
#pragma unroll 8
        for (int b = 0; b < NB; ++b) gb += dz1[b][l];
        rnd_adam(a, cb, gb, pb, mb, vb);
        b1s[l] = pb;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (l < kRndMaxIn) xs[slot ^ 1][g + 8 * r][l] = xn[r];
        yc[r] = yn[r];
        idx_a[r] = idx_b[r];
      }
    }
    __syncthreads();
  }

  // --- back to torch's tensors, in place
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = tid + 256 * u;
    if (e < n1) {
      a.param[0][e] = p1[u];
      a.m[0][e] = m1[u];
      a.v[0][e] = v1[u];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid + 256 * u;
    a.param[2][e] = p2[u];
    a.m[2][e] = m2[u];
    a.v[2][e] = v2[u];
    a.param[4][e] = p3[u];
    a.m[4][e] = m3[u];
    a.v[4][e] = v3[u];
  }
  if (bias >= 0) {
    a.param[2 * bias + 1][l] = pb;
    a.m[2 * bias + 1][l] = mb;
    a.v[2 * bias + 1][l] = vb;
    if (l == 0) *a.step[2 * bias + 1] = stb;
  }
  if (tid == 0) {
    *a.step[0] = st1;
    *a.step[2] = st2;
    *a.step[4] = st3;
  }
}

}  // namespace swarm
