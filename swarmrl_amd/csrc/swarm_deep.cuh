// swarm_deep.cuh -- a deep actor-critic MLP (2 or 3 hidden ReLU layers) on
// the fused paths: the rollout policy here, the PPO epoch gradient further
// down.
//
//   k_policy_deep_sample  the whole rollout policy of a network with L = 2 or
//                         3 hidden ReLU layers in one launch:
//                           h_1 = relu(W_1 x + b_1)
//                           h_l = relu(W_l h_{l-1} + b_l)
//                           logits = Wa h_L + ba
//                         and then the sampling tail of swarm_policy.cuh
//                         unchanged (sample_logits_reg / policy_emit: the same
//                         Philox keys, the same per-64-agent call counters and
//                         advance_group_counter contract), so a graph replay
//                         draws fresh numbers and the actions are bit-identical
//                         to k_sample_actions on this kernel's own logits.
//                         The critic head is not evaluated (the rollout never
//                         reads it, flax_network.py:174-195).
//
// The network of CI/unit_tests/force_function/test_force_fn.py:38-45 (three
// hidden layers) and the common 2 x 128 one; swarm_policy.cuh covers one
// hidden layer only.
//
// Decomposition: a workgroup of 4 waves takes 64 agents (one counter group,
// so no group straddles a block).  The activations of the 64 agents live in
// one LDS image [64][kDeepStride]; every layer is a product [units x K] x
// [K x agents] on v_mfma_f32_16x16x4_f32 with the units as M (A operand: the
// torch weight rows, read in place from global memory -- 64 KB per 128 x 128
// layer, shared by every block, so L2 hits) and the agents as N (B operand:
// the LDS image).  Wave w owns the unit tiles w and w + 4 for all four agent
// tiles: 8 independent accumulators, 6 float4 loads per 32 MFMAs.  The C/D
// map (col = lane & 15 = agent, row = 4 (lane >> 4) + reg = unit) gives each
// lane four consecutive units of one agent: bias + ReLU and one float4 store
// back into the image, between two barriers.  (Loading the weights of chunk
// c + 1 while chunk c multiplies measured no faster at 4096 agents and 4 %
// slower at 64 x 4096 -- 386 -> 402 us per slice -- and was dropped.)
//
// Numerics: an f32 MFMA is a k-ordered fmaf chain in exact f32.  The k order
// within a chunk of 16 is permuted (step s of lane quarter q takes
// k = 16 c + 4 q + s, so both operands are one float4 load per chunk); the
// sum is a different order of the same f32 products, within the tolerance
// of any f32 GEMM.  Ragged widths are padded with exact zeros (zero weight
// rows and columns, zero biases), which add nothing.
//
// No allocation, no host synchronisation, no run-time-indexed register
// arrays: the launch is capturable.  The deferred cluster build of an engine
// does not ride along in this launch (the stages no launch carried run at
// the next swarm_engine_integrate).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swarm_policy.cuh"
#include "swarm_ppo.cuh"

namespace swarm {

constexpr int kDeepMaxIn = 32;
constexpr int kDeepMinLayers = 2;
constexpr int kDeepMaxLayers = 3;
constexpr int kDeepMaxWidth = 128;
constexpr int kDeepMaxActions = 16;
constexpr int kDeepAgents = 64;    // agents per workgroup: one counter group
constexpr int kDeepStride = 132;   // floats per agent row of the LDS image (128 + 4: the
                                   // float4 reads of 16 rows x 4 quarters spread over all banks)
constexpr int kDeepLogitRow = 17;  // floats per agent row of the logits hand-over

typedef float deep_f4 __attribute__((ext_vector_type(4)));

struct DeepArgs {
  int n_hidden;
  int width[kDeepMaxLayers];
  const float* w[kDeepMaxLayers];  // [width[l]][width[l - 1]] (l = 0: [width[0]][d_in])
  const float* b[kDeepMaxLayers];
  const float* wa;  // [k][width[n_hidden - 1]]
  const float* ba;
};

// W[u][k0 .. k0 + 3] of the row-major matrix W [rows][cols], zeros outside
// it; vec (wave-uniform): rows are whole aligned float4s.
__device__ __forceinline__ deep_f4 deep_w4(const float* __restrict__ W, int rows, int cols, int u,
                                           int k0, bool vec) {
  deep_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (u < rows) {
    const float* r = W + (size_t)u * cols;
    if (vec) {
      if (k0 < cols) v = *reinterpret_cast<const deep_f4*>(r + k0);
    } else {
      if (k0 < cols) v.x = r[k0];
      if (k0 + 1 < cols) v.y = r[k0 + 1];
      if (k0 + 2 < cols) v.z = r[k0 + 2];
      if (k0 + 3 < cols) v.w = r[k0 + 3];
    }
  }
  return v;
}

__device__ __forceinline__ bool deep_rows_vec(const float* W, int cols) {
  return (cols & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
}

// One hidden layer over the block's 64 rows (agents or samples), NW waves.
// in: an LDS image [64][in_stride], columns [0, 16 ceil(cols / 16)) valid on
// entry (finite; the weights past cols are zero); out [64][kDeepStride] (may
// be `in`): on return relu(W in + b) in columns [0, 16 ceil(rows / 16)),
// zeros past rows.  Wave wv owns the unit tiles wv, wv + NW, ...  Every
// thread of the block calls it (two barriers).
template <int NW>
__device__ __forceinline__ void deep_layer(const float* __restrict__ W,
                                           const float* __restrict__ bias, int rows, int cols,
                                           const float* in, int in_stride, float* out, int lane,
                                           int wv) {
  constexpr int J = 8 / NW;
  const int ntile = (rows + 15) >> 4, nchunk = (cols + 15) >> 4;
  const int ul = lane & 15, q = lane >> 4;
  const bool vec = deep_rows_vec(W, cols);
  deep_f4 acc[J][4];
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[j][m] = deep_f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int c = 0; c < nchunk; ++c) {
    const int k0 = 16 * c + 4 * q;
    deep_f4 hb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      hb[m] = *reinterpret_cast<const deep_f4*>(in + (16 * m + ul) * in_stride + k0);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int t = wv + NW * j;
      if (t < ntile) {
        const deep_f4 wf = deep_w4(W, rows, cols, 16 * t + ul, k0, vec);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int m = 0; m < 4; ++m)
            acc[j][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], hb[m][s], acc[j][m], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // every wave has read the layer's input
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int t = wv + NW * j;
    if (t < ntile) {
      const int u0 = 16 * t + 4 * q;  // this lane's four units (rows 4 q + reg of the tile)
      deep_f4 bb;
      bb.x = u0 < rows ? bias[u0] : 0.0f;
      bb.y = u0 + 1 < rows ? bias[u0 + 1] : 0.0f;
      bb.z = u0 + 2 < rows ? bias[u0 + 2] : 0.0f;
      bb.w = u0 + 3 < rows ? bias[u0 + 3] : 0.0f;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        deep_f4 h = acc[j][m] + bb;
        h.x = fmaxf(h.x, 0.0f);
        h.y = fmaxf(h.y, 0.0f);
        h.z = fmaxf(h.z, 0.0f);
        h.w = fmaxf(h.w, 0.0f);
        *reinterpret_cast<deep_f4*>(out + (16 * m + ul) * kDeepStride + u0) = h;
      }
    }
  }
  __syncthreads();
}

// An output head W [rows <= 16][cols] over row tile wv (< 4) of the image
// act [64][kDeepStride]: head rows as M (rows past `rows` are zero).  Lane
// (ul, q) returns rows 4 q + reg of image row 16 wv + ul, without the bias.
// Two accumulators (even and odd chunks) for the MFMA latency.
__device__ __forceinline__ deep_f4 deep_head(const float* __restrict__ W, int rows, int cols,
                                             const float* act, int lane, int wv) {
  const int ul = lane & 15, q = lane >> 4;
  const int nchunk = (cols + 15) >> 4;
  const bool vec = deep_rows_vec(W, cols);
  const float* hrow = act + (16 * wv + ul) * kDeepStride;
  deep_f4 z0 = {0.0f, 0.0f, 0.0f, 0.0f}, z1 = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int c = 0; c < nchunk; c += 2) {
    const int k0 = 16 * c + 4 * q;
    const deep_f4 h0 = *reinterpret_cast<const deep_f4*>(hrow + k0);
    const deep_f4 w0 = deep_w4(W, rows, cols, ul, k0, vec);
    deep_f4 h1 = {0.0f, 0.0f, 0.0f, 0.0f}, w1 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (c + 1 < nchunk) {
      h1 = *reinterpret_cast<const deep_f4*>(hrow + k0 + 16);
      w1 = deep_w4(W, rows, cols, ul, k0 + 16, vec);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[s], h0[s], z0, 0, 0, 0);
      z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[s], h1[s], z1, 0, 0, 0);
    }
  }
  return z0 + z1;
}

// The rows [row0, row0 + 64) of x [n][d] into an LDS image [64][stride],
// zero-padded to whole chunks of 16 columns and past n.  The caller's
// barrier publishes it.
__device__ __forceinline__ void deep_stage_rows(const float* __restrict__ x, long n, int d,
                                                long row0, float* img, int stride) {
  const int kin = (d + 15) & ~15;
  for (int i = threadIdx.x; i < kDeepAgents * kin; i += blockDim.x) {
    const int r = i / kin, c = i - r * kin;
    const long g = row0 + r;
    img[r * stride + c] = (g < n && c < d) ? x[(size_t)g * d + c] : 0.0f;
  }
}

// m carries the sampling arguments (obs, n, d_in, k, keys, counters, tables,
// outputs); its one-hidden-layer weights are not read.  K: the padded action
// count of the sampling tail (4 or 16).
// The body of k_policy_deep_sample: workgroup blockIdx.x of a launch over m.n
// agents.  swarm_ensemble.cuh runs it per member on the member's slices: dp
// then holds the stacked parameters and mi the member, whose layers start
// mi layer sizes in (dp stays the kernel's own argument, so its arrays are
// indexed in place; the single-model kernel passes the constant 0).
template <int K>
__device__ __forceinline__ void deep_policy_body(const MlpArgs& m, const DeepArgs& dp,
                                                 size_t mi) {
  __shared__ __align__(16) float act[kDeepAgents * kDeepStride];
  __shared__ float lgs[kDeepAgents * kDeepLogitRow];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = m.n, k = m.k;
  const int a = blockIdx.x * kDeepAgents + lane;  // the sampling thread's agent (tid < 64)
  const bool valid = tid < kDeepAgents && a < n;
  const unsigned long long ctr = valid ? m.state[a >> 6] : 0ull;
  deep_stage_rows(m.obs, n, m.d_in, (long)blockIdx.x * kDeepAgents, act, kDeepStride);
  __syncthreads();
  int cols = m.d_in;
  for (int l = 0; l < dp.n_hidden; ++l) {
    const int rows = dp.width[l];
    deep_layer<4>(dp.w[l] + mi * (size_t)rows * cols, dp.b[l] + mi * (size_t)rows, rows, cols,
                  act, kDeepStride, act, lane, wv);
    cols = rows;
  }
  // the actor head: wave wv takes agent tile wv
  {
    const float* __restrict__ ba = dp.ba + mi * (size_t)k;
    const deep_f4 z = deep_head(dp.wa + mi * (size_t)k * cols, k, cols, act, lane, wv);
    const int ul = lane & 15, q = lane >> 4;
    float* lrow = lgs + (16 * wv + ul) * kDeepLogitRow + 4 * q;  // actions 4 q + reg
#pragma unroll
    for (int r = 0; r < 4; ++r) lrow[r] = z[r] + (4 * q + r < k ? ba[4 * q + r] : 0.0f);
  }
  __syncthreads();
  if (valid) {
    float lg[K];
#pragma unroll
    for (int j = 0; j < K; ++j) lg[j] = lgs[lane * kDeepLogitRow + j];
    policy_emit<K>(m, a, lg, ctr);
  }
  advance_group_counter(m.state, a, n, tid < kDeepAgents, ctr);
}

template <int K>
__global__ __launch_bounds__(256) void k_policy_deep_sample(MlpArgs m, DeepArgs dp) {
  deep_policy_body<K>(m, dp, 0);
}

// ---------------------------------------------------------------------------
// The gradient of one PPO epoch of the deep actor-critic MLP: the deep
// counterpart of swarm_ppo.cuh (same loss, same GAE, same reference
// semantics -- ProximalPolicyLoss._calculate_loss, swarmrl/losses/
// proximal_policy_loss.py:62-138: R = A_raw + V differentiated through V, only
// the normalised advantages constant, entropy eps 1e-8).  Four launches:
//
//   k_ppo_deep_values  V of every sample (the forward above, critic head)
//   k_ppo_gae          as it stands in swarm_ppo.cuh, without pack workgroups
//   k_ppo_deep_grads   per tile of 64 samples: the forward again, every
//                      layer's activations kept in LDS; dL/dlogits and dL/dV
//                      per sample as k_ppo_grads forms them; then back
//                      through the layers on the f32 matrix instructions:
//                        dW_l += dh_l (x) h_{l-1}   units as M and N, samples as K
//                        db_l += sum_s dh_l         an extra N tile against a
//                                                   column of ones
//                        dh_{l-1} = (W_l^T dh_l) . [h_{l-1} > 0]
//                      (ReLU' at 0 is 0, as torch and k_ppo_grads have it).
//                      A block of 8 waves loops over its tiles with the whole
//                      gradient of the network in accumulators (wave w owns
//                      unit tile w of every layer: 9 accumulator tiles for a
//                      128 x 128 layer) and writes one partial row at the end.
//   k_ppo_reduce       as it stands: fp64 sums of the block partials in a
//                      fixed order.  No floating-point atomics anywhere: the
//                      result is run-to-run identical.
//
// The grid is min(tiles, kDeepPpoBlocks) whatever the device, so the
// summation order depends on the sizes only, and the partial rows (160 KB for
// 32-128-128-128-(16+1)) stay at 40 MB.
constexpr int kDeepPpoBlocks = 256;
constexpr int kDeepXStride = 36;  // floats per sample row of the feature and head-gradient images

struct DeepPpoArgs {
  const float* x;
  int n, d;
  DeepArgs net;  // hidden layers and the actor head
  int k;
  const float* wc;
  const float* bc;
  const int64_t* actions;
  const float* old_logp;
  const float* adv;
  const float* dvalue;
  const double* gae_part;
  int n_part;
  float clip_eps, c_ent;
  // the gradient layout w1 | b1 | ... | wL | bL | wa | ba | wc | bc
  int off_w[kDeepMaxLayers], off_b[kDeepMaxLayers], off_wa, off_ba, off_wc, off_bc, size;
  float* partial;  // [gridDim.x][size]
};

__host__ __device__ constexpr int deep_grads_lds_floats(bool three) {
  // features | head gradients | dh (the logits hand-over aliases it) | h_1 .. h_L
  return 2 * kDeepAgents * kDeepXStride + (three ? 4 : 3) * kDeepAgents * kDeepStride;
}

// net and mi as in deep_policy_body (the hidden layers of member mi of a
// stack; 0 for a single model); x, wc, bc and values are the member's own.
template <int NW>
__device__ __forceinline__ void deep_ppo_values_body(const float* __restrict__ x, int n, int d,
                                                     const DeepArgs& net,
                                                     const float* __restrict__ wc,
                                                     const float* __restrict__ bc,
                                                     float* __restrict__ values, size_t mi) {
  __shared__ __align__(16) float act[kDeepAgents * kDeepStride];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long row0 = (long)blockIdx.x * kDeepAgents;
  deep_stage_rows(x, n, d, row0, act, kDeepStride);
  __syncthreads();
  int cols = d;
  for (int l = 0; l < net.n_hidden; ++l) {
    const int rows = net.width[l];
    deep_layer<NW>(net.w[l] + mi * (size_t)rows * cols, net.b[l] + mi * (size_t)rows, rows, cols,
                   act, kDeepStride, act, lane, wv);
    cols = rows;
  }
  if (wv < 4) {  // the critic as a head of one row: row 0 is with lanes q = 0, reg 0
    const deep_f4 z = deep_head(wc, 1, cols, act, lane, wv);
    const long s = row0 + 16 * wv + (lane & 15);
    if ((lane >> 4) == 0 && s < n) values[s] = z[0] + bc[0];
  }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_ppo_deep_values(const float* __restrict__ x, int n,
                                                             int d, DeepArgs net,
                                                             const float* __restrict__ wc,
                                                             const float* __restrict__ bc,
                                                             float* __restrict__ values) {
  deep_ppo_values_body<NW>(x, n, d, net, wc, bc, values, 0);
}

// ppo_advantage_sums for a block of up to 8 waves (fixed order: thread-strided
// sums, xor-shuffle tree, waves in order).
__device__ inline void deep_advantage_sums(const double* __restrict__ part, int n_part,
                                           double* out) {
  __shared__ double red[2][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n_part; i += blockDim.x) {
    a += part[2 * i];
    b += part[2 * i + 1];
  }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if (lane == 0) {
    red[0][w] = a;
    red[1][w] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) {
    a += red[0][i];
    b += red[1][i];
  }
  out[0] = a;
  out[1] = b;
}

// gout[s][v] = (sum_u wt(u, v) gin[s][u]) . [hprev[s][v] > 0] over the block's
// 64 samples: v (cols of them) as M, samples as N, u (rows of them) as K.
// wt(u, v): the weight, zero outside the matrix.  gin [64][gin_stride],
// columns [0, 16 ceil(rows / 16)) valid; gout [64][kDeepStride] (may be gin):
// columns [0, 16 ceil(cols / 16)) on return, zeros past cols.  Two barriers.
template <int NW, typename WT>
__device__ __forceinline__ void deep_backward(WT wt, int rows, int cols, const float* gin,
                                              int gin_stride, float* gout, const float* hprev,
                                              int lane, int wv) {
  constexpr int J = 8 / NW;
  const int ntile = (cols + 15) >> 4, nchunk = (rows + 15) >> 4;
  const int ul = lane & 15, q = lane >> 4;
  deep_f4 acc[J][4];
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[j][m] = deep_f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int c = 0; c < nchunk; ++c) {
    const int k0 = 16 * c + 4 * q;
    deep_f4 gb[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      gb[m] = *reinterpret_cast<const deep_f4*>(gin + (16 * m + ul) * gin_stride + k0);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int t = wv + NW * j;
      if (t < ntile) {
        deep_f4 wf;
        wf.x = wt(k0, 16 * t + ul);
        wf.y = wt(k0 + 1, 16 * t + ul);
        wf.z = wt(k0 + 2, 16 * t + ul);
        wf.w = wt(k0 + 3, 16 * t + ul);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int m = 0; m < 4; ++m)
            acc[j][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], gb[m][s], acc[j][m], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // every wave has read gin
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int t = wv + NW * j;
    if (t < ntile) {
      const int v0 = 16 * t + 4 * q;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int o = (16 * m + ul) * kDeepStride + v0;
        const deep_f4 h = *reinterpret_cast<const deep_f4*>(hprev + o);
        deep_f4 r = acc[j][m];
        r.x = h.x > 0.0f ? r.x : 0.0f;
        r.y = h.y > 0.0f ? r.y : 0.0f;
        r.z = h.z > 0.0f ? r.z : 0.0f;
        r.w = h.w > 0.0f ? r.w : 0.0f;
        *reinterpret_cast<deep_f4*>(gout + o) = r;
      }
    }
  }
  __syncthreads();
}

// acc[vt] += g[:, unit tile wv]^T hp[:, tile vt] over the 64 samples (K), and
// accb += g[:, unit tile wv]^T [1 0 .. 0] (column 0: the bias gradient).
// g [64][kDeepStride]; hp [64][hp_stride] with nvt <= NVT valid tiles.
template <int NVT>
__device__ __forceinline__ void deep_dw(const float* g, const float* hp, int hp_stride, int nvt,
                                        int lane, int wv, deep_f4 (&acc)[NVT], deep_f4& accb) {
  const int ul = lane & 15, q = lane >> 4;
  const float one = ul == 0 ? 1.0f : 0.0f;
#pragma unroll 2
  for (int c = 0; c < kDeepAgents / 4; ++c) {
    const int s = 4 * c + q;
    const float a = g[s * kDeepStride + 16 * wv + ul];
#pragma unroll
    for (int vt = 0; vt < NVT; ++vt) {
      if (vt < nvt) {
        const float b = hp[s * hp_stride + 16 * vt + ul];
        acc[vt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[vt], 0, 0, 0);
      }
    }
    accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a, one, accb, 0, 0, 0);
  }
}

// The accumulators of deep_dw into the block's partial row: rows u = 16 wv +
// 4 q + reg of W [rows][cols] at off_w, column 0 of accb into the bias.
template <int NVT>
__device__ __forceinline__ void deep_store_dw(float* out, int off_w, int off_b, int rows,
                                              int cols, int lane, int wv,
                                              const deep_f4 (&acc)[NVT], const deep_f4& accb) {
  const int ul = lane & 15, q = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = 16 * wv + 4 * q + r;
    if (u < rows) {
#pragma unroll
      for (int vt = 0; vt < NVT; ++vt) {
        const int v = 16 * vt + ul;
        if (v < cols) out[off_w + u * cols + v] = acc[vt][r];
      }
      if (ul == 0) out[off_b + u] = accb[r];
    }
  }
}

// K: the padded action count of the per-sample phase (4 or 16); L3: three
// hidden layers (else two).  Block of 8 waves, dynamic LDS
// deep_grads_lds_floats(L3) floats (deep_lds).  Block blockIdx.x of
// gridDim.x takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of the
// p.n samples and writes row blockIdx.x of p.partial.
template <int K, bool L3>
__device__ __forceinline__ void deep_ppo_grads_body(const DeepPpoArgs& p, float* deep_lds) {
  constexpr int NW = 8;
  float* X = deep_lds;                            // [64][kDeepXStride] features
  float* gz = X + kDeepAgents * kDeepXStride;     // [64][kDeepXStride] dL/dz | dL/dV | 0
  float* g = gz + kDeepAgents * kDeepXStride;     // [64][kDeepStride] dh of the current layer
  float* h1 = g + kDeepAgents * kDeepStride;
  float* h2 = h1 + kDeepAgents * kDeepStride;
  float* h3 = h2 + kDeepAgents * kDeepStride;     // L3 only
  float* lgs = g;                                 // [64][kDeepLogitRow], dead before g is written
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ul = lane & 15, q = lane >> 4;
  const int n = p.n, d = p.d, k = p.k;
  const int H1 = p.net.width[0], H2 = p.net.width[1], H3 = L3 ? p.net.width[2] : 0;
  const int HL = L3 ? H3 : H2;
  const float* hL = L3 ? h3 : h2;
  const float* __restrict__ wa = p.net.wa;
  const float* __restrict__ wc = p.wc;
  // normalised advantages (A - mean) / (std + eps): population std, fp32 eps
  double stats[2];
  deep_advantage_sums(p.gae_part, p.n_part, stats);
  const double mean = stats[0] / (double)n;
  const double var = fmax(stats[1] / (double)n - mean * mean, 0.0);
  const float a_mean = (float)mean;
  const float a_den = (float)sqrt(var) + 1.1920928955078125e-07f;
  const deep_f4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  deep_f4 aw1[2] = {zero4, zero4}, ab1 = zero4;
  deep_f4 aw2[8], ab2 = zero4, aw3[8], ab3 = zero4, ah[2] = {zero4, zero4};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    aw2[i] = zero4;
    aw3[i] = zero4;
  }
  deep_f4 ahb[2] = {zero4, zero4};  // wave 0: the head biases (column 0)
  const int nht = (k + 1 + 15) >> 4;  // head rows: the k actions, then the value
  const long tiles = ((long)n + kDeepAgents - 1) / kDeepAgents;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long row0 = tile * kDeepAgents;
    deep_stage_rows(p.x, n, d, row0, X, kDeepXStride);
    __syncthreads();
    deep_layer<NW>(p.net.w[0], p.net.b[0], H1, d, X, kDeepXStride, h1, lane, wv);
    deep_layer<NW>(p.net.w[1], p.net.b[1], H2, H1, h1, kDeepStride, h2, lane, wv);
    if constexpr (L3) deep_layer<NW>(p.net.w[2], p.net.b[2], H3, H2, h2, kDeepStride, h3, lane, wv);
    if (wv < 4) {
      const deep_f4 z = deep_head(wa, k, HL, hL, lane, wv);
      float* lrow = lgs + (16 * wv + ul) * kDeepLogitRow + 4 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r) lrow[r] = z[r] + (4 * q + r < k ? p.net.ba[4 * q + r] : 0.0f);
    }
    __syncthreads();
    // per sample: dL/dz of the clipped surrogate and the entropy term, dL/dV
    // from k_ppo_gae (k_ppo_grads, phase P)
    if (tid < kDeepAgents) {
      const long si = row0 + tid;
      float gq[K], dvs = 0.0f;
#pragma unroll
      for (int j = 0; j < K; ++j) gq[j] = 0.0f;
      if (si < n) {
        float z[K], pr[K];
#pragma unroll
        for (int j = 0; j < K; ++j) z[j] = lgs[tid * kDeepLogitRow + j];
        float m = z[0];
#pragma unroll
        for (int j = 1; j < K; ++j)
          if (j < k) m = fmaxf(m, z[j]);
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          pr[j] = j < k ? expf(z[j] - m) : 0.0f;
          sum += pr[j];
        }
        const int a = (int)p.actions[si];
        float pa = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          pr[j] = pr[j] / sum;
          pa = j == a ? pr[j] : pa;
        }
        // -min(r A, clip(r, 1 - eps, 1 + eps) A): a tie splits the gradient
        // evenly between the two arguments, clip passes it on its closed range
        const float A = (p.adv[si] - a_mean) / a_den;
        const float r = expf(logf(pa + 1e-8f) - p.old_logp[si]);
        const float lo = 1.0f - p.clip_eps, hi = 1.0f + p.clip_eps;
        const float rc = fminf(fmaxf(r, lo), hi);
        const float t1 = r * A, t2 = rc * A;
        const float w1st = t1 < t2 ? 1.0f : (t1 > t2 ? 0.0f : 0.5f);
        const float in = (r >= lo && r <= hi) ? 1.0f : 0.0f;
        const float d_r = -A * (w1st + (1.0f - w1st) * in);
        const float d_pa = d_r * r / (pa + 1e-8f);
        // entropy term: + c_ent sum_j (p_j + eps) log(p_j + eps)
        float dp[K], pdp = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          dp[j] = j < k ? p.c_ent * (logf(pr[j] + 1e-8f) + 1.0f) + (j == a ? d_pa : 0.0f) : 0.0f;
          pdp = fmaf(pr[j], dp[j], pdp);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) gq[j] = pr[j] * (dp[j] - pdp);
        dvs = p.dvalue[si];
      }
      float* row = gz + tid * kDeepXStride;
#pragma unroll
      for (int c = 0; c < 8; ++c) reinterpret_cast<deep_f4*>(row)[c] = zero4;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j < k) row[j] = gq[j];
      }
      row[k] = dvs;
    }
    __syncthreads();
    // the heads: d[Wa; Wc] += gz^T h_L (head rows as M, this wave's units as N;
    // wave 0 also sums gz against a column of ones: d[ba; bc])
    if (wv < ((HL + 15) >> 4)) {
      const float one = ul == 0 ? 1.0f : 0.0f;
#pragma unroll 2
      for (int c = 0; c < kDeepAgents / 4; ++c) {
        const int s = 4 * c + q;
        const float b = hL[s * kDeepStride + 16 * wv + ul];
#pragma unroll
        for (int ht = 0; ht < 2; ++ht) {
          if (ht < nht) {
            const float a = gz[s * kDeepXStride + 16 * ht + ul];
            ah[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, ah[ht], 0, 0, 0);
            if (wv == 0) ahb[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, one, ahb[ht], 0, 0, 0);
          }
        }
      }
    }
    // dh_L = ([Wa; Wc]^T gz) . [h_L > 0]
    deep_backward<NW>(
        [&](int u, int v) {
          return v < HL ? (u < k ? wa[(size_t)u * HL + v] : (u == k ? wc[v] : 0.0f)) : 0.0f;
        },
        k + 1, HL, gz, kDeepXStride, g, hL, lane, wv);
    if constexpr (L3) {
      if (wv < ((H3 + 15) >> 4)) deep_dw<8>(g, h2, kDeepStride, (H2 + 15) >> 4, lane, wv, aw3, ab3);
      const float* __restrict__ w3 = p.net.w[2];
      deep_backward<NW>(
          [&](int u, int v) { return (u < H3 && v < H2) ? w3[(size_t)u * H2 + v] : 0.0f; }, H3,
          H2, g, kDeepStride, g, h2, lane, wv);
    }
    if (wv < ((H2 + 15) >> 4)) deep_dw<8>(g, h1, kDeepStride, (H1 + 15) >> 4, lane, wv, aw2, ab2);
    {
      const float* __restrict__ w2 = p.net.w[1];
      deep_backward<NW>(
          [&](int u, int v) { return (u < H2 && v < H1) ? w2[(size_t)u * H1 + v] : 0.0f; }, H2,
          H1, g, kDeepStride, g, h1, lane, wv);
    }
    if (wv < ((H1 + 15) >> 4)) deep_dw<2>(g, X, kDeepXStride, (d + 15) >> 4, lane, wv, aw1, ab1);
    __syncthreads();  // the images are rewritten by the next tile
  }
  float* out = p.partial + (size_t)blockIdx.x * p.size;
  deep_store_dw<2>(out, p.off_w[0], p.off_b[0], H1, d, lane, wv, aw1, ab1);
  deep_store_dw<8>(out, p.off_w[1], p.off_b[1], H2, H1, lane, wv, aw2, ab2);
  if constexpr (L3) deep_store_dw<8>(out, p.off_w[2], p.off_b[2], H3, H2, lane, wv, aw3, ab3);
  {
    const int u = 16 * wv + ul;  // head accumulators: rows 16 ht + 4 q + reg, column u
#pragma unroll
    for (int ht = 0; ht < 2; ++ht) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int hr = 16 * ht + 4 * q + r;
        if (u < HL && hr < k) out[p.off_wa + hr * HL + u] = ah[ht][r];
        if (u < HL && hr == k) out[p.off_wc + u] = ah[ht][r];
        if (wv == 0 && ul == 0 && hr < k) out[p.off_ba + hr] = ahb[ht][r];
        if (wv == 0 && ul == 0 && hr == k) out[p.off_bc] = ahb[ht][r];
      }
    }
  }
}

template <int K, bool L3>
__global__ __launch_bounds__(512) void k_ppo_deep_grads(DeepPpoArgs p) {
  extern __shared__ __align__(16) float deep_lds[];
  deep_ppo_grads_body<K, L3>(p, deep_lds);
}

}  // namespace swarm
