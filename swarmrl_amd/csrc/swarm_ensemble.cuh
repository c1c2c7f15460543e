// swarm_ensemble.cuh -- M independent actor-critic MLPs in one launch.
//
// The reference trains a population of models with one process and one
// engine each (swarmrl/training_routines/ensemble_submit.py:93-138).  Here
// member m of an ensemble owns a contiguous block of the engine's envs and
// its own weights, seed and call counters; the member index is the outer
// grid dimension (blockIdx.y) of every kernel, and blockIdx.x / gridDim.x
// keep the meaning they have in the single-model kernels.  Each kernel
// offsets its pointers to the member's slices and runs the single-model body
// (policy_body of swarm_policy.cuh, the ppo_*_body functions of
// swarm_ppo.cuh, the deep_*_body functions of swarm_deep.cuh) on them: the
// same instructions in the same order on the
// same values, so a member's results are bit-identical to the single-model
// call on its slice alone, whoever shares the launch.  A workgroup serves
// one member only; sample, agent and counter-group indices are local to the
// member.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swarm_deep.cuh"
#include "swarm_policy.cuh"
#include "swarm_ppo.cuh"

namespace swarm {

constexpr int kEnsembleMaxMembers = 1024;

// swarm_policy_ensemble_sample: obs [M][n_per][d_in], stacked torch Linear
// layouts w1 [M][hidden][d_in], b1 [M][hidden], w2 [M][k][hidden], b2 [M][k],
// seeds [M] (device), state [M][n_state_per], outputs [M * n_per].
struct EnsembleMlpArgs {
  MlpArgs m;  // member 0's pointers; n = n_per; the keys are read from seeds
  const unsigned long long* seeds;
  int n_state_per;
};

template <int G, int D, int K>
__global__ __launch_bounds__(256) void k_policy_ensemble_sample(EnsembleMlpArgs e) {
  extern __shared__ __align__(16) float sw[];
  const size_t mi = blockIdx.y;
  MlpArgs m = e.m;
  const size_t n = (size_t)m.n;
  m.obs += mi * n * m.d_in;
  m.w1 += mi * (size_t)m.hidden * m.d_in;
  m.b1 += mi * (size_t)m.hidden;
  m.w2 += mi * (size_t)m.k * m.hidden;
  m.b2 += mi * (size_t)m.k;
  const unsigned long long seed = e.seeds[mi];
  m.key0 = (uint32_t)seed;
  m.key1 = (uint32_t)(seed >> 32);
  m.state += mi * (size_t)e.n_state_per;
  m.out_idx += mi * n;
  m.out_logp += mi * n;
  m.out_f += mi * n;
  m.out_t += mi * n;
  if (m.out_logits) m.out_logits += mi * n * m.k;
  policy_body<G, D, K>(m, blockIdx.x, sw);
}

// swarm_ppo_ensemble_epoch_grad: member-major data and stacked parameters
// (member 0's pointers; the strides follow from the sizes), per-member
// workspace slices, and the stacked gradient layout
// w1 [M][H*D] | b1 [M][H] | wa [M][K*H] | ba [M][K] | wc [M][H] | bc [M].
struct PpoEnsembleArgs {
  const float* x;            // [M][n][d]
  const int64_t* actions;    // [M][n]
  const float* old_logp;     // [M][n]
  const float* rewards;      // [M][T][S]
  const float *w1, *b1, *wa, *ba, *wc, *bc;
  int T, S, n, d, hidden, k, members;
  float gamma, lambda, clip_eps, c_ent;
  float *values, *adv, *dv;  // [M][n]
  double* spart;             // [M][2 gae_blocks]
  float* table;              // [M][table_floats]
  float* partial;            // [M][blocks][ppo_grad_size]
  float* grad;
  int gae_blocks, table_rows, table_floats, blocks;
};

template <int D>
__global__ __launch_bounds__(256) void k_ppo_ensemble_values(PpoEnsembleArgs a) {
  const size_t mi = blockIdx.y, n = (size_t)a.n;
  ppo_values_body<D>(a.x + mi * n * a.d, a.n, a.d, a.w1 + mi * (size_t)a.hidden * a.d,
                     a.b1 + mi * a.hidden, a.hidden, a.wc + mi * a.hidden, a.bc + mi,
                     a.values + mi * n);
}

template <int D>
__global__ __launch_bounds__(256) void k_ppo_ensemble_values_split(PpoEnsembleArgs a) {
  const size_t mi = blockIdx.y, n = (size_t)a.n;
  ppo_values_split_body<D>(a.x + mi * n * a.d, a.n, a.d, a.w1 + mi * (size_t)a.hidden * a.d,
                           a.b1 + mi * a.hidden, a.hidden, a.wc + mi * a.hidden, a.bc + mi,
                           a.values + mi * n);
}

template <int TM, int D, int K>
__global__ __launch_bounds__(256) void k_ppo_ensemble_gae(PpoEnsembleArgs a) {
  const size_t mi = blockIdx.y, n = (size_t)a.n;
  const PpoPack pk{a.w1 + mi * (size_t)a.hidden * a.d,
                   a.b1 + mi * a.hidden,
                   a.wa + mi * (size_t)a.k * a.hidden,
                   a.wc + mi * a.hidden,
                   a.d,
                   a.hidden,
                   a.k,
                   a.table_rows,
                   a.table + mi * (size_t)a.table_floats};
  ppo_gae_body<TM, D, K>(a.rewards + mi * n, a.values + mi * n, a.T, a.S, a.gamma, a.lambda,
                         a.adv + mi * n, a.dv + mi * n, a.spart + mi * 2 * (size_t)a.gae_blocks,
                         a.gae_blocks, pk);
}

template <int NW, int NT, bool kCoop, int D, int K>
__global__ __launch_bounds__(64 * NW * NT) void k_ppo_ensemble_grads(PpoEnsembleArgs a) {
  const size_t mi = blockIdx.y, n = (size_t)a.n;
  const size_t size = (size_t)ppo_grad_size(a.d, a.hidden, a.k);
  ppo_grads_body<NW, NT, kCoop, D, K>(
      a.x + mi * n * a.d, a.n, a.d, a.w1 + mi * (size_t)a.hidden * a.d, a.b1 + mi * a.hidden,
      a.hidden, a.wa + mi * (size_t)a.k * a.hidden, a.ba + mi * a.k, a.k, a.wc + mi * a.hidden,
      a.bc + mi, a.actions + mi * n, a.old_logp + mi * n, a.adv + mi * n, a.dv + mi * n,
      a.spart + mi * 2 * (size_t)a.gae_blocks, a.gae_blocks,
      a.table + mi * (size_t)a.table_floats, a.clip_eps, a.c_ent,
      a.partial + mi * (size_t)a.blocks * size);
}

// Member blockIdx.y's block partials -> its rows of the stacked gradient.
__global__ __launch_bounds__(1024) void k_ppo_ensemble_reduce(PpoEnsembleArgs a) {
  const size_t mi = blockIdx.y, M = (size_t)a.members;
  const int size = ppo_grad_size(a.d, a.hidden, a.k);
  const int sizes[6] = {a.hidden * a.d, a.hidden, a.k * a.hidden, a.k, a.hidden, 1};
  float* grad = a.grad;
  ppo_reduce_body(a.partial + mi * (size_t)a.blocks * size, a.blocks, size, [&](int p, float g) {
    int lo = 0, len = sizes[0];  // p's tensor: parameters [lo, lo + len)
#pragma unroll
    for (int t = 1; t < 6; ++t) {
      if (p >= lo + len) {
        lo += len;
        len = sizes[t];
      }
    }
    grad[M * lo + mi * len + (p - lo)] = g;
  });
}

// ---------------------------------------------------------------------------
// Ensembles of deep actor-critic MLPs (2 or 3 hidden layers, swarm_deep.cuh).

// Member mi's hidden layers and actor head for the gradient kernel, which
// indexes them with constants: every stacked tensor at member
// stride ([M][width[l]][width[l - 1]], [M][width[l]], wa [M][k][width[L - 1]],
// ba [M][k]).  Returns the last hidden width.
__device__ __forceinline__ int deep_member_net(DeepArgs& net, size_t mi, int d_in, int k) {
  int prev = d_in;
#pragma unroll
  for (int l = 0; l < kDeepMaxLayers; ++l) {
    if (l < net.n_hidden) {
      net.w[l] += mi * (size_t)net.width[l] * prev;
      net.b[l] += mi * (size_t)net.width[l];
      prev = net.width[l];
    }
  }
  net.wa += mi * (size_t)k * prev;
  net.ba += mi * (size_t)k;
  return prev;
}

// swarm_policy_deep_ensemble_sample: obs [M][n_per][d_in], seeds [M] (device),
// state [M][n_state_per], outputs [M * n_per].  Grid (ceil(n_per / 64), M):
// one workgroup is one counter group of one member.
struct DeepEnsembleArgs {
  MlpArgs m;    // member 0's pointers; n = n_per; the keys are read from seeds
  DeepArgs dp;  // member 0's pointers
  const unsigned long long* seeds;
  int n_state_per;
};

template <int K>
__global__ __launch_bounds__(256) void k_policy_deep_ensemble_sample(DeepEnsembleArgs e) {
  const size_t mi = blockIdx.y;
  MlpArgs m = e.m;
  const size_t n = (size_t)m.n;
  m.obs += mi * n * m.d_in;
  const unsigned long long seed = e.seeds[mi];
  m.key0 = (uint32_t)seed;
  m.key1 = (uint32_t)(seed >> 32);
  m.state += mi * (size_t)e.n_state_per;
  m.out_idx += mi * n;
  m.out_logp += mi * n;
  m.out_f += mi * n;
  m.out_t += mi * n;
  if (m.out_logits) m.out_logits += mi * n * m.k;
  deep_policy_body<K>(m, e.dp, mi);  // the member's layers of the stack e.dp
}

// swarm_ppo_deep_ensemble_epoch_grad: p holds member 0's pointers (data,
// stacked parameters, workspace slices) and the single-model gradient layout;
// the strides follow from the sizes.  The GAE launch is k_ppo_ensemble_gae
// without pack workgroups.  The stacked gradient layout is
// w1 [M][..] | b1 [M][..] | ... | wL | bL | wa | ba | wc | bc, each segment
// member-major: seg[t] is the single-model size of tensor t (2 L + 4 of them).
struct DeepPpoEnsembleArgs {
  DeepPpoArgs p;
  float* values;  // [M][n]
  int members, blocks;  // blocks: grads blocks (= partial rows) per member
  int seg[2 * kDeepMaxLayers + 4];
  float* grad;
};

__device__ __forceinline__ DeepPpoArgs deep_ppo_member(const DeepPpoEnsembleArgs& a, size_t mi) {
  DeepPpoArgs p = a.p;
  const size_t n = (size_t)p.n;
  p.x += mi * n * p.d;
  const int last = deep_member_net(p.net, mi, p.d, p.k);
  p.wc += mi * (size_t)last;
  p.bc += mi;
  p.actions += mi * n;
  p.old_logp += mi * n;
  p.adv += mi * n;
  p.dvalue += mi * n;
  p.gae_part += mi * 2 * (size_t)p.n_part;
  p.partial += mi * (size_t)a.blocks * p.size;
  return p;
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_ppo_deep_ensemble_values(DeepPpoEnsembleArgs a) {
  // a.p.net stays in place (its arrays are indexed by the layer loop)
  const size_t mi = blockIdx.y, n = (size_t)a.p.n;
  const int last = a.p.net.width[a.p.net.n_hidden - 1];
  deep_ppo_values_body<NW>(a.p.x + mi * n * a.p.d, a.p.n, a.p.d, a.p.net,
                           a.p.wc + mi * (size_t)last, a.p.bc + mi, a.values + mi * n, mi);
}

template <int K, bool L3>
__global__ __launch_bounds__(512) void k_ppo_deep_ensemble_grads(DeepPpoEnsembleArgs a) {
  extern __shared__ __align__(16) float deep_lds[];
  const DeepPpoArgs p = deep_ppo_member(a, blockIdx.y);
  deep_ppo_grads_body<K, L3>(p, deep_lds);
}

// Member blockIdx.y's block partials -> its rows of the stacked gradient.
__global__ __launch_bounds__(1024) void k_ppo_deep_ensemble_reduce(DeepPpoEnsembleArgs a) {
  const size_t mi = blockIdx.y, M = (size_t)a.members;
  const int size = a.p.size;
  float* grad = a.grad;
  ppo_reduce_body(a.p.partial + mi * (size_t)a.blocks * size, a.blocks, size,
                  [&](int p, float g) {
                    int lo = 0, len = a.seg[0];  // p's tensor: parameters [lo, lo + len)
#pragma unroll
                    for (int t = 1; t < 2 * kDeepMaxLayers + 4; ++t) {
                      if (p >= lo + len) {
                        lo += len;
                        len = a.seg[t];
                      }
                    }
                    grad[M * lo + mi * len + (p - lo)] = g;
                  });
}

}  // namespace swarm
