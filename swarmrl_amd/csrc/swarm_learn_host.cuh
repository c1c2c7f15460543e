// swarm_learn_host.cuh -- the host launch layer of the learner entry points:
// the policy samplers and the PPO epoch gradients of the one-layer MLP, the
// deep MLPs and their ensembles ("Host launch layer").
//
// Part of swarm_engine.hip's translation unit, included after the engine:
// policy_launch needs swarm_engine, flush_ride_along, flush_check,
// build_lds_bytes and k_policy_cbuild; everything here uses fail and HIP_TRY.
//
// Every decision that fixes a result's bits is taken in one place:
//   ppo_variant / mlp_variant / deep_variant   the template widths of a shape
//   ppo_plan        coop, the grads grid (= the summation order), the table
//   learn_workspace the slices of a caller's workspace
//   deep_fill       the layers and the gradient layout of a deep network
//   allow_lds       dynamic LDS above 64 KB
// and the single-model and ensemble entry points of a family both call it.
#pragma once

#include <mutex>
#include <type_traits>

#include "swarm_select.h"

namespace {

using swarm_select::Int;

// ---- argument checks (null: within the limits)

const char* mlp_limits(int32_t d_in, int32_t hidden, int32_t k) {
  if (d_in < 1 || d_in > swarm::kMlpMaxIn) return "1 <= d_in <= 16";
  if (hidden < 1 || hidden > swarm::kMlpMaxHidden) return "1 <= hidden <= 256";
  if (k < 1 || k > swarm::kMlpMaxActions) return "1 <= k <= 16 actions";
  return nullptr;
}

const char* ppo_limits(int32_t d_in, int32_t hidden, int32_t k) {
  if (d_in < 1 || d_in > swarm::kPpoMaxIn) return "1 <= d_in <= 32";
  if (hidden < 1 || hidden > swarm::kPpoMaxHidden) return "1 <= hidden <= 256";
  if (k < 1 || k > swarm::kPpoMaxK) return "1 <= k <= 16 actions";
  return nullptr;
}

// The limits of the deep kernels (swarm_deep.cuh).
const char* deep_limits(int32_t d_in, int32_t n_hidden, const int32_t* widths, int32_t k) {
  if (n_hidden < swarm::kDeepMinLayers || n_hidden > swarm::kDeepMaxLayers)
    return "2 <= n_hidden <= 3 hidden layers";
  if (d_in < 1 || d_in > swarm::kDeepMaxIn) return "1 <= d_in <= 32";
  if (k < 1 || k > swarm::kDeepMaxActions) return "1 <= k <= 16 actions";
  for (int l = 0; l < n_hidden; ++l)
    if (widths[l] < 1 || widths[l] > swarm::kDeepMaxWidth) return "1 <= hidden width <= 128";
  return nullptr;
}

const char* members_limit(int32_t M) {
  return M < 1 || M > swarm::kEnsembleMaxMembers ? "1 <= n_members <= 1024" : nullptr;
}

// An ensemble epoch: the members and a member's samples.
const char* ensemble_limits(int32_t M, int32_t T, int32_t S) {
  if (const char* why = members_limit(M)) return why;
  if ((long)T * S > INT32_MAX) return "T x S < 2^31 samples per member";
  return nullptr;
}

// The tail of every sampler's checks; n, n_state per member for an ensemble.
// *go: there are agents to sample for.
int sampler_check(float explore_p, int32_t n, int32_t n_state, bool per_member, bool* go) {
  *go = false;
  if (!(explore_p >= 0.0f && explore_p <= 1.0f))
    return fail(SWARM_EINVAL, "exploration probability must be in [0, 1]");
  if (n <= 0) return SWARM_OK;
  if (n_state < (n + 63) / 64)
    return fail(SWARM_EINVAL, per_member ? "state needs ceil(n_per / 64) counters per member"
                                         : "state needs ceil(n / 64) counters");
  *go = true;
  return SWARM_OK;
}

// ---- the template widths of a shape; f returns a status

// k_ppo_*: NW waves of 128 hidden units, D inputs, K actions.
template <class F>
int ppo_variant(int hidden, int d_in, int k, F&& f) {
  auto cell = [&](auto NN) -> int {
    if (d_in == 1 && k <= 4) return f(NN, Int<1>{}, Int<4>{});
    if (d_in <= 4 && k <= 4) return f(NN, Int<4>{}, Int<4>{});
    if (d_in <= 4) return f(NN, Int<4>{}, Int<16>{});
    if (d_in <= 16 && k <= 4) return f(NN, Int<16>{}, Int<4>{});
    if (d_in <= 16) return f(NN, Int<16>{}, Int<16>{});
    if (k <= 4) return f(NN, Int<32>{}, Int<4>{});
    return f(NN, Int<32>{}, Int<16>{});
  };
  return hidden <= 128 ? cell(Int<1>{}) : cell(Int<2>{});
}

// k_ppo_grads of a plan: NT tile waves, and whether they share each tile.
template <int NN, class F>
int ppo_grads_variant(bool coop, F&& f) {
  constexpr int TT = NN == 1 ? 4 : 1;
  if constexpr (NN == 1)
    if (coop) return f(Int<TT>{}, std::true_type{});
  return f(Int<TT>{}, std::false_type{});
}

// k_policy_*_sample: G lanes per agent (n agents, a member's for an ensemble),
// D inputs, K actions.  G fixes the order of the hidden-unit sum, so the
// logits' bits: enough waves to cover the SIMDs when agents are few.
template <class F>
int mlp_variant(int n, int d_in, int k, F&& f) {
  auto cell = [&](auto GG) -> int {
    if (d_in <= 4 && k <= 4) return f(GG, Int<4>{}, Int<4>{});
    if (d_in <= 4) return f(GG, Int<4>{}, Int<16>{});
    if (k <= 4) return f(GG, Int<16>{}, Int<4>{});
    return f(GG, Int<16>{}, Int<16>{});
  };
  return n <= 16384 ? cell(Int<4>{}) : (n <= 65536 ? cell(Int<2>{}) : cell(Int<1>{}));
}

template <int D, int K>
size_t mlp_lds_bytes(int hidden) {
  return (size_t)(hidden * swarm::MlpRow<D, K>::kStride + K) * sizeof(float);
}

// k_ppo_deep_*grads: K actions, three hidden layers or two.
template <class F>
int deep_variant(int k, int n_hidden, F&& f) {
  const bool three = n_hidden == 3;
  if (k <= 4 && !three) return f(Int<4>{}, std::false_type{});
  if (k <= 4) return f(Int<4>{}, std::true_type{});
  if (!three) return f(Int<16>{}, std::false_type{});
  return f(Int<16>{}, std::true_type{});
}

// ---- dynamic LDS

// `lds` bytes of dynamic LDS for kernel `fn`: above 64 KB it has to be
// allowed, once per (kernel, device).  Not a stream operation, so a call under
// stream capture is safe.
int allow_lds(const void* fn, int lds) {
  if (lds <= 65536) return SWARM_OK;
  int dev = -1;
  HIP_TRY(hipGetDevice(&dev));
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> allowed;
  const std::lock_guard<std::mutex> lock(mu);
  const std::pair<const void*, int> key(fn, dev);
  if (std::find(allowed.begin(), allowed.end(), key) != allowed.end()) return SWARM_OK;
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  allowed.push_back(key);
  return SWARM_OK;
}

// ---- workspaces

// Bump allocator over a caller's workspace, slices aligned to 256 bytes.
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t off = at;
    at += (bytes + 255) & ~(size_t)255;
    return off;
  }
  size_t total() const { return at; }
};

// The workspace of an epoch of M members (1: a single model), member-major
// slices: values | adv | dv [M][n], GAE partials [M][2 gae_blocks] (fp64),
// parameter tables [M][table_floats] (none for a deep net), block partials
// [M][partial_floats], the Adam ticket (swarm_ppo_epoch_step only).
struct LearnWorkspace {
  size_t values, adv, dv, spart, table, partial, ticket, total;
};
LearnWorkspace learn_workspace(size_t M, size_t n, size_t S, size_t table_floats,
                               size_t partial_floats, size_t ticket_bytes) {
  Carve c;
  LearnWorkspace w;
  w.values = c.take(M * n * 4);
  w.adv = c.take(M * n * 4);
  w.dv = c.take(M * n * 4);
  w.spart = c.take(M * ((S + 255) / 256) * 2 * sizeof(double));
  w.table = c.take(M * table_floats * 4);
  w.partial = c.take(M * partial_floats * 4);
  w.ticket = c.take(ticket_bytes);
  w.total = c.total();
  return w;
}

template <class T>
T* slice(void* workspace, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(workspace) + off);
}

// A single one-layer model reserves for every shape within the limits: unit
// rows of at most 256 units x PpoTable<32, 16>::kStride floats, kPpoBlocks
// partial rows and the ticket.
LearnWorkspace ppo_workspace(long n, long S, int d, int hidden, int k) {
  return learn_workspace(1, (size_t)n, (size_t)S,
                         (size_t)swarm::kPpoMaxHidden * swarm::PpoTable<32, 16>::kStride,
                         (size_t)swarm::kPpoBlocks * swarm::ppo_grad_size(d, hidden, k), 4);
}

int deep_ppo_blocks(long n) {
  return (int)std::min<long>((n + swarm::kDeepAgents - 1) / swarm::kDeepAgents,
                             swarm::kDeepPpoBlocks);
}

// Partial rows sized by the blocks a member launches.
LearnWorkspace deep_ppo_workspace(size_t M, long n, long S, int size) {
  return learn_workspace(M, (size_t)n, (size_t)S, 0, (size_t)deep_ppo_blocks(n) * (size_t)size, 0);
}

// ---- the one-layer epoch

// Workgroups of `fn` resident at once on a whole MI355X (256 CUs).  The grid
// size sets the fixed cross-block summation order of the gradient, so it is
// a function of the kernel and n only -- never of the device it runs on or
// its partition mode: replicas on any GPUs sum in the same order and stay
// bit-identical.
constexpr int kPpoOrderCUs = 256;
int ppo_resident_blocks(const void* fn, int threads, size_t lds) {
  const int cus = kPpoOrderCUs;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  return std::max(1, per_cu * cus);
}

// Every decision of an epoch over n = T * S samples (a member's own n for an
// ensemble, whose grads kernel runs the single-model body on the same grid).
struct PpoPlan {
  int rc;            // SWARM_OK, or the LDS allowance failed
  bool coop;         // fewer tiles than 4 per grads block: the 4 waves share each tile
  int blocks;        // grads blocks = partial rows (per member)
  int table_rows;    // the parameter table (per member): unit rows,
  int table_floats;  // floats
  int lds;           // bytes of dynamic LDS of the grads kernel
};

template <int NN, int DD, int KK>
PpoPlan ppo_plan(long n) {
  // k_ppo_grads: tiles of 128 samples; hidden <= 128: blocks of 4 tile waves
  // (TT), else 2 unit waves (NN); every block writes its partial row and the
  // reduce reads exactly the rows written
  constexpr int TT = NN == 1 ? 4 : 1;
  const long tiles128 = (n + 127) / 128;
  PpoPlan pl{};
  pl.coop = NN == 1 && tiles128 < 4L * swarm::kPpoBlocks;
  pl.blocks = (int)std::min<long>(pl.coop ? tiles128 : (tiles128 + TT - 1) / TT,
                                  swarm::kPpoBlocks);
  pl.table_rows = 128 * NN;
  pl.table_floats = pl.table_rows * swarm::PpoTable<DD, KK>::kStride;
  if (pl.coop) {
    pl.lds = swarm::ppo_grads_lds_floats<NN, TT, NN == 1, DD, KK>() * (int)sizeof(float);
    return pl;
  }
  // no more blocks than are resident at once: a second round of blocks would
  // leave most SIMDs idle for its tail.  The LDS allowance comes first: a
  // refused query falls back to one block per CU -- another grid, other bits
  const void* fn = reinterpret_cast<const void*>(&swarm::k_ppo_grads<NN, TT, false, DD, KK>);
  pl.lds = swarm::ppo_grads_lds_floats<NN, TT, false, DD, KK>() * (int)sizeof(float);
  pl.rc = allow_lds(fn, pl.lds);
  if (pl.rc == SWARM_OK)
    pl.blocks = std::min(pl.blocks, ppo_resident_blocks(fn, 64 * NN * TT, (size_t)pl.lds));
  return pl;
}

// swarm_ppo_profile: HIP events around every k_ppo_grads launch of this
// thread (bench.py's roofline of the update); not under graph capture.
struct PpoProfile {
  bool on = false;
  int reps = 1;  // back-to-back k_ppo_grads launches per epoch while timing
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};
thread_local PpoProfile g_ppo_prof;

// k_ppo_gae_ep of a shape's variant (defined after every other launch of this
// file: its instantiations come last in the code object).
int launch_gae_ep(int hidden, int d_in, int k, dim3 grid, hipStream_t s, const float* rewards,
                  const float* values, int T, int S, float gamma, float lambda, float* adv,
                  float* dv, double* spart, int gae_blocks, const swarm::PpoPack& pk,
                  const uint8_t* dones, int per_env);

// dones [T][S / per_env] of the *_ep entries: whole envs only.
const char* dones_limits(int32_t S, int32_t per_env) {
  if (per_env < 1 || S % per_env != 0) return "per_env must be >= 1 and divide S";
  return nullptr;
}

// V of every sample, GAE + dL/dV (+ the table), the gradients, their reduce
// (with adam: the optimizer step fused into it).  dones non-null: the GAE
// across episode ends (k_ppo_gae_ep).
int ppo_epoch(const float* x, int32_t T, int32_t S, int32_t d_in, const int64_t* actions,
              const float* old_logp, const float* rewards, const float* w1, const float* b1,
              int32_t hidden, const float* wa, const float* ba, int32_t k, const float* wc,
              const float* bc, float gamma, float lambda, float clip_eps, float entropy_coef,
              void* workspace, int64_t workspace_bytes, float* grad, void* stream,
              const swarm_adam_t* adam, const uint8_t* dones = nullptr, int32_t per_env = 1) {
  if (!x || !actions || !old_logp || !rewards || !w1 || !b1 || !wa || !ba || !wc || !bc ||
      !workspace || !grad)
    return fail(SWARM_EINVAL, "null argument");
  if (T < 1 || S < 1) return fail(SWARM_EINVAL, "T, S >= 1");
  if (dones)
    if (const char* why = dones_limits(S, per_env)) return fail(SWARM_EINVAL, why);
  if ((long)T * S > INT32_MAX) return fail(SWARM_ECAPACITY, "T x S < 2^31 samples");
  if (const char* why = ppo_limits(d_in, hidden, k)) return fail(SWARM_ECAPACITY, why);
  const int n = T * S;
  const LearnWorkspace ws = ppo_workspace(n, S, d_in, hidden, k);
  if (workspace_bytes < (int64_t)ws.total)
    return fail(SWARM_EINVAL, "workspace smaller than swarm_ppo_workspace_bytes");
  float* values = slice<float>(workspace, ws.values);
  float* adv = slice<float>(workspace, ws.adv);
  float* dv = slice<float>(workspace, ws.dv);
  double* spart = slice<double>(workspace, ws.spart);
  float* table = slice<float>(workspace, ws.table);
  float* partial = slice<float>(workspace, ws.partial);
  const int gae_blocks = (S + 255) / 256;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  PpoPlan pl{};
  const int rc = ppo_variant(hidden, d_in, k, [&](auto NN_, auto DD_, auto KK_) -> int {
    constexpr int NN = NN_, DD = DD_, KK = KK_;
    pl = ppo_plan<NN, DD, KK>(n);
    if (pl.rc) return pl.rc;
    if (n < (1 << 20))  // 64 samples a block
      hipLaunchKernelGGL((swarm::k_ppo_values_split<DD>), dim3((unsigned)(((long)n + 63) / 64)),
                         dim3(256), 0, s, x, n, d_in, w1, b1, hidden, wc, bc, values);
    else  // 4 samples a thread
      hipLaunchKernelGGL((swarm::k_ppo_values<DD>), dim3((unsigned)(((n + 3) / 4 + 255) / 256)),
                         dim3(256), 0, s, x, n, d_in, w1, b1, hidden, wc, bc, values);
    const swarm::PpoPack pk{w1, b1, wa, wc, d_in, hidden, k, pl.table_rows, table};
    const dim3 ggrid((unsigned)(gae_blocks + (pl.table_floats + 255) / 256));
    if (dones) {
      if (const int grc = launch_gae_ep(hidden, d_in, k, ggrid, s, rewards, values, T, S, gamma,
                                        lambda, adv, dv, spart, gae_blocks, pk, dones, per_env))
        return grc;
    } else if (T <= 32)
      hipLaunchKernelGGL((swarm::k_ppo_gae<32, DD, KK>), ggrid, dim3(256), 0, s, rewards, values,
                         T, S, gamma, lambda, adv, dv, spart, gae_blocks, pk);
    else
      hipLaunchKernelGGL((swarm::k_ppo_gae<0, DD, KK>), ggrid, dim3(256), 0, s, rewards, values,
                         T, S, gamma, lambda, adv, dv, spart, gae_blocks, pk);
    return ppo_grads_variant<NN>(pl.coop, [&](auto TT_, auto CO_) -> int {
      constexpr int TT = TT_;
      constexpr bool CO = CO_;
      const int arc = allow_lds(
          reinterpret_cast<const void*>(&swarm::k_ppo_grads<NN, TT, CO, DD, KK>), pl.lds);
      if (arc) return arc;
      hipEvent_t ev0 = nullptr, ev1 = nullptr;
      if (g_ppo_prof.on && hipEventCreate(&ev0) == hipSuccess &&
          hipEventCreate(&ev1) == hipSuccess)
        (void)hipEventRecord(ev0, s);
      for (int rep = 0; rep < (ev1 ? g_ppo_prof.reps : 1); ++rep)  // same partial rows
        hipLaunchKernelGGL((swarm::k_ppo_grads<NN, TT, CO, DD, KK>), dim3((unsigned)pl.blocks),
                           dim3(64 * NN * TT), (size_t)pl.lds, s, x, n, d_in, w1, b1, hidden, wa,
                           ba, k, wc, bc, actions, old_logp, adv, dv, spart, gae_blocks, table,
                           clip_eps, entropy_coef, partial);
      if (ev1) {
        (void)hipEventRecord(ev1, s);
        g_ppo_prof.ev.emplace_back(ev0, ev1);
      }
      return SWARM_OK;
    });
  });
  if (rc) return rc;
  const int size = swarm::ppo_grad_size(d_in, hidden, k);
  const dim3 rgrid((unsigned)((size + 63) / 64));
  if (adam) {
    swarm::AdamArgs a;
    a.lr = adam->lr;
    a.beta1 = adam->beta1;
    a.beta2 = adam->beta2;
    a.eps = adam->eps;
    const int sizes[6] = {hidden * d_in, hidden, k * hidden, k, hidden, 1};
    a.seg[0] = 0;
    for (int t = 0; t < 6; ++t) {
      if (!adam->param[t] || !adam->exp_avg[t] || !adam->exp_avg_sq[t] || !adam->step[t])
        return fail(SWARM_EINVAL, "null Adam tensor");
      a.param[t] = adam->param[t];
      a.m[t] = adam->exp_avg[t];
      a.v[t] = adam->exp_avg_sq[t];
      a.step[t] = adam->step[t];
      a.seg[t + 1] = a.seg[t] + sizes[t];
    }
    hipLaunchKernelGGL(swarm::k_ppo_reduce_adam, rgrid, dim3(1024), 0, s, partial, pl.blocks, size,
                       grad, a, slice<uint32_t>(workspace, ws.ticket));
  } else {
    hipLaunchKernelGGL(swarm::k_ppo_reduce, rgrid, dim3(1024), 0, s, partial, pl.blocks, size,
                       grad);
  }
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// The plan of a shape's variant, for the ensemble path (ppo_epoch plans
// inside its own dispatch).
PpoPlan ppo_plan_for(long n, int d_in, int hidden, int k) {
  PpoPlan pl{};
  ppo_variant(hidden, d_in, k, [&](auto NN, auto DD, auto KK) -> int {
    pl = ppo_plan<NN, DD, KK>(n);
    return pl.rc;
  });
  return pl;
}

// An ensemble's table and partial rows are sized by what a member launches.
LearnWorkspace ppo_ensemble_workspace(size_t M, size_t n, size_t S, int size, const PpoPlan& pl) {
  return learn_workspace(M, n, S, (size_t)pl.table_floats, (size_t)pl.blocks * (size_t)size, 0);
}

// ---- deep networks

// The hidden layers and actor head of a deep net into p.net, its gradient
// layout w1 | b1 | ... | wL | bL | wa | ba | wc | bc into p.off_* and p.size,
// and (seg non-null) the 2 L + 4 tensor sizes.  w null: the layout alone.
// False: a layer's parameters are null.
bool deep_fill(int d_in, int n_hidden, const int32_t* widths, const float* const* w,
               const float* const* b, const float* wa, const float* ba, int k,
               swarm::DeepPpoArgs& p, int* seg) {
  int nseg = 0, off = 0, prev = d_in;
  auto tensor = [&](int len) {  // the next tensor of the layout: its offset
    const int at = off;
    if (seg) seg[nseg++] = len;
    off += len;
    return at;
  };
  p.net.n_hidden = n_hidden;
  for (int l = 0; l < n_hidden; ++l) {
    if (w) {
      if (!w[l] || !b[l]) return false;
      p.net.w[l] = w[l];
      p.net.b[l] = b[l];
    }
    p.net.width[l] = widths[l];
    p.off_w[l] = tensor(widths[l] * prev);
    p.off_b[l] = tensor(widths[l]);
    prev = widths[l];
  }
  p.net.wa = wa;
  p.net.ba = ba;
  p.off_wa = tensor(k * prev);
  p.off_ba = tensor(k);
  p.off_wc = tensor(prev);
  p.off_bc = tensor(1);
  p.size = off;
  return true;
}

int deep_ppo_grad_size(int d_in, int n_hidden, const int32_t* widths, int k) {
  swarm::DeepPpoArgs p{};
  deep_fill(d_in, n_hidden, widths, nullptr, nullptr, nullptr, nullptr, k, p, nullptr);
  return p.size;
}

// The data and workspace slices of a deep epoch (member 0's for an ensemble).
void deep_ppo_bind(swarm::DeepPpoArgs& p, const float* x, int n, int d_in, int k, const float* wc,
                   const float* bc, const int64_t* actions, const float* old_logp, int gae_blocks,
                   float clip_eps, float entropy_coef, void* workspace,
                   const LearnWorkspace& ws) {
  p.x = x;
  p.n = n;
  p.d = d_in;
  p.k = k;
  p.wc = wc;
  p.bc = bc;
  p.actions = actions;
  p.old_logp = old_logp;
  p.adv = slice<float>(workspace, ws.adv);
  p.dvalue = slice<float>(workspace, ws.dv);
  p.gae_part = slice<double>(workspace, ws.spart);
  p.n_part = gae_blocks;
  p.clip_eps = clip_eps;
  p.c_ent = entropy_coef;
  p.partial = slice<float>(workspace, ws.partial);
}

// ---- the rollout policy of the one-layer MLP

// swarm_policy_mlp_sample; ride: the engine whose deferred build's last stage
// (the cluster build) rides along as extra workgroups of the same launch
// (k_policy_cbuild), or null.
int policy_launch(const float* obs, int32_t n, int32_t d_in, const float* w1, const float* b1,
                  int32_t hidden, const float* w2, const float* b2, int32_t k, uint64_t seed,
                  uint64_t* state, int32_t n_state, float explore_p, const float* f_table,
                  const float* t_table, int64_t* out_idx, float* out_logp, float* out_f,
                  float* out_t, float* out_logits, void* stream, swarm_engine* ride) {
  if (!obs || !w1 || !b1 || !w2 || !b2 || !state || !f_table || !t_table || !out_idx ||
      !out_logp || !out_f || !out_t)
    return fail(SWARM_EINVAL, "null argument");
  if (const char* why = mlp_limits(d_in, hidden, k)) return fail(SWARM_ECAPACITY, why);
  bool go;
  if (const int rc = sampler_check(explore_p, n, n_state, false, &go); rc || !go) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const swarm::MlpArgs m{obs, n, d_in, w1, b1, hidden, w2, b2, k, (uint32_t)seed,
                         (uint32_t)(seed >> 32), reinterpret_cast<unsigned long long*>(state),
                         explore_p, f_table, t_table, out_idx, out_logp, out_f, out_t, out_logits};
  return mlp_variant(n, d_in, k, [&](auto GG_, auto DD_, auto KK_) -> int {
    constexpr int GG = GG_, DD = DD_, KK = KK_;
    // the build stage may only ride along on the engine's stream: stages 1-2
    // and the run that consumes the build are ordered on it
    if constexpr (GG == 4 && DD == 4 && KK == 4) {
      if (ride && s == ride->stream && ride->ride_stage == 3) {
        // policy blocks of 1024 threads (256 agents: whole counter groups) and
        // one cluster-build workgroup per env
        const int pblocks = (int)(((long)n * GG + 1023) / 1024);
        const size_t lds = std::max(mlp_lds_bytes<DD, KK>(hidden),
                                    build_lds_bytes(ride->n, ride->sc.pair_cap));
        hipLaunchKernelGGL((k_policy_cbuild<GG, DD, KK>), dim3((unsigned)(pblocks + ride->n_envs)),
                           dim3(1024), lds, s, m, ride->n_envs, ride->st, ride->sc);
        HIP_TRY(hipGetLastError());
        ride->ride_stage = 0;
        ride->prebuilt = true;
        return SWARM_OK;
      }
    }
    if (ride && ride->ride_stage > 0) {
      const int rc = flush_ride_along(ride);
      if (rc) return rc;
    }
    const size_t lds = mlp_lds_bytes<DD, KK>(hidden);
    hipLaunchKernelGGL((swarm::k_policy_mlp_sample<GG, DD, KK>),
                       dim3((unsigned)(((long)n * GG + 255) / 256)), dim3(256), lds, s, m);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  });
}

}  // namespace

// ---- entry points: samplers

int swarm_sample_actions(const float* logits, int32_t n, int32_t k, uint64_t seed,
                         uint64_t* state, int32_t n_state, float explore_p,
                         const float* f_table, const float* t_table, int64_t* out_idx,
                         float* out_logp, float* out_f, float* out_t, void* stream) {
  if (!logits || !state || !f_table || !t_table || !out_idx || !out_logp || !out_f || !out_t)
    return fail(SWARM_EINVAL, "null argument");
  if (k < 1 || k > swarm::kMaxActions) return fail(SWARM_ECAPACITY, "1 <= k <= 64 actions");
  bool go;
  if (const int rc = sampler_check(explore_p, n, n_state, false, &go); rc || !go) return rc;
  hipLaunchKernelGGL(swarm::k_sample_actions, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), logits, n, k, (uint32_t)seed,
                     (uint32_t)(seed >> 32), reinterpret_cast<unsigned long long*>(state),
                     explore_p, f_table, t_table, out_idx, out_logp, out_f, out_t);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int swarm_policy_mlp_sample(const float* obs, int32_t n, int32_t d_in, const float* w1,
                            const float* b1, int32_t hidden, const float* w2, const float* b2,
                            int32_t k, uint64_t seed, uint64_t* state, int32_t n_state,
                            float explore_p, const float* f_table, const float* t_table,
                            int64_t* out_idx, float* out_logp, float* out_f, float* out_t,
                            float* out_logits, void* stream) {
  return policy_launch(obs, n, d_in, w1, b1, hidden, w2, b2, k, seed, state, n_state, explore_p,
                       f_table, t_table, out_idx, out_logp, out_f, out_t, out_logits, stream,
                       nullptr);
}

int swarm_engine_policy_mlp_sample(swarm_engine_t* e, const float* obs, int32_t n, int32_t d_in,
                                   const float* w1, const float* b1, int32_t hidden,
                                   const float* w2, const float* b2, int32_t k, uint64_t seed,
                                   uint64_t* state, int32_t n_state, float explore_p,
                                   const float* f_table, const float* t_table, int64_t* out_idx,
                                   float* out_logp, float* out_f, float* out_t, float* out_logits,
                                   void* stream) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  return policy_launch(obs, n, d_in, w1, b1, hidden, w2, b2, k, seed, state, n_state, explore_p,
                       f_table, t_table, out_idx, out_logp, out_f, out_t, out_logits, stream, e);
}

int swarm_policy_deep_sample(const float* obs, int32_t n, int32_t d_in, int32_t n_hidden,
                             const int32_t* widths, const float* const* w, const float* const* b,
                             const float* wa, const float* ba, int32_t k, uint64_t seed,
                             uint64_t* state, int32_t n_state, float explore_p,
                             const float* f_table, const float* t_table, int64_t* out_idx,
                             float* out_logp, float* out_f, float* out_t, float* out_logits,
                             void* stream) {
  if (!obs || !widths || !w || !b || !wa || !ba || !state || !f_table || !t_table || !out_idx ||
      !out_logp || !out_f || !out_t)
    return fail(SWARM_EINVAL, "null argument");
  if (const char* why = deep_limits(d_in, n_hidden, widths, k)) return fail(SWARM_ECAPACITY, why);
  swarm::DeepPpoArgs p{};
  if (!deep_fill(d_in, n_hidden, widths, w, b, wa, ba, k, p, nullptr))
    return fail(SWARM_EINVAL, "null parameter");
  bool go;
  if (const int rc = sampler_check(explore_p, n, n_state, false, &go); rc || !go) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const swarm::MlpArgs m{obs,     n,       d_in,     nullptr, nullptr, 0,     nullptr,
                         nullptr, k,       (uint32_t)seed, (uint32_t)(seed >> 32),
                         reinterpret_cast<unsigned long long*>(state), explore_p, f_table,
                         t_table, out_idx, out_logp, out_f,   out_t,   out_logits};
  const unsigned blocks = (unsigned)((n + swarm::kDeepAgents - 1) / swarm::kDeepAgents);
  if (k <= 4)
    hipLaunchKernelGGL(swarm::k_policy_deep_sample<4>, dim3(blocks), dim3(256), 0, s, m, p.net);
  else
    hipLaunchKernelGGL(swarm::k_policy_deep_sample<16>, dim3(blocks), dim3(256), 0, s, m, p.net);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// ---- entry points: the epoch of a single model

int64_t swarm_ppo_workspace_bytes(int32_t T, int32_t S, int32_t d_in, int32_t hidden,
                                  int32_t k) {
  if (T < 1 || S < 1 || d_in < 1 || hidden < 1 || k < 1) return -1;
  return (int64_t)ppo_workspace((long)T * S, S, d_in, hidden, k).total;
}

int swarm_ppo_profile(int32_t enable, double* grads_ms, int32_t* launches) {
  int32_t pairs = 0;
  const int rc = read_event_pairs(g_ppo_prof.ev, grads_ms, &pairs);
  if (launches) *launches = pairs * g_ppo_prof.reps;
  g_ppo_prof.reps = enable > 0 ? enable : 1;
  g_ppo_prof.on = enable > 0;
  return rc;
}

int swarm_ppo_epoch_grad(const float* x, int32_t T, int32_t S, int32_t d_in,
                         const int64_t* actions, const float* old_logp, const float* rewards,
                         const float* w1, const float* b1, int32_t hidden, const float* wa,
                         const float* ba, int32_t k, const float* wc, const float* bc,
                         float gamma, float lambda, float clip_eps, float entropy_coef,
                         void* workspace, int64_t workspace_bytes, float* grad, void* stream) {
  return ppo_epoch(x, T, S, d_in, actions, old_logp, rewards, w1, b1, hidden, wa, ba, k, wc, bc,
                   gamma, lambda, clip_eps, entropy_coef, workspace, workspace_bytes, grad, stream,
                   nullptr);
}

int swarm_ppo_epoch_step(const float* x, int32_t T, int32_t S, int32_t d_in,
                         const int64_t* actions, const float* old_logp, const float* rewards,
                         int32_t hidden, int32_t k, float gamma, float lambda, float clip_eps,
                         float entropy_coef, const swarm_adam_t* adam, void* workspace,
                         int64_t workspace_bytes, float* grad, void* stream) {
  if (!adam) return fail(SWARM_EINVAL, "null argument");
  if (!(adam->beta1 >= 0.0f && adam->beta1 < 1.0f && adam->beta2 >= 0.0f && adam->beta2 < 1.0f))
    return fail(SWARM_EINVAL, "Adam betas must be in [0, 1)");
  return ppo_epoch(x, T, S, d_in, actions, old_logp, rewards, adam->param[0], adam->param[1],
                   hidden, adam->param[2], adam->param[3], k, adam->param[4], adam->param[5],
                   gamma, lambda, clip_eps, entropy_coef, workspace, workspace_bytes, grad, stream,
                   adam);
}

int64_t swarm_ppo_deep_workspace_bytes(int32_t T, int32_t S, int32_t d_in, int32_t n_hidden,
                                       const int32_t* widths, int32_t k) {
  if (T < 1 || S < 1 || !widths || deep_limits(d_in, n_hidden, widths, k)) return -1;
  if ((long)T * S > INT32_MAX) return -1;
  return (int64_t)deep_ppo_workspace(1, (long)T * S, S,
                                     deep_ppo_grad_size(d_in, n_hidden, widths, k)).total;
}

namespace {

// swarm_ppo_deep_epoch_grad, and with dones its _ep sibling.
int deep_ppo_epoch(const float* x, int32_t T, int32_t S, int32_t d_in, const int64_t* actions,
                   const float* old_logp, const float* rewards, int32_t n_hidden,
                   const int32_t* widths, const float* const* w, const float* const* b,
                   const float* wa, const float* ba, int32_t k, const float* wc, const float* bc,
                   float gamma, float lambda, float clip_eps, float entropy_coef, void* workspace,
                   int64_t workspace_bytes, float* grad, void* stream, const uint8_t* dones,
                   int32_t per_env) {
  if (!x || !actions || !old_logp || !rewards || !widths || !w || !b || !wa || !ba || !wc ||
      !bc || !workspace || !grad)
    return fail(SWARM_EINVAL, "null argument");
  if (T < 1 || S < 1) return fail(SWARM_EINVAL, "T, S >= 1");
  if ((long)T * S > INT32_MAX) return fail(SWARM_ECAPACITY, "T x S < 2^31 samples");
  if (const char* why = deep_limits(d_in, n_hidden, widths, k)) return fail(SWARM_ECAPACITY, why);
  if (dones)
    if (const char* why = dones_limits(S, per_env)) return fail(SWARM_EINVAL, why);
  swarm::DeepPpoArgs p{};
  if (!deep_fill(d_in, n_hidden, widths, w, b, wa, ba, k, p, nullptr))
    return fail(SWARM_EINVAL, "null parameter");
  const int n = T * S;
  const LearnWorkspace ws = deep_ppo_workspace(1, n, S, p.size);
  if (workspace_bytes < (int64_t)ws.total)
    return fail(SWARM_EINVAL, "workspace smaller than swarm_ppo_deep_workspace_bytes");
  const int gae_blocks = (S + 255) / 256;
  deep_ppo_bind(p, x, n, d_in, k, wc, bc, actions, old_logp, gae_blocks, clip_eps, entropy_coef,
                workspace, ws);
  float* values = slice<float>(workspace, ws.values);
  float* adv = slice<float>(workspace, ws.adv);
  float* dv = slice<float>(workspace, ws.dv);
  double* spart = slice<double>(workspace, ws.spart);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned tiles = (unsigned)(((long)n + swarm::kDeepAgents - 1) / swarm::kDeepAgents);
  const int blocks = deep_ppo_blocks(n);
  hipLaunchKernelGGL(swarm::k_ppo_deep_values<8>, dim3(tiles), dim3(512), 0, s, x, n, d_in, p.net,
                     wc, bc, values);
  // k_ppo_gae as it stands, without pack workgroups (n_gae = its grid)
  const swarm::PpoPack none{};
  if (dones) {
    if (const int grc = launch_gae_ep(1, 1, 4, dim3((unsigned)gae_blocks), s, rewards, values, T,
                                      S, gamma, lambda, adv, dv, spart, gae_blocks, none, dones,
                                      per_env))
      return grc;
  } else if (T <= 32)
    hipLaunchKernelGGL((swarm::k_ppo_gae<32, 1, 4>), dim3((unsigned)gae_blocks), dim3(256), 0, s,
                       rewards, values, T, S, gamma, lambda, adv, dv, spart, gae_blocks, none);
  else
    hipLaunchKernelGGL((swarm::k_ppo_gae<0, 1, 4>), dim3((unsigned)gae_blocks), dim3(256), 0, s,
                       rewards, values, T, S, gamma, lambda, adv, dv, spart, gae_blocks, none);
  const int rc = deep_variant(k, n_hidden, [&](auto KK_, auto L3_) -> int {
    constexpr int KK = KK_;
    constexpr bool L3 = L3_;
    const int lds = swarm::deep_grads_lds_floats(L3) * (int)sizeof(float);
    const int arc =
        allow_lds(reinterpret_cast<const void*>(&swarm::k_ppo_deep_grads<KK, L3>), lds);
    if (arc) return arc;
    hipLaunchKernelGGL((swarm::k_ppo_deep_grads<KK, L3>), dim3((unsigned)blocks), dim3(512),
                       (size_t)lds, s, p);
    return SWARM_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(swarm::k_ppo_reduce, dim3((unsigned)((p.size + 63) / 64)), dim3(1024), 0, s,
                     p.partial, blocks, p.size, grad);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

}  // namespace

int swarm_ppo_deep_epoch_grad(const float* x, int32_t T, int32_t S, int32_t d_in,
                              const int64_t* actions, const float* old_logp,
                              const float* rewards, int32_t n_hidden, const int32_t* widths,
                              const float* const* w, const float* const* b, const float* wa,
                              const float* ba, int32_t k, const float* wc, const float* bc,
                              float gamma, float lambda, float clip_eps, float entropy_coef,
                              void* workspace, int64_t workspace_bytes, float* grad,
                              void* stream) {
  return deep_ppo_epoch(x, T, S, d_in, actions, old_logp, rewards, n_hidden, widths, w, b, wa, ba,
                        k, wc, bc, gamma, lambda, clip_eps, entropy_coef, workspace,
                        workspace_bytes, grad, stream, nullptr, 1);
}

int swarm_ppo_epoch_grad_ep(const float* x, int32_t T, int32_t S, int32_t d_in,
                            const int64_t* actions, const float* old_logp, const float* rewards,
                            const float* w1, const float* b1, int32_t hidden, const float* wa,
                            const float* ba, int32_t k, const float* wc, const float* bc,
                            float gamma, float lambda, float clip_eps, float entropy_coef,
                            void* workspace, int64_t workspace_bytes, float* grad, void* stream,
                            const uint8_t* dones, int32_t per_env) {
  if (!dones) return fail(SWARM_EINVAL, "null argument");
  return ppo_epoch(x, T, S, d_in, actions, old_logp, rewards, w1, b1, hidden, wa, ba, k, wc, bc,
                   gamma, lambda, clip_eps, entropy_coef, workspace, workspace_bytes, grad, stream,
                   nullptr, dones, per_env);
}

int swarm_ppo_epoch_step_ep(const float* x, int32_t T, int32_t S, int32_t d_in,
                            const int64_t* actions, const float* old_logp, const float* rewards,
                            int32_t hidden, int32_t k, float gamma, float lambda, float clip_eps,
                            float entropy_coef, const swarm_adam_t* adam, void* workspace,
                            int64_t workspace_bytes, float* grad, void* stream,
                            const uint8_t* dones, int32_t per_env) {
  if (!adam || !dones) return fail(SWARM_EINVAL, "null argument");
  if (!(adam->beta1 >= 0.0f && adam->beta1 < 1.0f && adam->beta2 >= 0.0f && adam->beta2 < 1.0f))
    return fail(SWARM_EINVAL, "Adam betas must be in [0, 1)");
  return ppo_epoch(x, T, S, d_in, actions, old_logp, rewards, adam->param[0], adam->param[1],
                   hidden, adam->param[2], adam->param[3], k, adam->param[4], adam->param[5],
                   gamma, lambda, clip_eps, entropy_coef, workspace, workspace_bytes, grad, stream,
                   adam, dones, per_env);
}

int swarm_ppo_deep_epoch_grad_ep(const float* x, int32_t T, int32_t S, int32_t d_in,
                                 const int64_t* actions, const float* old_logp,
                                 const float* rewards, int32_t n_hidden, const int32_t* widths,
                                 const float* const* w, const float* const* b, const float* wa,
                                 const float* ba, int32_t k, const float* wc, const float* bc,
                                 float gamma, float lambda, float clip_eps, float entropy_coef,
                                 void* workspace, int64_t workspace_bytes, float* grad,
                                 void* stream, const uint8_t* dones, int32_t per_env) {
  if (!dones) return fail(SWARM_EINVAL, "null argument");
  return deep_ppo_epoch(x, T, S, d_in, actions, old_logp, rewards, n_hidden, widths, w, b, wa, ba,
                        k, wc, bc, gamma, lambda, clip_eps, entropy_coef, workspace,
                        workspace_bytes, grad, stream, dones, per_env);
}

// ---- entry points: ensembles, M independent actor-critic MLPs per launch
// (swarm_ensemble.cuh)

int swarm_policy_ensemble_sample(const float* obs, int32_t n_members, int32_t n_per,
                                 int32_t d_in, const float* w1, const float* b1, int32_t hidden,
                                 const float* w2, const float* b2, int32_t k,
                                 const uint64_t* seeds, uint64_t* state, int32_t n_state_per,
                                 float explore_p, const float* f_table, const float* t_table,
                                 int64_t* out_idx, float* out_logp, float* out_f, float* out_t,
                                 float* out_logits, void* stream) {
  if (!obs || !w1 || !b1 || !w2 || !b2 || !seeds || !state || !f_table || !t_table || !out_idx ||
      !out_logp || !out_f || !out_t)
    return fail(SWARM_EINVAL, "null argument");
  if (const char* why = members_limit(n_members)) return fail(SWARM_ECAPACITY, why);
  if (const char* why = mlp_limits(d_in, hidden, k)) return fail(SWARM_ECAPACITY, why);
  bool go;
  if (const int rc = sampler_check(explore_p, n_per, n_state_per, true, &go); rc || !go)
    return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const swarm::EnsembleMlpArgs e{
      swarm::MlpArgs{obs, n_per, d_in, w1, b1, hidden, w2, b2, k, 0u, 0u,
                     reinterpret_cast<unsigned long long*>(state), explore_p, f_table, t_table,
                     out_idx, out_logp, out_f, out_t, out_logits},
      reinterpret_cast<const unsigned long long*>(seeds), n_state_per};
  // the variant of the member's own agent count, and whole blocks per member:
  // no block, so no counter group, straddles two
  return mlp_variant(n_per, d_in, k, [&](auto GG_, auto DD_, auto KK_) -> int {
    constexpr int GG = GG_, DD = DD_, KK = KK_;
    const dim3 grid((unsigned)(((long)n_per * GG + 255) / 256), (unsigned)n_members);
    const size_t lds = mlp_lds_bytes<DD, KK>(hidden);
    hipLaunchKernelGGL((swarm::k_policy_ensemble_sample<GG, DD, KK>), grid, dim3(256), lds, s, e);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  });
}

int64_t swarm_ppo_ensemble_workspace_bytes(int32_t n_members, int32_t T, int32_t S,
                                           int32_t d_in, int32_t hidden, int32_t k) {
  if (T < 1 || S < 1 || ensemble_limits(n_members, T, S) || ppo_limits(d_in, hidden, k))
    return -1;
  const long n = (long)T * S;
  const PpoPlan pl = ppo_plan_for(n, d_in, hidden, k);
  if (pl.rc) return -1;
  return (int64_t)ppo_ensemble_workspace((size_t)n_members, (size_t)n, (size_t)S,
                                         swarm::ppo_grad_size(d_in, hidden, k), pl).total;
}

// The four launches of ppo_epoch with the member index as grid dimension y.
int swarm_ppo_ensemble_epoch_grad(const float* x, int32_t n_members, int32_t T, int32_t S,
                                  int32_t d_in, const int64_t* actions, const float* old_logp,
                                  const float* rewards, const float* w1, const float* b1,
                                  int32_t hidden, const float* wa, const float* ba, int32_t k,
                                  const float* wc, const float* bc, float gamma, float lambda,
                                  float clip_eps, float entropy_coef, void* workspace,
                                  int64_t workspace_bytes, float* grad, void* stream) {
  if (!x || !actions || !old_logp || !rewards || !w1 || !b1 || !wa || !ba || !wc || !bc ||
      !workspace || !grad)
    return fail(SWARM_EINVAL, "null argument");
  if (T < 1 || S < 1) return fail(SWARM_EINVAL, "T, S >= 1");
  if (const char* why = ensemble_limits(n_members, T, S)) return fail(SWARM_ECAPACITY, why);
  if (const char* why = ppo_limits(d_in, hidden, k)) return fail(SWARM_ECAPACITY, why);
  const int n = T * S;
  const int size = swarm::ppo_grad_size(d_in, hidden, k);
  const unsigned M = (unsigned)n_members;
  const PpoPlan pl = ppo_plan_for(n, d_in, hidden, k);
  if (pl.rc) return pl.rc;
  const LearnWorkspace ws = ppo_ensemble_workspace(M, (size_t)n, (size_t)S, size, pl);
  if (workspace_bytes < (int64_t)ws.total)
    return fail(SWARM_EINVAL, "workspace smaller than swarm_ppo_ensemble_workspace_bytes");
  swarm::PpoEnsembleArgs a{};
  a.x = x;
  a.actions = actions;
  a.old_logp = old_logp;
  a.rewards = rewards;
  a.w1 = w1;
  a.b1 = b1;
  a.wa = wa;
  a.ba = ba;
  a.wc = wc;
  a.bc = bc;
  a.T = T;
  a.S = S;
  a.n = n;
  a.d = d_in;
  a.hidden = hidden;
  a.k = k;
  a.members = n_members;
  a.gamma = gamma;
  a.lambda = lambda;
  a.clip_eps = clip_eps;
  a.c_ent = entropy_coef;
  a.values = slice<float>(workspace, ws.values);
  a.adv = slice<float>(workspace, ws.adv);
  a.dv = slice<float>(workspace, ws.dv);
  a.spart = slice<double>(workspace, ws.spart);
  a.table = slice<float>(workspace, ws.table);
  a.partial = slice<float>(workspace, ws.partial);
  a.grad = grad;
  a.gae_blocks = (S + 255) / 256;
  a.table_rows = pl.table_rows;
  a.table_floats = pl.table_floats;
  a.blocks = pl.blocks;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rc = ppo_variant(hidden, d_in, k, [&](auto NN_, auto DD_, auto KK_) -> int {
    constexpr int NN = NN_, DD = DD_, KK = KK_;
    if (n < (1 << 20))
      hipLaunchKernelGGL((swarm::k_ppo_ensemble_values_split<DD>),
                         dim3((unsigned)(((long)n + 63) / 64), M), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((swarm::k_ppo_ensemble_values<DD>),
                         dim3((unsigned)(((n + 3) / 4 + 255) / 256), M), dim3(256), 0, s, a);
    const dim3 ggrid((unsigned)(a.gae_blocks + (pl.table_floats + 255) / 256), M);
    if (T <= 32)
      hipLaunchKernelGGL((swarm::k_ppo_ensemble_gae<32, DD, KK>), ggrid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((swarm::k_ppo_ensemble_gae<0, DD, KK>), ggrid, dim3(256), 0, s, a);
    return ppo_grads_variant<NN>(pl.coop, [&](auto TT_, auto CO_) -> int {
      constexpr int TT = TT_;
      constexpr bool CO = CO_;
      const int arc = allow_lds(
          reinterpret_cast<const void*>(&swarm::k_ppo_ensemble_grads<NN, TT, CO, DD, KK>),
          pl.lds);
      if (arc) return arc;
      hipLaunchKernelGGL((swarm::k_ppo_ensemble_grads<NN, TT, CO, DD, KK>),
                         dim3((unsigned)pl.blocks, M), dim3(64 * NN * TT), (size_t)pl.lds, s, a);
      return SWARM_OK;
    });
  });
  if (rc) return rc;
  hipLaunchKernelGGL(swarm::k_ppo_ensemble_reduce, dim3((unsigned)((size + 63) / 64), M),
                     dim3(1024), 0, s, a);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// ---- entry points: ensembles of deep actor-critic MLPs (swarm_ensemble.cuh
// over swarm_deep.cuh)

int swarm_policy_deep_ensemble_sample(const float* obs, int32_t n_members, int32_t n_per,
                                      int32_t d_in, int32_t n_hidden, const int32_t* widths,
                                      const float* const* w, const float* const* b,
                                      const float* wa, const float* ba, int32_t k,
                                      const uint64_t* seeds, uint64_t* state,
                                      int32_t n_state_per, float explore_p, const float* f_table,
                                      const float* t_table, int64_t* out_idx, float* out_logp,
                                      float* out_f, float* out_t, float* out_logits,
                                      void* stream) {
  if (!obs || !widths || !w || !b || !wa || !ba || !seeds || !state || !f_table || !t_table ||
      !out_idx || !out_logp || !out_f || !out_t)
    return fail(SWARM_EINVAL, "null argument");
  if (const char* why = members_limit(n_members)) return fail(SWARM_ECAPACITY, why);
  if (const char* why = deep_limits(d_in, n_hidden, widths, k)) return fail(SWARM_ECAPACITY, why);
  swarm::DeepPpoArgs p{};
  if (!deep_fill(d_in, n_hidden, widths, w, b, wa, ba, k, p, nullptr))
    return fail(SWARM_EINVAL, "null parameter");
  bool go;
  if (const int rc = sampler_check(explore_p, n_per, n_state_per, true, &go); rc || !go)
    return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  swarm::DeepEnsembleArgs e{};
  e.dp = p.net;
  e.m = swarm::MlpArgs{obs,     n_per,   d_in,    nullptr, nullptr, 0,  nullptr,
                       nullptr, k,       0u,      0u,
                       reinterpret_cast<unsigned long long*>(state), explore_p, f_table,
                       t_table, out_idx, out_logp, out_f,  out_t,   out_logits};
  e.seeds = reinterpret_cast<const unsigned long long*>(seeds);
  e.n_state_per = n_state_per;
  // whole blocks of 64 agents per member: one workgroup, one counter group
  const dim3 grid((unsigned)((n_per + swarm::kDeepAgents - 1) / swarm::kDeepAgents),
                  (unsigned)n_members);
  if (k <= 4)
    hipLaunchKernelGGL(swarm::k_policy_deep_ensemble_sample<4>, grid, dim3(256), 0, s, e);
  else
    hipLaunchKernelGGL(swarm::k_policy_deep_ensemble_sample<16>, grid, dim3(256), 0, s, e);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int64_t swarm_ppo_deep_ensemble_workspace_bytes(int32_t n_members, int32_t T, int32_t S,
                                                int32_t d_in, int32_t n_hidden,
                                                const int32_t* widths, int32_t k) {
  if (T < 1 || S < 1 || !widths || ensemble_limits(n_members, T, S) ||
      deep_limits(d_in, n_hidden, widths, k))
    return -1;
  return (int64_t)deep_ppo_workspace((size_t)n_members, (long)T * S, S,
                                     deep_ppo_grad_size(d_in, n_hidden, widths, k)).total;
}

int swarm_ppo_deep_ensemble_epoch_grad(const float* x, int32_t n_members, int32_t T, int32_t S,
                                       int32_t d_in, const int64_t* actions,
                                       const float* old_logp, const float* rewards,
                                       int32_t n_hidden, const int32_t* widths,
                                       const float* const* w, const float* const* b,
                                       const float* wa, const float* ba, int32_t k,
                                       const float* wc, const float* bc, float gamma,
                                       float lambda, float clip_eps, float entropy_coef,
                                       void* workspace, int64_t workspace_bytes, float* grad,
                                       void* stream) {
  if (!x || !actions || !old_logp || !rewards || !widths || !w || !b || !wa || !ba || !wc ||
      !bc || !workspace || !grad)
    return fail(SWARM_EINVAL, "null argument");
  if (T < 1 || S < 1) return fail(SWARM_EINVAL, "T, S >= 1");
  if (const char* why = ensemble_limits(n_members, T, S)) return fail(SWARM_ECAPACITY, why);
  if (const char* why = deep_limits(d_in, n_hidden, widths, k)) return fail(SWARM_ECAPACITY, why);
  swarm::DeepPpoEnsembleArgs a{};
  swarm::DeepPpoArgs& p = a.p;
  if (!deep_fill(d_in, n_hidden, widths, w, b, wa, ba, k, p, a.seg))
    return fail(SWARM_EINVAL, "null parameter");
  const int n = T * S;
  const LearnWorkspace ws = deep_ppo_workspace((size_t)n_members, n, S, p.size);
  if (workspace_bytes < (int64_t)ws.total)
    return fail(SWARM_EINVAL, "workspace smaller than swarm_ppo_deep_ensemble_workspace_bytes");
  const int gae_blocks = (S + 255) / 256;
  deep_ppo_bind(p, x, n, d_in, k, wc, bc, actions, old_logp, gae_blocks, clip_eps, entropy_coef,
                workspace, ws);
  // the grids of swarm_ppo_deep_epoch_grad, from the member's own n
  const unsigned tiles = (unsigned)(((long)n + swarm::kDeepAgents - 1) / swarm::kDeepAgents);
  const int blocks = deep_ppo_blocks(n);
  a.values = slice<float>(workspace, ws.values);
  a.members = n_members;
  a.blocks = blocks;
  a.grad = grad;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned M = (unsigned)n_members;
  hipLaunchKernelGGL(swarm::k_ppo_deep_ensemble_values<8>, dim3(tiles, M), dim3(512), 0, s, a);
  // k_ppo_ensemble_gae without pack workgroups (its grid is the GAE blocks:
  // no parameter table, so the one-layer weights stay null)
  swarm::PpoEnsembleArgs g{};
  g.rewards = rewards;
  g.T = T;
  g.S = S;
  g.n = n;
  g.members = n_members;
  g.gamma = gamma;
  g.lambda = lambda;
  g.values = a.values;
  g.adv = slice<float>(workspace, ws.adv);
  g.dv = slice<float>(workspace, ws.dv);
  g.spart = slice<double>(workspace, ws.spart);
  g.gae_blocks = gae_blocks;
  if (T <= 32)
    hipLaunchKernelGGL((swarm::k_ppo_ensemble_gae<32, 1, 4>), dim3((unsigned)gae_blocks, M),
                       dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((swarm::k_ppo_ensemble_gae<0, 1, 4>), dim3((unsigned)gae_blocks, M),
                       dim3(256), 0, s, g);
  const int rc = deep_variant(k, n_hidden, [&](auto KK_, auto L3_) -> int {
    constexpr int KK = KK_;
    constexpr bool L3 = L3_;
    const int lds = swarm::deep_grads_lds_floats(L3) * (int)sizeof(float);
    const int arc = allow_lds(
        reinterpret_cast<const void*>(&swarm::k_ppo_deep_ensemble_grads<KK, L3>), lds);
    if (arc) return arc;
    hipLaunchKernelGGL((swarm::k_ppo_deep_ensemble_grads<KK, L3>), dim3((unsigned)blocks, M),
                       dim3(512), (size_t)lds, s, a);
    return SWARM_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(swarm::k_ppo_deep_ensemble_reduce, dim3((unsigned)((p.size + 63) / 64), M),
                     dim3(1024), 0, s, a);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

// ---- the GAE across episode ends (declared above ppo_epoch)

namespace {

int launch_gae_ep(int hidden, int d_in, int k, dim3 grid, hipStream_t s, const float* rewards,
                  const float* values, int T, int S, float gamma, float lambda, float* adv,
                  float* dv, double* spart, int gae_blocks, const swarm::PpoPack& pk,
                  const uint8_t* dones, int per_env) {
  return ppo_variant(hidden, d_in, k, [&](auto, auto DD_, auto KK_) -> int {
    constexpr int DD = DD_, KK = KK_;
    if (T <= 32)
      hipLaunchKernelGGL((swarm::k_ppo_gae_ep<32, DD, KK>), grid, dim3(256), 0, s, rewards, values,
                         T, S, gamma, lambda, adv, dv, spart, gae_blocks, pk, dones, per_env);
    else
      hipLaunchKernelGGL((swarm::k_ppo_gae_ep<0, DD, KK>), grid, dim3(256), 0, s, rewards, values,
                         T, S, gamma, lambda, adv, dv, spart, gae_blocks, pk, dones, per_env);
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  });
}

}  // namespace
