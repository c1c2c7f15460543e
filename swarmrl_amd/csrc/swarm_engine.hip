// swarm_engine.hip -- MI355X (gfx950) active-Brownian swarm engine.
//
// Implements the C ABI of include/swarmrl_amd.h.  The per-step hot path of
// the reference (ESPResSo Brownian dynamics + WCA via a cell system, driven by
// swarmrl/engine/espresso.py:1251-1308) runs here as hand-written HIP:
//
//   integrator      swarm_integrator.cuh: per window k_cluster_build ->
//                   k_cluster_run -> k_check (cluster-parallel Brownian
//                   dynamics + WCA, exact fallback to the global path);
//                   k_global also runs steepest descent (espresso.py:1161-1168).
//   observables     swarm_observe.cuh: k_grid_build, k_vision*, k_field*,
//                   k_pairs, the trajectory ring.
//   packing         swarm_pack.h (plain C++17): the build/run contract -- packing
//                   classes, their layout in waves, the pair and class words.
//   planning        swarm_plan.h over swarm_sizes.h (plain C++17): the checks,
//                   cell grids, path choices and buffer sizes an engine fixes
//                   at creation, one pure function (swarm::plan_engine).
//   launches        swarm_engine_host.cuh (engine, observables) and
//                   swarm_learn_host.cuh (policies, PPO); this file keeps the
//                   engine's state and the C ABI's checks around them.
//
// Number formats: positions are uint32 box fractions + int32
// image counters, angles uint32 turn fractions, pair sums int64 fixed point,
// so results are independent of neighbour order and bit-identical to the
// CPU oracle.  Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/swarmrl_amd.h"
#include "swarm_device.cuh"
#include "swarm_integrator.cuh"
#include "swarm_integrator3.cuh"
#include "swarm_deep.cuh"
#include "swarm_policy.cuh"
#include "swarm_ppo.cuh"
#include "swarm_ensemble.cuh"
#include "swarm_rnd.cuh"
#include "swarm_rod.cuh"
#include "swarm_ellipsoid.cuh"
#include "swarm_langevin.cuh"
#include "swarm_observe.cuh"
#include "swarm_reset.cuh"
#include "swarm_plan.h"

namespace {

constexpr double kTwo32 = 4294967296.0;
constexpr double kTwoPi = 6.283185307179586476925;
using swarm::kSkinUm;  // the Verlet skin (swarm_plan.h)

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess)                                                    \
      return fail(SWARM_EDEVICE, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

void derive(const swarm_params_t& p, Derived& d) {
  std::memset(&d, 0, sizeof(d));
  for (int a = 0; a < 3; ++a) {
    d.sx[a] = (float)(p.box[a] / kTwo32);
    d.inv_sx[a] = (float)(kTwo32 / p.box[a]);
  }
  const double kT = p.kT, dt = p.time_step;
  for (int s = 0; s < p.n_species; ++s) {
    const double gt = p.gamma_t[s], gr = p.gamma_r[s];
    d.mob_dt[s] = (float)(dt / gt);
    d.rot_dt[s] = (float)(dt / gr);
    d.sig_t[s] = (float)std::sqrt(2.0 * kT * dt / gt);
    d.sig_r[s] = (float)std::sqrt(2.0 * kT * dt / gr);
    d.inv_gt[s] = (float)(1.0 / gt);
    d.inv_gr[s] = (float)(1.0 / gr);
    d.sig_v[s] = p.mass[s] > 0.0 ? (float)std::sqrt(kT / p.mass[s]) : 0.0f;
    d.sig_w[s] = p.rinertia[s] > 0.0 ? (float)std::sqrt(kT / p.rinertia[s]) : 0.0f;
  }
  d.rc_max = swarm::max_cutoff(p);
  for (int s = 0; s < p.n_species; ++s)
    for (int t = 0; t < p.n_species; ++t) {
      const double rc = p.radius[s] + p.radius[t];
      const double rc2 = rc * rc;
      d.cut2[s * kMaxSpecies + t] = (float)rc2;
      d.sig6[s * kMaxSpecies + t] = (float)(rc2 * rc2 * rc2 * 0.5);
    }
  for (int s = 0; s < p.n_species; ++s)
    for (int t = 0; t < p.n_species; ++t) {
      const double r = p.radius[s] + p.radius[t] + kSkinUm;
      d.nb2[s * kMaxSpecies + t] = (float)(r * r);
    }
  d.skin = (float)kSkinUm;
  d.rc_max_f = (float)d.rc_max;
  {
    const double g = 0.99 * 0.25 * std::min(p.box[0], p.box[1]);
    d.glim2 = (float)(g * g);
  }
  d.eps24 = (float)(24.0 * p.wca_epsilon);
  d.n_species = p.n_species;
  d.key0 = (uint32_t)p.seed;
  d.key1 = (uint32_t)(p.seed >> 32);
  d.noisy = p.kT > 0.0 ? 1 : 0;
  d.periodic = p.periodic;
  for (int s = 0; s < p.n_species; ++s) {  // walls: WCA with a radius-0 wall type
    const double rc2 = p.radius[s] * p.radius[s];
    d.wcut2[s] = (float)rc2;
    d.wsig6[s] = (float)(rc2 * rc2 * rc2 * 0.5);
  }
}

using swarm::cell_grid;  // swarm_plan.h (the observables' grids use the same rule)

}  // namespace

// =================================================================== C ABI
struct swarm_engine {
  // ---- fixed at creation
  swarm_params_t params;
  Derived derived;
  int32_t n_envs = 0, n = 0;
  int device = 0;
  int n_cus = 0;
  // the cell grids, every path choice and the buffer sizes (swarm_plan.h).
  // Nothing writes it after swarm_engine_create but swarm_engine_set_rod,
  // swarm_engine_set_ellipsoids and swarm_engine_set_langevin, which take the
  // engine off the cluster path for good (the second also widens the
  // global-path grid).
  swarm::EnginePlan plan;
  DevState st{};
  Scratch sc{};
  VisionSorted vs{};
  Derived* d_derived = nullptr;
  double* d_box = nullptr;
  uint64_t* d_step = nullptr;
  uint32_t* d_arrive = nullptr;
  int32_t* d_order = nullptr;  // observable grid scratch (with d_start below)
  int32_t* d_count = nullptr;
  float* d_noise = nullptr;  // plan.noise_table: the two noise tables (k_noise)
  float* own_f_swim = nullptr;
  float* own_torque_z = nullptr;
  // every device buffer the engine owns, the lazily created ones below
  // included (dev_malloc / dev_free); swarm_engine_destroy frees what is listed
  std::vector<void*> allocs;

  // ---- what a call can change
  hipStream_t stream = nullptr;
  // trajectory ring (swarm_engine_traj_ring): host-pinned, device-mapped
  unsigned char* traj_host = nullptr;
  unsigned char* traj_dev = nullptr;
  uint64_t* d_traj_count = nullptr;
  int traj_cap = 0, traj_env = 0;
  size_t traj_entry = 0;
  // observable grid scratch, grown on demand
  int32_t* d_start = nullptr;
  size_t start_cap = 0;
  int32_t* d_pairs = nullptr;
  size_t pairs_cap = 0;
  // swarm_engine_prebuild: the next window's build (and noise table) were
  // launched ahead on another stream from the current positions
  bool prebuilt = false;
  // swarm_engine_defer_build: the next stage of the deferred three-launch
  // build (1 sort, 2 pairs, 3 cluster build; 0 none) that rides along in the
  // next observable / policy launch; flushed before a window runs
  int ride_stage = 0;
  // plan.defer_check (SWARMRL_AMD_DEFER_CHECK on an l1_pairs engine): after
  // swarm_engine_hint_defer_check the next integrate call leaves its last
  // window's check pending (check_pending, check_steps: its sub-steps)
  // instead of launching k_check; the reward launch that follows carries it
  // (launch_field), anything else flushes it first (flush_check).  Host-side
  // state: it must not outlive a stream capture (swarm_engine_flush_check).
  bool defer_hint = false;
  bool check_pending = false;
  int check_steps = 0;
  // speculative vision grid (swarm_vision_cone_persistent): the last
  // persistent call's arguments; vgrid_ready: the reward launch built the
  // grid of the current positions for them (honoured while the deferred
  // build is at stage 2, i.e. nothing moved the colloids since).
  bool spec_ok = false;
  VisionArgs spec_va{};
  bool vgrid_ready = false;
  // swarm_engine_prebuild_noise: the next window's noise table for this many
  // sub-steps was launched ahead (on a stream of the caller's)
  int prebuilt_noise_steps = 0;
  // plan.noise_blocks > 0: the last k_cluster_run_wide filled the next
  // window's noise table beside the run (the table's first step and length
  // are checked on the device, this flag only skips k_noise)
  bool next_table_ready = false;
  // swarm_engine_profile: HIP events around every k_cluster_run launch;
  // launches captured into a graph get event-record nodes whose events are
  // kept (graph_events) for swarm_engine_profile_graph after each replay
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> graph_events;
  // per captured run node, an empty event pair recorded right after it: the
  // cost of an event-record node pair itself (swarm_engine_profile_graph)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> graph_cal;
  // and each captured run node's own start / end stamps (swarm::stamp_start,
  // stamp_end): d_tstamp[k][kStampSub][2] for the k-th captured run node
  unsigned long long* d_tstamp = nullptr;
  int stamp_next = 0;
  // [kMaxStamps][kRoles][2]: the workgroup roles of the launches that follow
  // the k-th captured run node (its k_check, then the next window's build and
  // observable launches), swarm::role_begin / role_end
  unsigned long long* d_rstamp = nullptr;
  // swarm_engine_set_rod: every sub-step runs on k_rod_run (swarm_rod.cuh)
  bool has_rod = false;
  swarm::RodArgs rod{};
  // swarm_engine_set_ellipsoids: every sub-step runs on k_ellipsoid_run
  // (swarm_ellipsoid.cuh); ell_gb: aspect ratio != 1 (Gay-Berne pairs)
  bool has_ell = false, ell_gb = false;
  swarm::EllArgs* d_ell = nullptr;
  // swarm_engine_set_langevin: every sub-step runs on k_langevin_run
  // (swarm_langevin.cuh); lv: the host copy of d_lv, gamma_flow: the flow
  // field's friction (swarm_engine_set_flow_field), d_flow: its records and
  // their capacity in values
  bool has_lv = false;
  swarm::LangevinArgs lv{};
  swarm::LangevinArgs* d_lv = nullptr;
  double gamma_flow = 0.0;
  float* d_flow = nullptr;
  size_t flow_cap = 0;
  // a sub-step or an overlap-removal step has run
  bool stepped = false;
  // swarm_engine_set_potential_field: the field's device copy (derived.pot.phi
  // points at it while a field is set) and its capacity in values
  float* d_pot = nullptr;
  size_t pot_cap = 0;
  // swarm_engine_set_reset_plan: the home state, each particle's placement
  // group (-1: home) and the groups; d_reset_envs: the env list of a
  // swarm_engine_reset_envs call; reset_ordinal: the non-empty calls so far
  bool has_reset_plan = false;
  uint32_t* d_home_q = nullptr;
  int32_t* d_home_img = nullptr;
  uint32_t* d_home_ang = nullptr;
  float* d_home_dir3 = nullptr;
  int32_t* d_group_of = nullptr;
  swarm::ResetGroup* d_groups = nullptr;
  size_t groups_cap = 0;
  int32_t* d_reset_envs = nullptr;
  uint64_t reset_ordinal = 0;
  // swarm_engine_reset_marked: per env, the device-mask resets it has had
  uint32_t* d_reset_counts = nullptr;
};

// Device buffers of the engine: listed in e->allocs before anything else can
// fail, so that swarm_engine_destroy frees them whatever becomes of the call.
namespace {

template <typename T>
hipError_t dev_malloc(swarm_engine* e, T** p, size_t bytes) {
  void* v = nullptr;
  const hipError_t err = hipMalloc(&v, bytes);
  if (err != hipSuccess) return err;
  e->allocs.push_back(v);
  *p = reinterpret_cast<T*>(v);
  return hipSuccess;
}

// Frees *p (null: nothing to do) and clears it.
template <typename T>
hipError_t dev_free(swarm_engine* e, T** p) {
  if (!*p) return hipSuccess;
  e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), (void*)*p), e->allocs.end());
  const hipError_t err = hipFree(*p);
  *p = nullptr;
  return err;
}

}  // namespace

// every launch of the integrator and the observables (launch_*, run_bd,
// vision_cone_impl, launch_field, the LDS sizes and their opt-in)
#include "swarm_engine_host.cuh"

namespace {

// The SWARMRL_AMD_* overrides of swarm::plan_engine, read here and nowhere
// else: the first character of each variable's value, 0 for unset (an empty
// value is set: it counts as a blank).
swarm::PlanOverrides read_plan_overrides() {
  auto first = [](const char* name) -> char {
    const char* s = std::getenv(name);
    return !s ? 0 : s[0] ? s[0] : ' ';
  };
  swarm::PlanOverrides ov;
  ov.cluster_path = first("SWARMRL_AMD_CLUSTER_PATH");
  ov.local_uf = first("SWARMRL_AMD_LOCAL_UF");
  ov.nlist = first("SWARMRL_AMD_NLIST");
  ov.noise_table = first("SWARMRL_AMD_NOISE_TABLE");
  ov.env_build = first("SWARMRL_AMD_ENV_BUILD");
  ov.wide_run = first("SWARMRL_AMD_WIDE_RUN");
  ov.rot_helper = first("SWARMRL_AMD_ROT_HELPER");
  ov.defer_check = first("SWARMRL_AMD_DEFER_CHECK");
  return ov;
}

// One row of swarm_engine_create's allocation table (SWARM_ENGINE_BUFS,
// swarm_plan.h): the member that takes the buffer, and its element size.
struct BufSlot {
  void** member;
  size_t elem;
};
template <swarm::EngineBuf kId, typename T>
BufSlot buf_slot(T** member) {
  static_assert(kId == swarm::kBufDerived || swarm::kBufElemBytes[kId] == sizeof(T),
                "swarm_plan.h: a row's bytes per element disagree with the member's type");
  return {reinterpret_cast<void**>(member), sizeof(T)};
}

void to_fixed(double x, double L, uint32_t* q, int32_t* img) {
  const double u = x / L;
  double fl = std::floor(u);
  double qd = std::nearbyint((u - fl) * kTwo32);
  if (qd >= kTwo32) {
    qd -= kTwo32;
    fl += 1.0;
  }
  *q = (uint32_t)qd;
  *img = (int32_t)fl;
}

// host copy of swarm::sincos_turn (same fp32 operation sequence)
void host_sincos_turn(uint32_t a, float* s_out, float* c_out) {
  const uint32_t b = a + 0x20000000u;
  const uint32_t quad = b >> 30;
  const int32_t rem = (int32_t)(b & 0x3FFFFFFFu) - 0x20000000;
  const float x = (float)rem * 1.46291807926715968e-09f;
  const float z = x * x;
  float sp = -1.9515295891e-4f;
  sp = sp * z;
  sp = sp + 8.3321608736e-3f;
  sp = sp * z;
  sp = sp + -1.6666654611e-1f;
  sp = sp * z;
  sp = sp * x;
  const float s = sp + x;
  float cp = 2.443315711809948e-5f;
  cp = cp * z;
  cp = cp + -1.388731625493765e-3f;
  cp = cp * z;
  cp = cp + 4.166664568298827e-2f;
  cp = cp * z;
  cp = cp * z;
  float c = cp - 0.5f * z;
  c = c + 1.0f;
  float so, co;
  switch (quad) {
    case 0: so = s; co = c; break;
    case 1: so = c; co = -s; break;
    case 2: so = -s; co = -c; break;
    default: so = -c; co = s; break;
  }
  *s_out = so;
  *c_out = co;
}

uint32_t angle_fixed(double dx, double dy) {
  const double phi = std::atan2(dy, dx);
  const int64_t a = (int64_t)std::nearbyint(phi / kTwoPi * kTwo32);
  return (uint32_t)(a & 0xFFFFFFFFLL);
}

// Host fp64 positions and directors [E][N][3] in the engine's own formats
// (swarm_engine_upload_state, and the home state of a reset plan): q, img
// [3][M], ang [M], in 3-D the normalised directors d3 [3][M].
struct HostState {
  std::vector<uint32_t> q, ang;
  std::vector<int32_t> img;
  std::vector<float> d3;
};

void state_to_fixed(const swarm_engine* e, const double* pos, const double* director,
                    HostState* h) {
  const size_t M = (size_t)e->st.m;
  const int D = e->params.n_dims;
  h->q.assign(3 * M, 0u);
  h->img.assign(3 * M, 0);
  h->ang.assign(M, 0u);
  h->d3.assign(D == 3 ? 3 * M : 0, 0.0f);
  for (size_t g = 0; g < M; ++g) {
    for (int a = 0; a < D; ++a)
      to_fixed(pos[3 * g + a], e->params.box[a], &h->q[a * M + g], &h->img[a * M + g]);
    h->ang[g] = angle_fixed(director[3 * g + 0], director[3 * g + 1]);
    if (D == 3) {
      const double* v = director + 3 * g;
      const double nm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      for (int a = 0; a < 3; ++a) h->d3[a * M + g] = (float)(nm > 0.0 ? v[a] / nm : (a == 2));
    }
  }
}

}  // namespace

extern "C" {

const char* swarm_last_error(void) { return g_err.c_str(); }

#ifndef SWARM_BUILD_ID
#define SWARM_BUILD_ID "unknown"
#endif
const char* swarm_build_id(void) { return SWARM_BUILD_ID; }

// the plan's static_lds
static_assert(swarm::kPairTablesBytes == sizeof(swarm::PairTables), "swarm_sizes.h: PairTables");

int swarm_engine_create(const swarm_params_t* params, int32_t n_envs, int32_t n_particles,
                        const int32_t* species, swarm_engine_t** out) {
  // 1. the arguments
  if (!params || !out || !species) return fail(SWARM_EINVAL, "null argument");
  *out = nullptr;

  // 2. the plan (its parameter checks first), then what it does not see:
  // the species indices and the device
  swarm::EnginePlan plan;
  const char* msg = "";
  if (const int rc = swarm::plan_engine(*params, n_envs, n_particles, read_plan_overrides(),
                                        swarm::kPairTablesBytes, &plan, &msg))
    return fail(rc, msg);
  for (int i = 0; i < n_particles; ++i)
    if (species[i] < 0 || species[i] >= params->n_species)
      return fail(SWARM_EINVAL, "species index out of range");
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return fail(SWARM_EDEVICE, "no HIP device");

  // 3. the plan into the kernels' arguments
  swarm_engine* e = new swarm_engine();
  e->params = *params;
  derive(*params, e->derived);
  e->n_envs = n_envs;
  e->n = n_particles;
  e->device = device;
  e->plan = plan;
  const size_t M = (size_t)n_envs * n_particles;
  e->st.n = n_particles;
  e->st.m = (int32_t)M;
  e->st.dims = params->n_dims;
  e->st.reuse = params->reuse_forces ? 1 : 0;
  e->sc.pair_cap = plan.pair_cap;
  e->sc.periodic = params->periodic ? 1 : 0;
  e->sc.local_uf = plan.local_uf ? 1 : 0;
  e->sc.multi_species = params->n_species > 1 ? 1 : 0;
  e->sc.sort_stage_k = plan.sort_stage_k;
  e->sc.one_pass = plan.one_pass ? 1 : 0;
  e->sc.fill_singletons = plan.fill_singletons ? 1 : 0;
  e->sc.S = plan.S;
  e->sc.wmax = plan.wmax;
  e->sc.l1_pairs = plan.l1_pairs ? 1 : 0;
  if (plan.l1_pairs) {
    e->derived.cand_disp = (float)plan.cand_disp;
    for (int a = 0; a < params->n_species; ++a)
      for (int b = 0; b < params->n_species; ++b) {
        const double r = params->radius[a] + params->radius[b] + kSkinUm + 2.0 * plan.cand_disp;
        e->derived.nbc2[a * kMaxSpecies + b] = (float)(r * r);
      }
    // (launch_field: a check rides in the reward launch while every
    // workgroup of the launch is resident)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess)
      e->n_cus = cus;
  }

  // 4. the buffers the plan lists, zeroed, in the plan's order
  uint64_t* vcheck = nullptr;
#define SWARM_BUF_SLOT(id, bytes, member, elements) buf_slot<swarm::kBuf##id>(&member),
  const BufSlot slots[swarm::kNumEngineBufs] = {SWARM_ENGINE_BUFS(SWARM_BUF_SLOT)};
#undef SWARM_BUF_SLOT
  hipError_t err = hipSuccess;
  for (int k = 0; k < swarm::kNumEngineBufs && err == hipSuccess; ++k) {
    const BufSlot& s = slots[k];
    const size_t bytes = plan.count[k] * s.elem;
    if (bytes == 0) continue;  // not on this engine's paths
    err = dev_malloc(e, s.member, bytes);
    if (err == hipSuccess) err = hipMemsetAsync(*s.member, 0, bytes, e->stream);
  }
  allow_engine_lds(device);
  if (err != hipSuccess) {
    swarm_engine_destroy(e);
    return fail(SWARM_EDEVICE, std::string("engine buffers: ") + hipGetErrorString(err));
  }
  e->own_f_swim = e->st.f_swim;
  e->own_torque_z = e->st.torque_z;
  if (vcheck) {
    e->sc.vtag = vcheck;
    e->sc.verdict = vcheck + n_envs;
    e->sc.varrive = vcheck + 2 * (size_t)n_envs;
    e->sc.cstats = reinterpret_cast<unsigned long long*>(vcheck + 3 * (size_t)n_envs);
  }

  // 5. the upload
  std::vector<uint8_t> sp(n_particles);
  for (int i = 0; i < n_particles; ++i) sp[i] = (uint8_t)species[i];
  if (hipMemcpy(e->st.species, sp.data(), sp.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(e->d_derived, &e->derived, sizeof(Derived), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(e->d_box, params->box, 3 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    swarm_engine_destroy(e);
    return fail(SWARM_EDEVICE, "initial upload failed");
  }
  *out = e;
  return SWARM_OK;
}

void swarm_engine_destroy(swarm_engine_t* e) {
  if (!e) return;
  (void)flush_check(e);
  (void)hipDeviceSynchronize();
  for (auto* v : {&e->prof_events, &e->graph_events, &e->graph_cal})
    for (auto& pr : *v) {
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->traj_host) (void)hipHostFree(e->traj_host);
  delete e;
}

int swarm_engine_set_stream(swarm_engine_t* e, void* stream) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  // (binding the stream the engine is on already changes nothing: a pending
  // check stays pending for the reward launch)
  if (e->stream != reinterpret_cast<hipStream_t>(stream))
    if (const int frc = flush_check(e)) return frc;
  e->stream = reinterpret_cast<hipStream_t>(stream);
  return SWARM_OK;
}

int swarm_engine_upload_raw(swarm_engine_t* e, const uint32_t* q, const int32_t* img,
                            const uint32_t* ang) {
  if (e) e->prebuilt = false, e->prebuilt_noise_steps = 0, e->ride_stage = 0;
  if (!e || !q || !img || !ang) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  HIP_TRY(hipMemcpyAsync(e->st.q, q, 3 * M * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->st.img, img, 3 * M * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->st.ang, ang, M * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  // a fresh state: the last force calculation saw these orientations (both
  // reuse_forces slots: the device window counter's parity is not known here)
  for (int k = 0; k < 2; ++k)
    HIP_TRY(hipMemcpyAsync(e->st.ang_prev + k * M, ang, M * sizeof(uint32_t),
                           hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_download_raw(swarm_engine_t* e, uint32_t* q, int32_t* img, uint32_t* ang) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  if (q) HIP_TRY(hipMemcpyAsync(q, e->st.q, 3 * M * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  if (img) HIP_TRY(hipMemcpyAsync(img, e->st.img, 3 * M * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  if (ang) HIP_TRY(hipMemcpyAsync(ang, e->st.ang, M * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_upload_state(swarm_engine_t* e, const double* pos, const double* director) {
  if (!e || !pos || !director) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  HostState h;
  state_to_fixed(e, pos, director, &h);
  if (e->params.n_dims == 3) {
    const int rc = swarm_engine_upload_directors(e, h.d3.data());
    if (rc) return rc;
  }
  const int rc = swarm_engine_upload_raw(e, h.q.data(), h.img.data(), h.ang.data());
  if (rc || !e->has_rod) return rc;
  // a rod's beads follow from its centre (the raw upload keeps them as given)
  if (const int src = launch_rod_snap(e)) return src;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_download_state(swarm_engine_t* e, double* pos, double* director, double* velocity) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  std::vector<uint32_t> q(3 * M), ang(M);
  std::vector<int32_t> img(3 * M);
  std::vector<float> vel(velocity ? 3 * M : 0);
  const int D = e->params.n_dims;
  std::vector<float> d3(D == 3 && director ? 3 * M : 0);
  if (!d3.empty())
    HIP_TRY(hipMemcpyAsync(d3.data(), e->st.dir3, 3 * M * sizeof(float), hipMemcpyDeviceToHost,
                           e->stream));
  HIP_TRY(hipMemcpyAsync(q.data(), e->st.q, 3 * M * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(img.data(), e->st.img, 3 * M * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(ang.data(), e->st.ang, M * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  if (velocity)
    HIP_TRY(hipMemcpyAsync(vel.data(), e->st.vel, 3 * M * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t g = 0; g < M; ++g) {
    if (pos) {
      for (int a = 0; a < 3; ++a)
        pos[3 * g + a] = a < D ? ((double)img[a * M + g] + (double)q[a * M + g] / kTwo32) *
                                     e->params.box[a]
                               : 0.0;
    }
    if (director && D == 3) {
      for (int a = 0; a < 3; ++a) director[3 * g + a] = d3[a * M + g];
    } else if (director) {
      float so, co;
      host_sincos_turn(ang[g], &so, &co);
      director[3 * g + 0] = co;
      director[3 * g + 1] = so;
      director[3 * g + 2] = 0.0;
    }
    if (velocity)
      for (int a = 0; a < 3; ++a) velocity[3 * g + a] = vel[a * M + g];
  }
  return SWARM_OK;
}

int swarm_engine_set_actions(swarm_engine_t* e, const float* f_swim, const float* torque_z,
                             int32_t on_device) {
  if (!e || !f_swim || !torque_z) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  if (on_device == 2) {
    // bind: later launches read the caller's buffers directly (zero copy);
    // the caller keeps them alive and unchanged until the next set_actions
    e->st.f_swim = const_cast<float*>(f_swim);
    e->st.torque_z = const_cast<float*>(torque_z);
    return SWARM_OK;
  }
  e->st.f_swim = e->own_f_swim;
  e->st.torque_z = e->own_torque_z;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpyAsync(e->st.f_swim, f_swim, M * sizeof(float), kind, e->stream));
  HIP_TRY(hipMemcpyAsync(e->st.torque_z, torque_z, M * sizeof(float), kind, e->stream));
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_set_external_force(swarm_engine_t* e, const double* f_ext) {
  if (!e || !f_ext) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  std::vector<float> f(3 * M);
  for (size_t g = 0; g < M; ++g)
    for (int a = 0; a < 3; ++a) f[a * M + g] = (float)f_ext[3 * g + a];
  HIP_TRY(hipMemcpyAsync(e->st.f_ext, f.data(), 3 * M * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_set_directors(swarm_engine_t* e, const double* dir, const uint8_t* mask) {
  if (!e || !dir || !mask) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  if (e->params.n_dims == 3) {  // coll.director = new_direction (espresso.py:1238-1239)
    std::vector<float> d3(3 * M);
    HIP_TRY(hipMemcpyAsync(d3.data(), e->st.dir3, 3 * M * sizeof(float), hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t g = 0; g < M; ++g) {
      if (!mask[g]) continue;
      const double* v = dir + 3 * g;
      const double nm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      if (!(nm > 0.0)) return fail(SWARM_EINVAL, "new_direction must be non-zero");
      for (int a = 0; a < 3; ++a) d3[a * M + g] = (float)(v[a] / nm);
    }
    // the director only: with reuse_forces the next run's sub-step 0 still
    // swims along the director of the last force calculation (dir3_prev)
    HIP_TRY(hipMemcpyAsync(e->st.dir3, d3.data(), 3 * M * sizeof(float), hipMemcpyHostToDevice,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SWARM_OK;
  }
  std::vector<uint32_t> ang(M);
  HIP_TRY(hipMemcpyAsync(ang.data(), e->st.ang, M * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t g = 0; g < M; ++g)
    if (mask[g]) ang[g] = angle_fixed(dir[3 * g + 0], dir[3 * g + 1]);
  HIP_TRY(hipMemcpyAsync(e->st.ang, ang.data(), M * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_remove_overlap(swarm_engine_t* e, int32_t n_steps, double gamma, double max_disp) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  e->prebuilt = false;
  e->ride_stage = 0;
  e->prebuilt_noise_steps = 0;
  if (n_steps <= 0) return SWARM_OK;
  e->stepped = true;
  return launch_global(e, n_steps, 1, (float)gamma, (float)max_disp);
}

int swarm_engine_set_reset_plan(swarm_engine_t* e, const double* pos, const double* director,
                                const swarm_reset_group_t* groups, int32_t n_groups) {
  if (!e || !pos || !director || (n_groups > 0 && !groups))
    return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (n_groups < 0) return fail(SWARM_EINVAL, "n_groups must be >= 0");
  const int D = e->params.n_dims;
  double half = e->params.box[0];
  for (int a = 1; a < D; ++a) half = std::min(half, e->params.box[a]);
  half *= 0.5;
  std::vector<int32_t> group_of(e->n, -1);
  std::vector<swarm::ResetGroup> dev(std::max(n_groups, 1));
  for (int g = 0; g < n_groups; ++g) {
    const swarm_reset_group_t& s = groups[g];
    if (s.first < 0 || s.count < 0 || (int64_t)s.first + s.count > e->n)
      return fail(SWARM_EINVAL, "reset group " + std::to_string(g) + " is out of range");
    if (!std::isfinite(s.radius) || s.radius < 0.0)
      return fail(SWARM_EINVAL, "reset group " + std::to_string(g) +
                                    ": the radius must be finite and >= 0");
    if (!(s.radius <= half))
      return fail(SWARM_EINVAL, "reset group " + std::to_string(g) +
                                    ": the radius exceeds half the shortest box edge");
    swarm::ResetGroup& r = dev[g];
    r = swarm::ResetGroup{};
    for (int a = 0; a < D; ++a) {
      if (!std::isfinite(s.centre[a]))
        return fail(SWARM_EINVAL, "reset group " + std::to_string(g) + ": non-finite centre");
      to_fixed(s.centre[a], e->params.box[a], &r.cq[a], &r.cimg[a]);
    }
    r.radius = (float)s.radius;
    for (int i = s.first; i < s.first + s.count; ++i) {
      if (group_of[i] != -1) return fail(SWARM_EINVAL, "reset groups overlap");
      // (a group of radius 0 places nothing: its particles go home)
      group_of[i] = s.radius > 0.0 ? g : -2;
    }
  }
  for (int32_t& g : group_of) g = std::max(g, -1);
  HostState h;
  state_to_fixed(e, pos, director, &h);

  const size_t M = (size_t)e->st.m;
  if (!e->d_home_q) {
    HIP_TRY(dev_malloc(e, &e->d_home_q, 3 * M * sizeof(uint32_t)));
    HIP_TRY(dev_malloc(e, &e->d_home_img, 3 * M * sizeof(int32_t)));
    HIP_TRY(dev_malloc(e, &e->d_home_ang, M * sizeof(uint32_t)));
    if (D == 3) HIP_TRY(dev_malloc(e, &e->d_home_dir3, 3 * M * sizeof(float)));
    HIP_TRY(dev_malloc(e, &e->d_group_of, (size_t)e->n * sizeof(int32_t)));
    HIP_TRY(dev_malloc(e, &e->d_reset_envs, (size_t)e->n_envs * sizeof(int32_t)));
    HIP_TRY(dev_malloc(e, &e->d_reset_counts, (size_t)e->n_envs * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(e->d_reset_counts, 0, (size_t)e->n_envs * sizeof(uint32_t),
                           e->stream));
  }
  if (dev.size() > e->groups_cap) {
    e->has_reset_plan = false;
    e->groups_cap = 0;
    HIP_TRY(dev_free(e, &e->d_groups));
    HIP_TRY(dev_malloc(e, &e->d_groups, dev.size() * sizeof(swarm::ResetGroup)));
    e->groups_cap = dev.size();
  }
  HIP_TRY(hipMemcpyAsync(e->d_home_q, h.q.data(), 3 * M * sizeof(uint32_t), hipMemcpyHostToDevice,
                         e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_home_img, h.img.data(), 3 * M * sizeof(int32_t),
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_home_ang, h.ang.data(), M * sizeof(uint32_t), hipMemcpyHostToDevice,
                         e->stream));
  if (D == 3)
    HIP_TRY(hipMemcpyAsync(e->d_home_dir3, h.d3.data(), 3 * M * sizeof(float),
                           hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_group_of, group_of.data(), group_of.size() * sizeof(int32_t),
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_groups, dev.data(), dev.size() * sizeof(swarm::ResetGroup),
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->has_reset_plan = true;
  return SWARM_OK;
}

int swarm_engine_download_reuse_slots(swarm_engine_t* e, float* f_prev, float* tz_prev,
                                      uint32_t* ang_prev, float* dir3_prev, float* txy_prev) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  const bool three_d = e->params.n_dims == 3;
  auto get = [&](void* dst, const void* src, size_t bytes) {
    return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream) : hipSuccess;
  };
  HIP_TRY(get(f_prev, e->st.f_prev, 2 * M * sizeof(float)));
  HIP_TRY(get(tz_prev, e->st.tz_prev, 2 * M * sizeof(float)));
  HIP_TRY(get(ang_prev, e->st.ang_prev, 2 * M * sizeof(uint32_t)));
  if (three_d) {
    HIP_TRY(get(dir3_prev, e->st.dir3_prev, 6 * M * sizeof(float)));
    HIP_TRY(get(txy_prev, e->st.txy_prev, 4 * M * sizeof(float)));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_reset_envs(swarm_engine_t* e, const uint8_t* env_mask, int32_t sd_steps,
                            double gamma, double max_disp) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  // their per-env kernels take the workgroup's index as the env
  if (e->has_rod || e->has_ell || e->has_lv)
    return fail(SWARM_EINVAL,
                "reset in place is not supported with a rod, ellipsoids or the Langevin "
                "thermostat");
  if (sd_steps < 0) return fail(SWARM_EINVAL, "sd_steps must be >= 0");
  if (!e->has_reset_plan) return fail(SWARM_ESTATE, "no reset plan (swarm_engine_set_reset_plan)");
  std::vector<int32_t> envs;
  for (int32_t k = 0; k < e->n_envs; ++k)
    if (!env_mask || env_mask[k]) envs.push_back(k);
  if (envs.empty()) return SWARM_OK;
  // the listed envs' positions change under a pending build and the vision grid
  e->prebuilt = false;
  e->ride_stage = 0;
  e->prebuilt_noise_steps = 0;
  e->vgrid_ready = false;
  HIP_TRY(hipMemcpyAsync(e->d_reset_envs, envs.data(), envs.size() * sizeof(int32_t),
                         hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));  // (envs is this call's)
  const int n_listed = (int)envs.size();
  if (const int rc = launch_place(e, n_listed)) return rc;
  ++e->reset_ordinal;
  if (sd_steps == 0) return SWARM_OK;
  e->stepped = true;
  return launch_global_envs(e, n_listed, sd_steps, (float)gamma, (float)max_disp);
}

int swarm_engine_reset_marked(swarm_engine_t* e, const uint8_t* d_mask, int32_t sd_steps,
                              double gamma, double max_disp) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (e->has_rod || e->has_ell || e->has_lv)
    return fail(SWARM_EINVAL,
                "reset in place is not supported with a rod, ellipsoids or the Langevin "
                "thermostat");
  if (sd_steps < 0) return fail(SWARM_EINVAL, "sd_steps must be >= 0");
  if (!d_mask) return fail(SWARM_EINVAL, "null mask");
  if (!e->has_reset_plan) return fail(SWARM_ESTATE, "no reset plan (swarm_engine_set_reset_plan)");
  // the host cannot know whether an env is marked: as if one were
  e->prebuilt = false;
  e->ride_stage = 0;
  e->prebuilt_noise_steps = 0;
  e->vgrid_ready = false;
  if (const int rc = launch_place_marked(e, d_mask)) return rc;
  if (sd_steps == 0) return SWARM_OK;
  e->stepped = true;
  return launch_global_marked(e, d_mask, sd_steps, (float)gamma, (float)max_disp);
}

int swarm_engine_reset_counts(swarm_engine_t* e, uint32_t* counts) {
  if (!e || !counts) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (!e->d_reset_counts) {  // (no plan yet: no marked reset can have run)
    std::memset(counts, 0, (size_t)e->n_envs * sizeof(uint32_t));
    return SWARM_OK;
  }
  HIP_TRY(hipMemcpyAsync(counts, e->d_reset_counts, (size_t)e->n_envs * sizeof(uint32_t),
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_field_history_marked(swarm_engine_t* e, const uint8_t* d_mask, const int32_t* agent_idx,
                               int32_t n_agents, uint32_t* hist_q, int32_t* hist_img) {
  if (!e || !d_mask || !agent_idx || !hist_q || !hist_img)
    return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (n_agents <= 0) return SWARM_OK;
  const long items = (long)n_agents * e->n_envs;
  hipLaunchKernelGGL(swarm::k_field_history_marked, dim3((unsigned)((items + 255) / 256)),
                     dim3(256), 0, e->stream, e->st, d_mask, agent_idx, n_agents, e->n_envs,
                     hist_q, hist_img);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int swarm_engine_integrate(swarm_engine_t* e, int32_t n_steps) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (n_steps < 0) return fail(SWARM_EINVAL, "n_steps must be >= 0");
  if (n_steps == 0) return SWARM_OK;
  e->stepped = true;
  return run_bd(e, n_steps);
}

namespace {
// Sum the event pairs (all recorded launches have run), destroy them.
int read_event_pairs(std::vector<std::pair<hipEvent_t, hipEvent_t>>& ev, double* total_ms,
                     int32_t* count) {
  double total = 0.0;
  int rc = SWARM_OK;
  for (auto& pr : ev) {
    float ms = 0.0f;
    if (rc == SWARM_OK) {
      hipError_t err = hipEventSynchronize(pr.second);
      if (err == hipSuccess) err = hipEventElapsedTime(&ms, pr.first, pr.second);
      if (err != hipSuccess) rc = fail(SWARM_EDEVICE, hipGetErrorString(err));
    }
    total += ms;
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  if (total_ms) *total_ms = total;
  if (count) *count = (int32_t)ev.size();
  ev.clear();
  return rc;
}
}  // namespace

int swarm_engine_profile(swarm_engine_t* e, int32_t enable, double* run_ms, int32_t* launches) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  const int rc = read_event_pairs(e->prof_events, run_ms, launches);
  e->profile = enable != 0;
  // the launch stamps of captured run nodes (allocated here: never under capture)
  if (e->profile && !e->d_tstamp)
    HIP_TRY(dev_malloc(e, &e->d_tstamp, 2 * (size_t)kMaxStamps * swarm::kStampSub *
                                            sizeof(unsigned long long)));
  if (e->profile && !e->d_rstamp)
    HIP_TRY(dev_malloc(e, &e->d_rstamp, 2 * (size_t)kMaxStamps * swarm::kRoles *
                                            swarm::kStampSub * sizeof(unsigned long long)));
  if (!e->profile) e->sc.rstamp = nullptr;
  return rc;
}

int swarm_engine_profile_graph(swarm_engine_t* e, int32_t release, float* ms_out, float* cal_out,
                               int32_t cap, int32_t* launches) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (cap < 0 || (cap > 0 && !ms_out)) return fail(SWARM_EINVAL, "ms_out needs cap entries");
  // the replay ran on a stream the engine does not know: wait for the device
  HIP_TRY(hipDeviceSynchronize());
  int rc = SWARM_OK;
  auto read = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, float* out) {
    int k = 0;
    for (auto& pr : v) {
      float ms = 0.0f;
      const hipError_t err = hipEventElapsedTime(&ms, pr.first, pr.second);
      if (err != hipSuccess && rc == SWARM_OK) rc = fail(SWARM_EDEVICE, hipGetErrorString(err));
      if (out && k < cap) out[k] = ms;
      ++k;
    }
    return k;
  };
  const int k = read(e->graph_events, ms_out);
  read(e->graph_cal, cal_out);
  if (launches) *launches = k;
  if (release) {
    for (auto* v : {&e->graph_events, &e->graph_cal}) {
      for (auto& pr : *v) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
      }
      v->clear();
    }
    e->stamp_next = 0;
  }
  return rc;
}

namespace {
// The (min start, max end) of each of `n` stamp records of kStampSub pairs.
void reduce_stamps(const std::vector<unsigned long long>& raw, int n,
                   std::vector<unsigned long long>* out) {
  out->assign(2 * (size_t)n, 0ull);
  for (int k = 0; k < n; ++k) {
    unsigned long long b = ~0ull, en = 0ull;
    for (int j = 0; j < swarm::kStampSub; ++j) {
      b = std::min(b, raw[2 * ((size_t)k * swarm::kStampSub + j)]);
      en = std::max(en, raw[2 * ((size_t)k * swarm::kStampSub + j) + 1]);
    }
    (*out)[2 * (size_t)k] = b;
    (*out)[2 * (size_t)k + 1] = en;
  }
}

// The run nodes' (start, end) stamps, reduced over their pairs.
int read_run_stamps(swarm_engine* e, std::vector<unsigned long long>* t) {
  const int n = e->stamp_next;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<unsigned long long> raw(2 * (size_t)n * swarm::kStampSub);
  HIP_TRY(hipMemcpy(raw.data(), e->d_tstamp, raw.size() * sizeof(unsigned long long),
                    hipMemcpyDeviceToHost));
  reduce_stamps(raw, n, t);
  return SWARM_OK;
}

__global__ void k_stamp_reset(unsigned long long* t, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) {
    t[2 * k] = ~0ull;
    t[2 * k + 1] = 0ull;
  }
}
}  // namespace

int swarm_engine_profile_stamps(swarm_engine_t* e, int32_t reset, void* stream, float* ms_out,
                                int32_t cap, int32_t* launches) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  const int n = e->stamp_next;
  if (launches) *launches = n;
  if (!e->d_tstamp || n == 0) return SWARM_OK;
  if (reset) {
    const int nt = n * swarm::kStampSub;
    hipLaunchKernelGGL(k_stamp_reset, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), e->d_tstamp, nt);
    if (e->d_rstamp) {
      const int nr = n * swarm::kRoles * swarm::kStampSub;
      hipLaunchKernelGGL(k_stamp_reset, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0,
                         reinterpret_cast<hipStream_t>(stream), e->d_rstamp, nr);
    }
    HIP_TRY(hipGetLastError());
    return SWARM_OK;
  }
  if (cap < 0 || (cap > 0 && !ms_out)) return fail(SWARM_EINVAL, "ms_out needs cap entries");
  std::vector<unsigned long long> t;
  int rc = read_run_stamps(e, &t);
  if (rc) return rc;
  int dev = 0, khz = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
  if (khz <= 0) return fail(SWARM_EDEVICE, "no wall clock rate");
  for (int k = 0; k < n && k < cap; ++k)
    ms_out[k] = t[2 * k + 1] > t[2 * k] ? (float)((double)(t[2 * k + 1] - t[2 * k]) / khz) : 0.0f;
  return SWARM_OK;
}

int swarm_engine_profile_roles(swarm_engine_t* e, double* us_out, int32_t cap,
                               int32_t* n_roles) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (n_roles) *n_roles = swarm::kRoles;
  const int n = e->stamp_next;
  if (cap < 0 || (cap > 0 && !us_out)) return fail(SWARM_EINVAL, "us_out needs cap entries");
  const size_t per = 2 * (size_t)swarm::kRoles;
  for (int32_t k = 0; k < cap; ++k) us_out[k] = std::nan("");
  if (!e->d_tstamp || !e->d_rstamp || n == 0) return SWARM_OK;
  std::vector<unsigned long long> t, r;
  int rc = read_run_stamps(e, &t);
  if (rc) return rc;
  std::vector<unsigned long long> raw(per * n * swarm::kStampSub);
  HIP_TRY(hipMemcpy(raw.data(), e->d_rstamp, raw.size() * sizeof(unsigned long long),
                    hipMemcpyDeviceToHost));
  reduce_stamps(raw, n * swarm::kRoles, &r);
  int dev = 0, khz = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
  if (khz <= 0) return fail(SWARM_EDEVICE, "no wall clock rate");
  const double us_per_tick = 1000.0 / khz;
  for (int k = 0; k < n; ++k) {
    const unsigned long long ref = t[2 * k + 1];  // end of the k-th run node
    if (ref == 0) continue;
    for (int q = 0; q < swarm::kRoles; ++q) {
      const unsigned long long b = r[per * k + 2 * q], en = r[per * k + 2 * q + 1];
      const size_t o = per * k + 2 * q;
      if (b == ~0ull || en == 0 || o + 1 >= (size_t)cap) continue;
      us_out[o] = ((double)b - (double)ref) * us_per_tick;
      us_out[o + 1] = ((double)en - (double)ref) * us_per_tick;
    }
  }
  return SWARM_OK;
}

int swarm_engine_time_run(swarm_engine_t* e, int32_t n_steps, int32_t reps, double* run_ms) {
  if (!e || !run_ms) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (n_steps < 1 || n_steps > swarm::kMaxWindow || reps < 1)
    return fail(SWARM_EINVAL, "1 <= n_steps <= 128 and reps >= 1");
  if (!e->plan.cluster_path || e->plan.nlist_path || e->params.n_dims != 2)
    return fail(SWARM_ESTATE, "swarm_engine_time_run times the 2-D cluster window only");
  if (e->prebuilt) {  // a pending side-stream build would race with this one
    HIP_TRY(hipDeviceSynchronize());
    e->prebuilt = false;
  }
  e->ride_stage = 0;  // a deferred build is superseded by the one below
  int rc = launch_build(e, e->stream);
  if (!rc && e->plan.noise_table && !e->next_table_ready) rc = launch_noise(e, e->stream, n_steps);
  if (rc) return rc;
  hipEvent_t ev0, ev1;
  HIP_TRY(hipEventCreate(&ev0));
  HIP_TRY(hipEventCreate(&ev1));
  HIP_TRY(hipEventRecord(ev0, e->stream));
  for (int r = 0; r < reps && !rc; ++r) rc = launch_run(e, n_steps);
  HIP_TRY(hipEventRecord(ev1, e->stream));
  // the exact check restores a consistent state (the repeated windows ran on
  // one decomposition and their movers overflow the list: exact re-run)
  if (!rc) rc = launch_check(e, n_steps);
  float ms = 0.0f;
  hipError_t err = hipEventSynchronize(ev1);
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev0, ev1);
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  if (rc) return rc;
  if (err != hipSuccess) return fail(SWARM_EDEVICE, hipGetErrorString(err));
  *run_ms = (double)ms / reps;
  return SWARM_OK;
}

int swarm_engine_debug_phases(swarm_engine_t* e, uint64_t* out32) {
  if (!e || !out32) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out32, e->sc.phase, 32 * sizeof(uint64_t), hipMemcpyDeviceToHost));
#ifdef SWARM_PHASE_TIMING
  HIP_TRY(hipMemcpyFromSymbol(out32 + 24, HIP_SYMBOL(swarm::g_global_phase), 3 * sizeof(uint64_t)));
#endif
  return SWARM_OK;
}

int swarm_engine_debug_wave_stamps(swarm_engine_t* e, uint64_t* out, int32_t n_words) {
  if (!e || !out) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t cap = 4 * (size_t)e->n_envs * (e->sc.S / 64);
  if (n_words < 0 || (size_t)n_words > cap) return fail(SWARM_EINVAL, "n_words out of range");
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(out, e->sc.phase + 32, (size_t)n_words * sizeof(uint64_t),
                    hipMemcpyDeviceToHost));
  return SWARM_OK;
}

int swarm_engine_prebuild(swarm_engine_t* e, void* stream, int32_t n_steps_hint) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (n_steps_hint < 0) return fail(SWARM_EINVAL, "n_steps_hint must be >= 0");
  if (!e->plan.cluster_path) return SWARM_OK;  // the global path has no build step
  const int rc = launch_build(e, stream ? reinterpret_cast<hipStream_t>(stream) : e->stream);
  if (rc) return rc;
  e->prebuilt = true;
  return SWARM_OK;
}

int swarm_engine_prebuild_noise(swarm_engine_t* e, void* stream, int32_t n_steps_hint) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (n_steps_hint < 0) return fail(SWARM_EINVAL, "n_steps_hint must be >= 0");
  if (!e->plan.noise_table || n_steps_hint == 0) return SWARM_OK;
  if (e->next_table_ready) return SWARM_OK;  // filled beside the last run
  const int n = std::min<int>(n_steps_hint, swarm::kMaxWindow);
  const int rc = launch_noise(e, stream ? reinterpret_cast<hipStream_t>(stream) : e->stream, n);
  if (rc) return rc;
  e->prebuilt_noise_steps = n;
  return SWARM_OK;
}

int swarm_engine_build_stats(swarm_engine_t* e, uint64_t* out4, int32_t reset) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (!e->sc.stats) {  // (not a cluster-window engine)
    if (out4) std::memset(out4, 0, 4 * sizeof(uint64_t));
    return SWARM_OK;
  }
  if (out4) {
    HIP_TRY(hipMemcpyAsync(out4, e->sc.stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (reset) HIP_TRY(hipMemsetAsync(e->sc.stats, 0, 4 * sizeof(uint64_t), e->stream));
  return SWARM_OK;
}

int swarm_engine_hint_defer_check(swarm_engine_t* e) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  e->defer_hint = e->plan.defer_check;
  return SWARM_OK;
}

int swarm_engine_flush_check(swarm_engine_t* e) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  e->defer_hint = false;
  return flush_check(e);
}

int swarm_engine_check_stats(swarm_engine_t* e, uint64_t* out4, int32_t reset) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (!e->sc.cstats) {  // (no check of this engine can ride in the reward launch)
    if (out4) std::memset(out4, 0, 4 * sizeof(uint64_t));
    return SWARM_OK;
  }
  if (out4) {
    HIP_TRY(hipMemcpyAsync(out4, e->sc.cstats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  if (reset) HIP_TRY(hipMemsetAsync(e->sc.cstats, 0, 4 * sizeof(uint64_t), e->stream));
  return SWARM_OK;
}

int swarm_engine_window_stats(swarm_engine_t* e, int32_t* fallback, int32_t* waves) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  const size_t E = (size_t)e->n_envs;
  if (fallback)
    HIP_TRY(hipMemcpyAsync(fallback, e->sc.fallback, E * sizeof(int32_t), hipMemcpyDeviceToHost,
                           e->stream));
  if (waves)
    HIP_TRY(hipMemcpyAsync(waves, e->sc.env_waves, E * sizeof(int32_t), hipMemcpyDeviceToHost,
                           e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

// ---------------------------------------------------- trajectory ring
static size_t traj_entry_bytes(int n, int dims) {
  const size_t b = 8 + 4 * (size_t)n * (size_t)(3 * dims + (dims == 3 ? 3 : 1));
  return (b + 255) & ~(size_t)255;
}

int swarm_engine_traj_ring(swarm_engine_t* e, int32_t capacity, int32_t env, void** host_ring,
                           int64_t* entry_bytes) {
  if (!e || !host_ring || !entry_bytes) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (capacity < 1 || env < 0 || env >= e->n_envs)
    return fail(SWARM_EINVAL, "trajectory ring: capacity >= 1 and 0 <= env < n_envs");
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (e->traj_host) {
    HIP_TRY(hipHostFree(e->traj_host));
    e->traj_host = e->traj_dev = nullptr;
  }
  if (!e->d_traj_count) HIP_TRY(dev_malloc(e, &e->d_traj_count, sizeof(uint64_t)));
  HIP_TRY(hipMemset(e->d_traj_count, 0, sizeof(uint64_t)));
  const size_t eb = traj_entry_bytes(e->n, e->params.n_dims);
  const size_t bytes = 64 + eb * (size_t)capacity;
  void* h = nullptr;
  HIP_TRY(hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(h, 0, bytes);
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    (void)hipHostFree(h);
    return fail(SWARM_EDEVICE, "hipHostGetDevicePointer failed");
  }
  e->traj_host = reinterpret_cast<unsigned char*>(h);
  e->traj_dev = reinterpret_cast<unsigned char*>(d);
  e->traj_cap = capacity;
  e->traj_env = env;
  e->traj_entry = eb;
  *host_ring = h;
  *entry_bytes = (int64_t)eb;
  return SWARM_OK;
}

int swarm_engine_traj_record(swarm_engine_t* e) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (!e->traj_dev) return fail(SWARM_ESTATE, "no trajectory ring (swarm_engine_traj_ring)");
  hipLaunchKernelGGL(k_traj_write, dim3((unsigned)((e->n + 255) / 256)), dim3(256), 0, e->stream,
                     e->st, e->traj_env, e->traj_dev, e->traj_cap, e->traj_entry,
                     e->d_traj_count, e->d_step);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_traj_bump, dim3(1), dim3(64), 0, e->stream, e->d_traj_count, e->traj_dev);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int swarm_traj_entry_to_host(const swarm_engine_t* e, const void* entry, double* pos,
                             double* director, double* velocity, uint64_t* step) {
  if (!e || !entry) return fail(SWARM_EINVAL, "null argument");
  const int N = e->n, D = e->params.n_dims;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(entry);
  if (step) std::memcpy(step, b, 8);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(b + 8);
  const int32_t* img = reinterpret_cast<const int32_t*>(q + (size_t)D * N);
  const uint32_t* ang = reinterpret_cast<const uint32_t*>(img + (size_t)D * N);
  const float* d3 = reinterpret_cast<const float*>(ang);
  const float* vel = reinterpret_cast<const float*>(ang + (D == 3 ? (size_t)3 * N : (size_t)N));
  for (size_t g = 0; g < (size_t)N; ++g) {  // as swarm_engine_download_state
    if (pos)
      for (int a = 0; a < 3; ++a)
        pos[3 * g + a] = a < D ? ((double)img[a * N + g] + (double)q[a * N + g] / kTwo32) *
                                     e->params.box[a]
                               : 0.0;
    if (director && D == 3) {
      for (int a = 0; a < 3; ++a) director[3 * g + a] = d3[a * N + g];
    } else if (director) {
      float so, co;
      host_sincos_turn(ang[g], &so, &co);
      director[3 * g + 0] = co;
      director[3 * g + 1] = so;
      director[3 * g + 2] = 0.0;
    }
    if (velocity)
      for (int a = 0; a < 3; ++a) velocity[3 * g + a] = a < D ? vel[a * N + g] : 0.0;
  }
  return SWARM_OK;
}

int swarm_rnd_distance(const float* x, int32_t n, int32_t d_in, int32_t width,
                       const float* const* target, const float* const* predictor, int32_t order,
                       float* out, void* stream) {
  if (!x || !target || !predictor || !out) return fail(SWARM_EINVAL, "null argument");
  if (width != swarm::kRndWidth) return fail(SWARM_ECAPACITY, "RND width must be 32");
  if (d_in < 1 || d_in > swarm::kRndMaxIn) return fail(SWARM_ECAPACITY, "1 <= d_in <= 16");
  if (order < 1) return fail(SWARM_EINVAL, "distance order must be >= 1");
  swarm::RndPtrs tp, pp;
  for (int k = 0; k < 6; ++k) {
    if (!target[k] || !predictor[k]) return fail(SWARM_EINVAL, "null parameter");
    tp.w[k] = target[k];
    pp.w[k] = predictor[k];
  }
  if (n <= 0) return SWARM_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  if (d_in <= 4)
    hipLaunchKernelGGL(swarm::k_rnd_distance<4>, dim3(blocks), dim3(256), 0, s, x, n, d_in, tp,
                       pp, order, out);
  else
    hipLaunchKernelGGL(swarm::k_rnd_distance<16>, dim3(blocks), dim3(256), 0, s, x, n, d_in, tp,
                       pp, order, out);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

namespace {
// swarm_rnd_env_reward's workspace: the blocks' fp64 partials, then one
// ticket per env (zero between calls: the caller zeroes it once).
// Workgroups per env: one per 32-observation group (capping them at 64 or
// 128 so that each stages the networks once for several groups measured
// slower: C5 106.8 -> 100.9 M, same box).
int rnd_blocks(int per_env) {
  return (per_env + swarm::kRndObsPerBlock - 1) / swarm::kRndObsPerBlock;
}
size_t rnd_partials_bytes(int n_envs, int per_env) {
  return ((size_t)n_envs * rnd_blocks(per_env) * sizeof(double) + 255) & ~(size_t)255;
}
}  // namespace

int swarm_rnd_env_reward(const float* x, int32_t n_envs, int32_t per_env, int32_t d_in,
                         int32_t width, const float* const* target, const float* const* predictor,
                         int32_t order, int32_t clip, float clip_lo, float clip_hi,
                         const float* base, float* metric, float* env_reward, float* rewards,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !target || !predictor || !metric || !env_reward || !rewards || !workspace)
    return fail(SWARM_EINVAL, "null argument");
  if (width != swarm::kRndWidth) return fail(SWARM_ECAPACITY, "RND width must be 32");
  if (d_in < 1 || d_in > swarm::kRndMaxIn) return fail(SWARM_ECAPACITY, "1 <= d_in <= 16");
  if (order < 1) return fail(SWARM_EINVAL, "distance order must be >= 1");
  if (n_envs < 0 || per_env < 0) return fail(SWARM_EINVAL, "n_envs, per_env >= 0");
  if (n_envs == 0 || per_env == 0) return SWARM_OK;
  const int kb = rnd_blocks(per_env);
  const size_t pb = rnd_partials_bytes(n_envs, per_env);
  if (workspace_bytes < (int64_t)(pb + (size_t)n_envs * sizeof(uint32_t)))
    return fail(SWARM_ECAPACITY, "workspace below swarm_rnd_env_workspace_bytes");
  swarm::RndPtrs tp, pp;
  for (int k = 0; k < 6; ++k) {
    if (!target[k] || !predictor[k]) return fail(SWARM_EINVAL, "null parameter");
    tp.w[k] = target[k];
    pp.w[k] = predictor[k];
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* partial = static_cast<double*>(workspace);
  uint32_t* tickets = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + pb);
  const dim3 grid((unsigned)kb, (unsigned)n_envs);
  if (d_in <= 4)
    hipLaunchKernelGGL(swarm::k_rnd_env<4>, grid, dim3(256), 0, s, x, per_env, d_in, tp, pp,
                       order, clip ? 1 : 0, clip_lo, clip_hi, base, metric, env_reward, rewards,
                       partial, tickets);
  else
    hipLaunchKernelGGL(swarm::k_rnd_env<16>, grid, dim3(256), 0, s, x, per_env, d_in, tp, pp,
                       order, clip ? 1 : 0, clip_lo, clip_hi, base, metric, env_reward, rewards,
                       partial, tickets);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int64_t swarm_rnd_env_workspace_bytes(int32_t n_envs, int32_t per_env) {
  if (n_envs < 0 || per_env < 0) return -1;
  return (int64_t)(rnd_partials_bytes(n_envs, per_env) + (size_t)n_envs * sizeof(uint32_t));
}

int swarm_rnd_targets(const float* x, int32_t n, int32_t d_in, int32_t width,
                      const float* const* target, float* y, void* stream) {
  if (!x || !target || !y) return fail(SWARM_EINVAL, "null argument");
  if (width != swarm::kRndWidth) return fail(SWARM_ECAPACITY, "RND width must be 32");
  if (d_in < 1 || d_in > swarm::kRndMaxIn) return fail(SWARM_ECAPACITY, "1 <= d_in <= 16");
  if (n < 0) return fail(SWARM_EINVAL, "n >= 0");
  swarm::RndPtrs tp;
  for (int k = 0; k < 6; ++k) {
    if (!target[k]) return fail(SWARM_EINVAL, "null parameter");
    tp.w[k] = target[k];
  }
  if (n == 0) return SWARM_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)(((int64_t)n + 255) / 256);
  if (d_in <= 4)
    hipLaunchKernelGGL(swarm::k_rnd_targets<4>, dim3(blocks), dim3(256), 0, s, x, n, d_in, tp, y);
  else
    hipLaunchKernelGGL(swarm::k_rnd_targets<16>, dim3(blocks), dim3(256), 0, s, x, n, d_in, tp, y);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

namespace {
// Minibatch steps per launch of k_rnd_train: a step measured 2.6 us at B = 8
// and 11.7 us at B = 64, so a launch stays below 0.4 s;
// longer epochs (n / B beyond this) run as several launches on the stream,
// the state going through torch's tensors in between.
constexpr int kRndStepsPerLaunch = 32768;
}  // namespace

int swarm_rnd_train_epoch(const float* x, const float* y, const int64_t* perm, int32_t n,
                          int32_t d_in, int32_t width, int32_t batch_size, int32_t loss_order,
                          const swarm_adam_t* adam, float* loss_out, void* stream) {
  if (!x || !y || !perm || !adam) return fail(SWARM_EINVAL, "null argument");
  if (width != swarm::kRndWidth) return fail(SWARM_ECAPACITY, "RND width must be 32");
  if (d_in < 1 || d_in > swarm::kRndMaxIn) return fail(SWARM_ECAPACITY, "1 <= d_in <= 16");
  if (batch_size < 1 || batch_size > swarm::kRndMaxBatch)
    return fail(SWARM_ECAPACITY, "1 <= batch_size <= 64");
  if (loss_order < 1) return fail(SWARM_EINVAL, "loss order must be an integer >= 1");
  if (n < 0) return fail(SWARM_EINVAL, "n >= 0");
  if (!(adam->beta1 >= 0.0f && adam->beta1 < 1.0f && adam->beta2 >= 0.0f && adam->beta2 < 1.0f))
    return fail(SWARM_EINVAL, "Adam betas must be in [0, 1)");
  swarm::RndTrainArgs a;
  a.lr = adam->lr;
  a.beta1 = adam->beta1;
  a.beta2 = adam->beta2;
  a.eps = adam->eps;
  a.log2_beta1 = (float)std::log2((double)adam->beta1);
  a.log2_beta2 = (float)std::log2((double)adam->beta2);
  for (int t = 0; t < 6; ++t) {
    if (!adam->param[t] || !adam->exp_avg[t] || !adam->exp_avg_sq[t] || !adam->step[t])
      return fail(SWARM_EINVAL, "null Adam tensor");
    a.param[t] = adam->param[t];
    a.m[t] = adam->exp_avg[t];
    a.v[t] = adam->exp_avg_sq[t];
    a.step[t] = adam->step[t];
  }
  if (n == 0) return SWARM_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int steps = (int)(((int64_t)n + batch_size - 1) / batch_size);
  const int R = (batch_size + 7) / 8;
  const long long* pm = reinterpret_cast<const long long*>(perm);
  for (int s0 = 0; s0 < steps; s0 += kRndStepsPerLaunch) {
    const int s1 = std::min(steps, s0 + kRndStepsPerLaunch);
    if (R == 1)
      hipLaunchKernelGGL(swarm::k_rnd_train<1>, dim3(1), dim3(256), 0, s, x, y, pm, n, d_in,
                         batch_size, loss_order, s0, s1, a, loss_out);
    else if (R == 2)
      hipLaunchKernelGGL(swarm::k_rnd_train<2>, dim3(1), dim3(256), 0, s, x, y, pm, n, d_in,
                         batch_size, loss_order, s0, s1, a, loss_out);
    else if (R <= 4)
      hipLaunchKernelGGL(swarm::k_rnd_train<4>, dim3(1), dim3(256), 0, s, x, y, pm, n, d_in,
                         batch_size, loss_order, s0, s1, a, loss_out);
    else
      hipLaunchKernelGGL(swarm::k_rnd_train<8>, dim3(1), dim3(256), 0, s, x, y, pm, n, d_in,
                         batch_size, loss_order, s0, s1, a, loss_out);
    HIP_TRY(hipGetLastError());
  }
  return SWARM_OK;
}

int64_t swarm_engine_step_count(const swarm_engine_t* e) {
  if (!e) return -1;
  // (the pending check advances the counter; its flush changes no field a
  // caller of this const entry can see)
  if (flush_check(const_cast<swarm_engine_t*>(e))) return -1;
  uint64_t v = 0;
  if (hipMemcpyAsync(&v, e->d_step, sizeof(v), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
      hipStreamSynchronize(e->stream) != hipSuccess)
    return -1;
  return (int64_t)v;
}

int swarm_engine_device_views(swarm_engine_t* e, swarm_device_views_t* v) {
  if (!e || !v) return fail(SWARM_EINVAL, "null argument");
  v->q = e->st.q;
  v->img = e->st.img;
  v->ang = e->st.ang;
  v->f_swim = e->st.f_swim;
  v->torque_z = e->st.torque_z;
  v->f_ext = e->st.f_ext;
  v->vel = e->st.vel;
  v->omega_z = e->st.omega;
  v->species = e->st.species;
  v->n_envs = e->n_envs;
  v->n_particles = e->n;
  v->n_dims = e->params.n_dims;
  v->dir3 = e->st.dir3;
  v->torque_xy = e->st.torque_xy;
  v->omega_xy = e->st.omega_xy;
  return SWARM_OK;
}

int swarm_vision_cone(swarm_engine_t* e, const swarm_vision_params_t* vp, const int32_t* agent_idx,
                      int32_t n_agents, const float* radii, const int32_t* types, float* out) {
  return vision_cone_impl(e, vp, agent_idx, n_agents, radii, types, out, false);
}

int swarm_vision_cone_persistent(swarm_engine_t* e, const swarm_vision_params_t* vp,
                                 const int32_t* agent_idx, int32_t n_agents, const float* radii,
                                 const int32_t* types, float* out) {
  return vision_cone_impl(e, vp, agent_idx, n_agents, radii, types, out, true);
}

namespace {
int policy_launch(const float* obs, int32_t n, int32_t d_in, const float* w1, const float* b1,
                  int32_t hidden, const float* w2, const float* b2, int32_t k, uint64_t seed,
                  uint64_t* state, int32_t n_state, float explore_p, const float* f_table,
                  const float* t_table, int64_t* out_idx, float* out_logp, float* out_f,
                  float* out_t, float* out_logits, void* stream, swarm_engine* ride);
}  // namespace

int swarm_engine_vision_policy(swarm_engine_t* e, const swarm_vision_params_t* vp,
                               const int32_t* agent_idx, int32_t n_agents, const float* radii,
                               const int32_t* types, float* features, const float* w1,
                               const float* b1, int32_t hidden, const float* w2, const float* b2,
                               int32_t k, uint64_t seed, uint64_t* agent_state, int32_t n_state,
                               float explore_p, const float* f_table, const float* t_table,
                               int64_t* out_idx, float* out_logp, float* out_f, float* out_t,
                               float* out_logits) {
  if (!e || !vp || !w1 || !b1 || !w2 || !b2 || !agent_state || !f_table || !t_table || !out_idx ||
      !out_logp || !out_f || !out_t)
    return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const int nb = vp->n_cones * vp->n_types;
  if (nb < 1 || nb > 4) return fail(SWARM_ECAPACITY, "the fused policy takes <= 4 cone bins");
  if (hidden < 1 || hidden > swarm::kMlpMaxHidden)
    return fail(SWARM_ECAPACITY, "1 <= hidden <= 256");
  if (k < 1 || k > 4) return fail(SWARM_ECAPACITY, "the fused policy takes 1 <= k <= 4 actions");
  if (!(explore_p >= 0.0f && explore_p <= 1.0f))
    return fail(SWARM_EINVAL, "exploration probability must be in [0, 1]");
  if (n_agents <= 0) return SWARM_OK;
  const long n = (long)e->n_envs * n_agents;
  if (n_state < n) return fail(SWARM_EINVAL, "agent_state needs one counter per agent");
  const swarm::MlpArgs m{features, (int)n, nb, w1, b1, hidden, w2, b2, k, (uint32_t)seed,
                         (uint32_t)(seed >> 32), reinterpret_cast<unsigned long long*>(agent_state),
                         explore_p, f_table, t_table, out_idx, out_logp, out_f, out_t, out_logits};
  if (!e->plan.wide_run) {
    // throughput-bound engines (many envs): the cone is VALU-bound and the
    // MLP's four lanes per agent would lengthen every group; the two kernels
    // of the calls this replaces, the policy drawing with the first
    // ceil(n / 64) counters as its group counters
    const int rc = vision_cone_impl(e, vp, agent_idx, n_agents, radii, types, features, true);
    if (rc) return rc;
    return policy_launch(features, (int32_t)n, nb, w1, b1, hidden, w2, b2, k, seed, agent_state,
                         n_state, explore_p, f_table, t_table, out_idx, out_logp, out_f, out_t,
                         out_logits, e->stream, e);
  }
  return vision_cone_impl(e, vp, agent_idx, n_agents, radii, types, features, true, &m);
}

int swarm_field_distance(swarm_engine_t* e, const int32_t* agent_idx, int32_t n_agents,
                         const double source[3], const double box_scale[3], uint32_t* hist_q,
                         int32_t* hist_img, float* d_cur, float* d_prev, int32_t update_history,
                         int32_t init_only) {
  if (!e || !agent_idx || !hist_q || !hist_img) return fail(SWARM_EINVAL, "null argument");
  if (!init_only && (!d_cur || !d_prev || !source || !box_scale)) return fail(SWARM_EINVAL, "null argument");
  if (n_agents <= 0) return SWARM_OK;
  const double s[3] = {source ? source[0] : 0.0, source ? source[1] : 0.0, source ? source[2] : 0.0};
  const double b[3] = {box_scale ? box_scale[0] : 1.0, box_scale ? box_scale[1] : 1.0,
                       box_scale ? box_scale[2] : 1.0};
  const FieldArgs f{e->d_box, agent_idx, n_agents, s[0], s[1], s[2], b[0], b[1], b[2], hist_q,
                    hist_img, d_cur, d_prev, update_history, init_only, e->n_envs, 0, 0.0f, 0.0f,
                    0.0f, nullptr};
  return launch_field(e, f);
}

int swarm_field_transform(swarm_engine_t* e, const int32_t* agent_idx, int32_t n_agents,
                          const double source[3], const double box_scale[3], uint32_t* hist_q,
                          int32_t* hist_img, float decay_a, float decay_b, float scale,
                          int32_t clip_at_zero, float* out) {
  if (!e || !agent_idx || !hist_q || !hist_img || !source || !box_scale || !out)
    return fail(SWARM_EINVAL, "null argument");
  if (n_agents <= 0) return SWARM_OK;
  const FieldArgs f{e->d_box, agent_idx, n_agents, source[0], source[1], source[2],
                    box_scale[0], box_scale[1], box_scale[2], hist_q, hist_img, nullptr, nullptr,
                    1, 0, e->n_envs, clip_at_zero ? 2 : 1, decay_a, decay_b, scale, out};
  return launch_field(e, f);
}

int swarm_pair_distances(swarm_engine_t* e, const int32_t* agent_idx, int32_t n_agents,
                         const int32_t* sensed_idx, int32_t m0, int32_t mc,
                         const double box_scale[3], float* out) {
  if (!e || !agent_idx || !sensed_idx || !box_scale || !out)
    return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (m0 < 0 || mc < 0) return fail(SWARM_EINVAL, "negative sensed range");
  if (n_agents <= 0 || mc == 0) return SWARM_OK;
  const dim3 grid((unsigned)((n_agents + 255) / 256), (unsigned)((mc + 255) / 256),
                  (unsigned)e->n_envs);
  hipLaunchKernelGGL(k_pair_dist, grid, dim3(256), 0, e->stream, e->st, e->d_box, agent_idx,
                     n_agents, sensed_idx, m0, mc, (float)box_scale[0], (float)box_scale[1],
                     (float)box_scale[2], out);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

int swarm_engine_neighbor_pairs(swarm_engine_t* e, int32_t env, double cutoff, int32_t* pairs,
                                int32_t max_pairs, int32_t* n_pairs) {
  if (!e || !pairs || !n_pairs) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (env < 0 || env >= e->n_envs) return fail(SWARM_EINVAL, "env out of range");
  if (e->params.n_dims != 2) return fail(SWARM_EINVAL, "neighbor_pairs is 2-D only");
  if (!(2.0 * cutoff < std::min(e->params.box[0], e->params.box[1])))
    return fail(SWARM_EINVAL, "cutoff must be below half the box length");
  int lx, ly;
  cell_grid(e->params, e->n, cutoff, &lx, &ly);
  int rc = build_grid(e, lx, ly);
  if (rc) return rc;
  if ((size_t)max_pairs > e->pairs_cap) {
    e->pairs_cap = 0;
    HIP_TRY(dev_free(e, &e->d_pairs));
    HIP_TRY(dev_malloc(e, &e->d_pairs, 2 * (size_t)std::max(max_pairs, 1) * sizeof(int32_t)));
    e->pairs_cap = (size_t)max_pairs;
  }
  HIP_TRY(hipMemsetAsync(e->d_count, 0, sizeof(int32_t), e->stream));
  const float c2 = (float)(cutoff * cutoff);
  hipLaunchKernelGGL(k_pairs, dim3((e->n + 255) / 256), dim3(256), 0, e->stream, e->st,
                     e->d_derived, env, c2, lx, ly, e->d_start, e->d_order, e->d_pairs, max_pairs,
                     e->d_count);
  HIP_TRY(hipGetLastError());
  int32_t cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, e->d_count, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *n_pairs = cnt;
  const int32_t got = std::min(cnt, max_pairs);
  if (got > 0)
    HIP_TRY(hipMemcpy(pairs, e->d_pairs, 2 * (size_t)got * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (cnt > max_pairs) return fail(SWARM_ECAPACITY, "more pairs than max_pairs");
  return SWARM_OK;
}

int swarm_engine_set_torque_xy(swarm_engine_t* e, const float* torque_xy, int32_t on_device) {
  if (!e || !torque_xy) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(hipMemcpyAsync(e->st.torque_xy, torque_xy, 2 * M * sizeof(float), kind, e->stream));
  if (!on_device) HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_upload_directors(swarm_engine_t* e, const float* dir3) {
  if (!e || !dir3) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  HIP_TRY(hipMemcpyAsync(e->st.dir3, dir3, 3 * M * sizeof(float), hipMemcpyHostToDevice,
                         e->stream));
  for (int k = 0; k < 2; ++k)
    HIP_TRY(hipMemcpyAsync(e->st.dir3_prev + k * 3 * M, dir3, 3 * M * sizeof(float),
                           hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_download_directors(swarm_engine_t* e, float* dir3) {
  if (!e || !dir3) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  HIP_TRY(hipMemcpyAsync(dir3, e->st.dir3, 3 * M * sizeof(float), hipMemcpyDeviceToHost,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_set_walls(swarm_engine_t* e, const swarm_wall_t* walls, int32_t n_walls) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (n_walls < 0 || n_walls > SWARM_MAX_WALLS) return fail(SWARM_ECAPACITY, "0 <= n_walls <= 16");
  if (n_walls > 0 && !walls) return fail(SWARM_EINVAL, "null walls");
  if (n_walls > 0 && e->has_rod) return fail(SWARM_EINVAL, "walls with a rod are not supported");
  if (n_walls > 0 && e->has_ell)
    return fail(SWARM_EINVAL, "walls with ellipsoids are not supported");
  Derived& d = e->derived;
  d.n_walls = n_walls;
  for (int k = 0; k < n_walls; ++k) {
    const swarm_wall_t& w = walls[k];
    float* o = d.wp[k];
    d.wkind[k] = w.kind;
    if (w.kind == 0) {
      for (int a = 0; a < 3; ++a) o[a] = (float)w.normal[a];
      o[3] = (float)w.offset;
    } else if (w.kind == 1) {
      const double la = std::sqrt(w.a[0] * w.a[0] + w.a[1] * w.a[1]);
      const double lb = std::sqrt(w.b[0] * w.b[0] + w.b[1] * w.b[1]);
      if (!(la > 0.0) || !(lb > 0.0)) return fail(SWARM_EINVAL, "degenerate wall");
      o[0] = (float)w.corner[0];
      o[1] = (float)w.corner[1];
      o[2] = (float)(w.a[0] / la);
      o[3] = (float)(w.a[1] / la);
      o[4] = (float)(w.b[0] / lb);
      o[5] = (float)(w.b[1] / lb);
      o[6] = (float)la;
      o[7] = (float)lb;
    } else {
      return fail(SWARM_EINVAL, "wall kind must be 0 (plane) or 1 (slab)");
    }
  }
  HIP_TRY(hipMemcpyAsync(e->d_derived, &e->derived, sizeof(Derived), hipMemcpyHostToDevice,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

// Gridded external potential (espresso.py:995-1036): the host field is
// copied to the device and described in Derived::pot; every
// integrator path but the rod kernel reads it (swarm_potential.cuh).  Like
// swarm_engine_set_walls it moves no particle, so a pending build stays valid.
int swarm_engine_set_potential_field(swarm_engine_t* e, const float* phi, int32_t nx, int32_t ny,
                                     int32_t nz, const double* spacing) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  Derived& d = e->derived;
  if (!phi) {  // remove the field (the device copy is kept for a later one)
    d.pot = swarm::PotentialField{};
  } else {
    if (!spacing) return fail(SWARM_EINVAL, "null spacing");
    if (e->has_rod) return fail(SWARM_EINVAL, "a potential with a rod is not supported");
    if (e->has_ell) return fail(SWARM_EINVAL, "a potential with ellipsoids is not supported");
    const int32_t n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a)
      if (n[a] < 1) return fail(SWARM_EINVAL, "grid counts must be positive");
    if (e->params.n_dims == 2 && nz != 1)
      return fail(SWARM_EINVAL, "a 2-D engine takes a potential with nz = 1");
    const uint64_t count = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    // 2-D: one record of its four corners per cell (swarm_potential.cuh)
    const bool records = e->params.n_dims == 2;
    const uint64_t words = records ? 4 * count : count;
    if ((uint64_t)nx * (uint64_t)ny > 0x7fffffffull || words > 0x7fffffffull)
      return fail(SWARM_EINVAL, "potential grid too large (32-bit indexing)");
    for (int a = 0; a < 3; ++a) {
      const double h = spacing[a], L = e->params.box[a];
      if (!std::isfinite(h) || !(h > 0.0)) return fail(SWARM_EINVAL, "grid spacing must be positive");
      if (!(std::fabs(n[a] * h - L) <= 1e-9 * L))
        return fail(SWARM_EINVAL, "the potential grid must tile the box");
    }
    for (uint64_t k = 0; k < count; ++k)
      if (!std::isfinite(phi[k])) return fail(SWARM_EINVAL, "non-finite potential value");
    std::vector<float> rec;
    if (records) {
      rec.resize((size_t)words);
      for (int32_t i = 0; i < nx; ++i) {
        const size_t r0 = (size_t)i * ny, r1 = (size_t)((i + 1) % nx) * ny;
        for (int32_t j = 0; j < ny; ++j) {
          const size_t j1 = (size_t)((j + 1) % ny);
          float* o = &rec[4 * (r0 + j)];
          o[0] = phi[r0 + j];
          o[1] = phi[r1 + j];
          o[2] = phi[r0 + j1];
          o[3] = phi[r1 + j1];
        }
      }
    }
    if (words > e->pot_cap) {
      // the new copy first: a failed allocation leaves the old field in place
      float* v = nullptr;
      HIP_TRY(dev_malloc(e, &v, words * sizeof(float)));
      if (e->d_pot) {
        // no kernel may find the old copy once it is freed: the device's
        // descriptor is cleared first, and the stream drained of its readers
        d.pot = swarm::PotentialField{};
        hipError_t err = hipMemcpyAsync(e->d_derived, &e->derived, sizeof(Derived),
                                        hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        if (err == hipSuccess) err = dev_free(e, &e->d_pot);
        if (err != hipSuccess) {
          (void)dev_free(e, &v);
          if (!e->d_pot) e->pot_cap = 0;
          return fail(SWARM_EDEVICE, std::string("potential field: ") + hipGetErrorString(err));
        }
      }
      e->d_pot = v;
      e->pot_cap = (size_t)words;
    }
    HIP_TRY(hipMemcpyAsync(e->d_pot, records ? rec.data() : phi, words * sizeof(float),
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // (rec is a local)
    d.pot.phi = e->d_pot;
    for (int a = 0; a < 3; ++a) {
      d.pot.n[a] = n[a];
      d.pot.inv_h[a] = (float)(1.0 / spacing[a]);
    }
  }
  HIP_TRY(hipMemcpyAsync(e->d_derived, &e->derived, sizeof(Derived), hipMemcpyHostToDevice,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_wall_violations(swarm_engine_t* e, uint64_t* count) {
  if (!e || !count) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  unsigned long long v = 0;
  HIP_TRY(hipMemcpyAsync(&v, e->st.wall_viol, sizeof(v), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *count = v;
  return SWARM_OK;
}

// An engine that takes a rod, ellipsoids or the Langevin thermostat:
// swarm::plan_no_cluster_windows, and nothing pending of what a window would
// have used.
static void no_cluster_windows(swarm_engine_t* e) {
  swarm::plan_no_cluster_windows(e->plan);
  e->defer_hint = false;
  e->prebuilt = false;
  e->prebuilt_noise_steps = 0;
  e->ride_stage = 0;
}

int swarm_engine_set_rod(swarm_engine_t* e, const swarm_rod_t* rod) {
  if (!e || !rod) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (e->has_rod) return fail(SWARM_EINVAL, "the engine already has a rod");
  if (e->has_ell) return fail(SWARM_EINVAL, "a rod with ellipsoids is not supported");
  if (e->has_lv) return fail(SWARM_EINVAL, "a rod under the Langevin thermostat is not supported");
  if (e->params.n_dims != 2) return fail(SWARM_EINVAL, "Rod can only be added in 2d");
  if (!e->params.periodic) return fail(SWARM_EINVAL, "a rod needs a periodic box");
  if (e->derived.n_walls) return fail(SWARM_EINVAL, "a rod with walls is not supported");
  if (e->derived.pot.phi) return fail(SWARM_EINVAL, "a rod with a potential is not supported");
  if (rod->n < 1 || rod->n % 2 != 1) return fail(SWARM_EINVAL, "n_particles must be uneven");
  if (rod->n > swarm::kRodMaxParticles)
    return fail(SWARM_ECAPACITY, "a rod has at most 255 particles");
  if (e->n > swarm::kRodMaxEnv)
    return fail(SWARM_ECAPACITY, "an engine with a rod has at most 4096 particles per env");
  if (rod->first < 0 || rod->first + rod->n > e->n)
    return fail(SWARM_EINVAL, "rod particles out of range");
  if (!(rod->delta > 0.0) || !std::isfinite(rod->delta))
    return fail(SWARM_EINVAL, "rod bead spacing must be positive");
  // every bead within half a box of the centre: its offset is one int32
  // fixed-point displacement (swarm_rod.cuh:rod_place)
  const double half = 0.5 * (rod->n - 1) * rod->delta;
  if (!(half < 0.49 * std::min(e->params.box[0], e->params.box[1])))
    return fail(SWARM_EINVAL, "the rod must be shorter than the box");
  const size_t lds =
      swarm::env_lds_words(e->n, 1 << (e->plan.lxg + e->plan.lyg), false, swarm::kRodTailWords) * 4;
  if (lds + sizeof(swarm::PairTables) > kMaxLds)
    return fail(SWARM_ECAPACITY, "env does not fit the LDS of one workgroup");
  e->rod.first = rod->first;
  e->rod.n = rod->n;
  e->rod.delta = (float)rod->delta;
  e->rod.fixed = rod->fixed ? 1 : 0;
  e->has_rod = true;
  no_cluster_windows(e);
  if (const int rc = launch_rod_snap(e)) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

// Ellipsoids (espresso.py:802-832, 420-436): the per-engine constants of
// k_ellipsoid_run (swarm_ellipsoid.cuh), in fp64 and rounded once.
int swarm_engine_set_ellipsoids(swarm_engine_t* e, const swarm_ellipsoids_t* ell) {
  if (!e || !ell) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (e->stepped)
    return fail(SWARM_ESTATE, "ellipsoids must be set before the first integrate or overlap removal");
  if (e->has_ell) return fail(SWARM_EINVAL, "the engine already has ellipsoids");
  if (e->has_lv)
    return fail(SWARM_EINVAL, "ellipsoids under the Langevin thermostat are not supported");
  const swarm_params_t& p = e->params;
  if (p.n_dims != 2) return fail(SWARM_EINVAL, "ellipsoids are 2-D only");
  if (!p.periodic) return fail(SWARM_EINVAL, "ellipsoids need a periodic box");
  if (e->has_rod) return fail(SWARM_EINVAL, "ellipsoids with a rod are not supported");
  if (e->derived.n_walls) return fail(SWARM_EINVAL, "ellipsoids with walls are not supported");
  if (e->derived.pot.phi) return fail(SWARM_EINVAL, "ellipsoids with a potential are not supported");
  const double k = ell->aspect_ratio;
  if (!(k > 0.0) || !std::isfinite(k)) return fail(SWARM_EINVAL, "aspect_ratio must be positive");
  for (int s = 0; s < p.n_species; ++s)
    if (!(ell->gamma_par[s] > 0.0) || !(ell->gamma_perp[s] > 0.0) ||
        !std::isfinite(ell->gamma_par[s]) || !std::isfinite(ell->gamma_perp[s]))
      return fail(SWARM_EINVAL, "the frictions along and across the director must be positive");
  const bool gb = k != 1.0;
  const double wide = 2.0 * std::max(k, 1.0 / k);
  int lx = e->plan.lxg, ly = e->plan.lyg;
  if (gb) {
    // Gay-Berne cutoff 2 (r_i + r_j) max(k, 1 / k) against WCA's r_i + r_j:
    // the grid of the widest pair (swarm::max_cutoff)
    const double rc = wide * swarm::max_cutoff(p);
    if (!(rc < 0.5 * std::min(p.box[0], p.box[1])))
      return fail(SWARM_EINVAL, "the Gay-Berne cutoff must be below half the box");
    cell_grid(p, e->n, rc, &lx, &ly);
  }
  const size_t fixed = swarm::kEllStaticLds;
  auto fits = [&](int n, int gx, int gy) {
    return swarm::env_lds_words(n, 1 << (gx + gy), true, 0) * 4 + fixed <= kMaxLds;
  };
  if (!fits(e->n, lx, ly)) {
    // 40 bytes of state per particle beside the cell counts and the pair
    // tables: the most this box and cutoff admit
    int limit = e->n, gx = lx, gy = ly;
    while (limit > 1 && !fits(limit, gx, gy)) {
      --limit;
      cell_grid(p, limit, gb ? wide * swarm::max_cutoff(p) : swarm::max_cutoff(p), &gx, &gy);
    }
    return fail(SWARM_ECAPACITY, "an engine with ellipsoids holds at most " +
                                     std::to_string(limit) +
                                     " particles per env in this box (the 160 KB of LDS of one"
                                     " workgroup)");
  }
  swarm::EllArgs a{};
  const double chi = (k * k - 1.0) / (k * k + 1.0);
  a.chi = (float)chi;
  a.hchi = (float)(0.5 * chi);
  a.chi2 = (float)(chi * chi);
  a.eps4 = (float)(4.0 * p.wca_epsilon);
  const double kT = p.kT, dt = p.time_step;
  for (int s = 0; s < p.n_species; ++s) {
    const double ga = ell->gamma_par[s], gq = ell->gamma_perp[s];
    a.mob_par[s] = (float)(dt / ga);
    a.mob_perp[s] = (float)(dt / gq);
    a.sig_par[s] = (float)std::sqrt(2.0 * kT * dt / ga);
    a.sig_perp[s] = (float)std::sqrt(2.0 * kT * dt / gq);
    a.inv_gpar[s] = (float)(1.0 / ga);
    a.inv_gperp[s] = (float)(1.0 / gq);
    for (int t = 0; t < p.n_species; ++t) {
      const double rs = p.radius[s] + p.radius[t];
      const double s0 = rs * std::pow(2.0, -1.0 / 6.0), rc = wide * rs;
      const int pk = s * swarm::kMaxSpecies + t;
      a.sig0[pk] = (float)s0;
      a.isig0[pk] = s0 > 0.0 ? (float)(1.0 / s0) : 0.0f;
      a.rcut[pk] = (float)rc;
      a.rcut2[pk] = (float)(rc * rc);
    }
  }
  HIP_TRY(dev_malloc(e, &e->d_ell, sizeof(swarm::EllArgs)));
  HIP_TRY(hipMemcpyAsync(e->d_ell, &a, sizeof(a), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));  // (a is a local)
  e->has_ell = true;
  e->ell_gb = gb;
  e->plan.lxg = lx;
  e->plan.lyg = ly;
  no_cluster_windows(e);
  return SWARM_OK;
}

int swarm_rod_reward(swarm_engine_t* e, const int32_t* agent_idx, int32_t n_agents,
                     uint32_t* hist_ang, double* ring, int32_t* count, int32_t history,
                     double scale, int32_t partition, float* out) {
  if (!e || !agent_idx || !hist_ang || !ring || !count || !out)
    return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  if (!e->has_rod) return fail(SWARM_ESTATE, "the engine has no rod");
  if (n_agents < 1 || history < 1) return fail(SWARM_EINVAL, "n_agents and history must be >= 1");
  hipLaunchKernelGGL(swarm::k_rod_reward, dim3(e->n_envs), dim3(256), 0, e->stream, e->st, e->rod,
                     e->d_box, agent_idx, n_agents, hist_ang, ring, count, history, scale,
                     partition, out);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}

}  // extern "C"

// ---- the Langevin thermostat and the flow field (swarm_langevin.cuh)

namespace {

// The constants of k_langevin_run from the params and the flow's friction, in
// fp64 and rounded once; the flow's records stay as they are.  Refuses what
// the explicit friction cannot integrate: dt (gamma_t + gamma_flow) / m >= 2
// or dt gamma_r / I >= 2.
int langevin_derive(const swarm_params_t& p, double gamma_flow, swarm::LangevinArgs* a) {
  const double kT = p.kT, dt = p.time_step;
  for (int s = 0; s < p.n_species; ++s) {
    const double m = p.mass[s], in = p.rinertia[s];
    if (!(m > 0.0) || !(in > 0.0) || !std::isfinite(m) || !std::isfinite(in))
      return fail(SWARM_EINVAL, "the Langevin thermostat needs a positive mass and rinertia");
    const double gt = p.gamma_t[s] + gamma_flow, gr = p.gamma_r[s];
    const double at = dt * gt / m, ar = dt * gr / in;
    if (!(at < 2.0))
      return fail(SWARM_EINVAL, "unstable Langevin step: dt (gamma_t + gamma_flow) / mass = " +
                                    std::to_string(at) + " for species " + std::to_string(s) +
                                    ", it must be below 2");
    if (!(ar < 2.0))
      return fail(SWARM_EINVAL, "unstable Langevin step: dt gamma_r / rinertia = " +
                                    std::to_string(ar) + " for species " + std::to_string(s) +
                                    ", it must be below 2");
    a->dt_m[s] = (float)(dt / m);
    a->dt_i[s] = (float)(dt / in);
    a->gam[s] = (float)gt;
    a->gam_r[s] = (float)gr;
    a->sig_t[s] = (float)std::sqrt(24.0 * kT * p.gamma_t[s] / dt);
    a->sig_r[s] = (float)std::sqrt(24.0 * kT * gr / dt);
  }
  for (int ax = 0; ax < 2; ++ax) a->dt_sx[ax] = (float)(dt * kTwo32 / p.box[ax]);
  a->dt = (float)dt;
  a->gflow = (float)gamma_flow;
  return SWARM_OK;
}

int langevin_upload(swarm_engine* e) {
  HIP_TRY(hipMemcpyAsync(e->d_lv, &e->lv, sizeof(swarm::LangevinArgs), hipMemcpyHostToDevice,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

}  // namespace

extern "C" {

int swarm_engine_set_langevin(swarm_engine_t* e) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (e->stepped)
    return fail(SWARM_ESTATE,
                "the thermostat must be set before the first integrate or overlap removal");
  if (e->has_lv) return fail(SWARM_EINVAL, "the engine already runs the Langevin thermostat");
  const swarm_params_t& p = e->params;
  if (p.n_dims != 2) return fail(SWARM_EINVAL, "the Langevin thermostat is 2-D only");
  if (!p.periodic) return fail(SWARM_EINVAL, "the Langevin thermostat needs a periodic box");
  if (e->has_rod) return fail(SWARM_EINVAL, "the Langevin thermostat with a rod is not supported");
  if (e->has_ell)
    return fail(SWARM_EINVAL, "the Langevin thermostat with ellipsoids is not supported");
  const size_t fixed = sizeof(swarm::PairTables) + 256;  // (the helpers' own 256 bytes)
  auto fits = [&](int n, int gx, int gy) {
    return swarm::env_lds_words(n, 1 << (gx + gy), false, swarm::langevin_tail_words(n)) * 4 +
               fixed <= kMaxLds;
  };
  if (!fits(e->n, e->plan.lxg, e->plan.lyg)) {
    // 44 bytes of state per particle beside the cell counts and the pair
    // tables: the most this box admits
    int limit = e->n, gx = e->plan.lxg, gy = e->plan.lyg;
    while (limit > 1 && !fits(limit, gx, gy)) {
      --limit;
      cell_grid(p, limit, swarm::max_cutoff(p), &gx, &gy);
    }
    return fail(SWARM_ECAPACITY, "an engine under the Langevin thermostat holds at most " +
                                     std::to_string(limit) +
                                     " particles per env in this box (the 160 KB of LDS of one"
                                     " workgroup)");
  }
  swarm::LangevinArgs a{};
  if (const int rc = langevin_derive(p, 0.0, &a)) return rc;
  HIP_TRY(dev_malloc(e, &e->d_lv, sizeof(swarm::LangevinArgs)));
  e->lv = a;
  e->gamma_flow = 0.0;
  if (const int rc = langevin_upload(e)) return rc;
  // the velocities are integrator state from here on: they start at rest
  const size_t M = (size_t)e->st.m;
  HIP_TRY(hipMemsetAsync(e->st.vel, 0, 3 * M * sizeof(float), e->stream));
  HIP_TRY(hipMemsetAsync(e->st.omega, 0, M * sizeof(float), e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->has_lv = true;
  no_cluster_windows(e);
  return SWARM_OK;
}

int swarm_engine_set_flow_field(swarm_engine_t* e, const float* u, int32_t nx, int32_t ny,
                                int32_t nz, const double* spacing, double gamma) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  if (!e->has_lv)
    return fail(SWARM_EINVAL,
                "a flow field needs the Langevin thermostat (swarm_engine_set_langevin)");
  if (!u) {  // remove the field (the device copy is kept for a later one)
    swarm::LangevinArgs a = e->lv;
    if (const int rc = langevin_derive(e->params, 0.0, &a)) return rc;
    a.flow = nullptr;
    a.fn[0] = a.fn[1] = 0;
    e->lv = a;
    e->gamma_flow = 0.0;
    return langevin_upload(e);
  }
  if (!spacing) return fail(SWARM_EINVAL, "null spacing");
  const int32_t n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a)
    if (n[a] < 1) return fail(SWARM_EINVAL, "grid counts must be positive");
  if (nz != 1) return fail(SWARM_EINVAL, "a 2-D engine takes a flow field with nz = 1");
  const uint64_t count = (uint64_t)nx * (uint64_t)ny;
  const uint64_t words = 8 * count;  // one record of four corners x two components per cell
  if (words > 0x7fffffffull) return fail(SWARM_EINVAL, "flow grid too large (32-bit indexing)");
  for (int a = 0; a < 3; ++a) {
    const double h = spacing[a], L = e->params.box[a];
    if (!std::isfinite(h) || !(h > 0.0)) return fail(SWARM_EINVAL, "grid spacing must be positive");
    if (!(std::fabs(n[a] * h - L) <= 1e-9 * L))
      return fail(SWARM_EINVAL, "the flow grid must tile the box");
  }
  if (!std::isfinite(gamma) || !(gamma >= 0.0))
    return fail(SWARM_EINVAL, "the flow's friction must be finite and not negative");
  for (uint64_t k = 0; k < 3 * count; ++k)
    if (!std::isfinite(u[k])) return fail(SWARM_EINVAL, "non-finite flow value");
  swarm::LangevinArgs a = e->lv;
  if (const int rc = langevin_derive(e->params, gamma, &a)) return rc;
  // u[i][j][0][c], c = 0, 1 (the z component is unused in 2-D)
  std::vector<float> rec((size_t)words);
  for (int32_t i = 0; i < nx; ++i) {
    const size_t r0 = (size_t)i * ny, r1 = (size_t)((i + 1) % nx) * ny;
    for (int32_t j = 0; j < ny; ++j) {
      const size_t j1 = (size_t)((j + 1) % ny);
      float* o = &rec[8 * (r0 + j)];
      for (int c = 0; c < 2; ++c) {
        o[4 * c + 0] = u[3 * (r0 + j) + c];
        o[4 * c + 1] = u[3 * (r1 + j) + c];
        o[4 * c + 2] = u[3 * (r0 + j1) + c];
        o[4 * c + 3] = u[3 * (r1 + j1) + c];
      }
    }
  }
  if (words > e->flow_cap) {
    // the new copy first: a failed allocation leaves the old field in place
    float* v = nullptr;
    HIP_TRY(dev_malloc(e, &v, words * sizeof(float)));
    if (e->d_flow) {
      // no kernel may find the old copy once it is freed: the device's
      // descriptor is cleared first, and the stream drained of its readers
      e->lv.flow = nullptr;
      int rc = langevin_upload(e);
      if (rc == SWARM_OK && dev_free(e, &e->d_flow) != hipSuccess)
        rc = fail(SWARM_EDEVICE, "flow field: hipFree failed");
      if (rc) {
        (void)dev_free(e, &v);
        if (!e->d_flow) e->flow_cap = 0;
        return rc;
      }
    }
    e->d_flow = v;
    e->flow_cap = (size_t)words;
  }
  HIP_TRY(hipMemcpyAsync(e->d_flow, rec.data(), words * sizeof(float), hipMemcpyHostToDevice,
                         e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));  // (rec is a local)
  a.flow = e->d_flow;
  a.fn[0] = nx;
  a.fn[1] = ny;
  e->lv = a;
  e->gamma_flow = gamma;
  return langevin_upload(e);
}

int swarm_engine_upload_velocities(swarm_engine_t* e, const float* vel, const float* omega) {
  if (!e || !vel || !omega) return fail(SWARM_EINVAL, "null argument");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  HIP_TRY(hipMemcpyAsync(e->st.vel, vel, 3 * M * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->st.omega, omega, M * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

int swarm_engine_download_velocities(swarm_engine_t* e, float* vel, float* omega) {
  if (!e) return fail(SWARM_EINVAL, "null engine");
  if (const int frc = flush_check(e)) return frc;
  const size_t M = (size_t)e->st.m;
  if (vel)
    HIP_TRY(hipMemcpyAsync(vel, e->st.vel, 3 * M * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (omega)
    HIP_TRY(hipMemcpyAsync(omega, e->st.omega, M * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SWARM_OK;
}

}  // extern "C"

// the policy samplers and the PPO epochs (swarm_sample_actions ..
// swarm_ppo_deep_ensemble_epoch_grad)
#include "swarm_learn_host.cuh"

int swarm_engine_defer_build(swarm_engine_t* e, int32_t* deferred) {
  if (!e || !deferred) return fail(SWARM_EINVAL, "null argument");
  *deferred = 0;
  // the three-launch 2-D cluster build of a latency-bound engine only (the
  // stages the fused observable / policy launches know how to carry)
  const swarm::EnginePlan& pl = e->plan;
  const bool ok = pl.cluster_path && !pl.nlist_path && !pl.env_build && !pl.big_build &&
                  e->params.n_dims == 2 && pl.wide_run;
  if (!ok) return SWARM_OK;
  e->prebuilt = false;
  e->ride_stage = 1;
  e->vgrid_ready = false;
  *deferred = 1;
  return SWARM_OK;
}

int swarm_neighbor_reduce(const double* pos, const double* dir, const double* vel,
                          const int32_t* types, int32_t n_envs, int32_t n,
                          const int32_t* agent_idx, int32_t n_agents, uint32_t cand_type_mask,
                          double vision_range, double half_angle, double* out, void* stream) {
  if (!pos || !dir || !types || !agent_idx || !out) return fail(SWARM_EINVAL, "null argument");
  if (n_envs < 1 || n < 0 || n_agents < 0) return fail(SWARM_EINVAL, "bad sizes");
  if (n_agents == 0) return SWARM_OK;
  const dim3 grid((unsigned)((n_agents + 255) / 256), (unsigned)n_envs);
  hipLaunchKernelGGL(k_neighbor_reduce, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     pos, dir, vel, types, n, agent_idx, n_agents, cand_type_mask, vision_range,
                     half_angle, out);
  HIP_TRY(hipGetLastError());
  return SWARM_OK;
}
