// Stand-alone check of swarmrl_amd/csrc/swarm_plan.h and swarm_sizes.h (host
// compiler only, tests/test_plan_cpu.py).  Results are bit-identical on every
// path of the engine, so no correctness test notices a path threshold that
// slipped; this program prints what swarm::plan_engine decides for a fixed
// grid of engines, both sides of every threshold, one line per row, and the
// test compares the lines with tests/plan_rows_parent.txt: the same fields
// printed by swarm_engine_create itself, on the device, at the commit before
// plan_engine existed.
//
//   plan_selftest          the lines, then the invariants' verdict
//   plan_selftest --rows   the grid's inputs, one row per line (what a driver
//                          needs to create the same engines through the C ABI)
//
// A valid row prints every EnginePlan field, the number of allocations, their
// total bytes and an order-sensitive checksum of their sizes (FNV-1a over the
// byte counts; the Derived block, one struct of the device headers, counts as
// an allocation of no bytes).  A refused row prints its status and message.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "swarm_plan.h"

using swarm::EnginePlan;
using swarm::kMaxLds;

static int failures = 0;
static const char* g_row = "";

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("plan: row %s: line %d: %s\n", g_row, __LINE__, #cond);   \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

// ov: one character per override in PlanOverrides' order (cluster_path,
// local_uf, nlist, noise_table, env_build, wide_run, rot_helper, defer_check),
// '-' for unset.  Species 0 has radius r0, every other species r1.
struct Row {
  const char* name;
  int dims, periodic;
  double box[3];
  int n_species;
  double r0, r1, kT, dt, gamma_t, gamma_r;
  int n_envs, n;
  const char* ov;
};

// the benchmark's box: area fraction 0.1 of unit-radius colloids in the
// placement disc (bench.py:build_workload)
static double bench_box(int n) { return 2.0 * std::sqrt(n * 1.0 / 0.1); }

static Row bench(const char* name, int n_envs, int n, const char* ov = "--------") {
  const double L = bench_box(n);
  return {name, 2, 1, {L, L, L}, 1, 1.0, 1.0, 1.0, 1e-3, 1.0, 1.0, n_envs, n, ov};
}
static Row boxed(const char* name, int dims, int periodic, double L, int n_envs, int n,
                 const char* ov = "--------") {
  return {name, dims, periodic, {L, L, L}, 1, 1.0, 1.0, 1.0, 1e-3, 1.0, 1.0, n_envs, n, ov};
}

// N thresholds that follow from the LDS formulas (checked in main): the
// largest N for which build_is_big is false, and the smallest and largest
// for which the build sort stages its rows in LDS (sort_stage_k > 0)
constexpr int kLastSmallBuild = 8031;
// the largest N whose union-find forest fits the build's LDS (cluster_path)
constexpr int kLastClusterBuild = 38264;
constexpr int kFirstStagedSort = 4, kLastStagedSort = 16384;

static const Row* grid(int* count) {
  static Row rows[128];
  int k = 0;
  auto add = [&](Row r) { rows[k++] = r; };
  // bench.py's shapes
  add(bench("head_1x4096", 1, 4096));
  add(bench("batched_64x4096", 64, 4096));
  add(bench("c3train_1x4096", 1, 4096));
  add(bench("c4_8x1024", 8, 1024));
  // M = E N: latency-bound, noise blocks, the run_wpb ladder beside 64 noise
  // blocks (est = M / 46 + 1 against 224) and beside none (est / 2 against 256;
  // est against 224 without the wide run)
  add(bench("M_32768", 32, 1024));
  add(bench("M_32769", 33, 993));
  add(bench("M_16384", 16, 1024));
  add(bench("M_16385", 5, 3277));
  add(bench("M_7359", 3, 2453));
  add(bench("M_7360", 2, 3680));
  add(bench("M_23597", 7, 3371));
  add(bench("M_23598", 6, 3933));
  add(bench("M_10303_narrow", 1, 10303, "-----0--"));
  add(bench("M_10304_narrow", 1, 10304, "-----0--"));
  // N: chip sort, local_uf and the sort chunk; the cluster path's last N.
  // (N < 65536 in cluster_path never decides: the forest's LDS ends the path
  // at kLastClusterBuild, and 65536 colloids are refused for the check's LDS.
  // The N_cluster_build pair tests the limit that acts, N_65535 | N_65536
  // only record that nothing else changes there.)
  add(bench("N_4096", 1, 4096));
  add(bench("N_4097", 1, 4097));
  add(bench("N_65535", 1, 65535));
  add(bench("N_65536", 1, 65536));
  add(bench("N_cluster_build_last", 1, kLastClusterBuild));
  add(bench("N_cluster_build_next", 1, kLastClusterBuild + 1));
  add(bench("N_small_build_last", 1, kLastSmallBuild));
  add(bench("N_small_build_next", 1, kLastSmallBuild + 1));
  add(bench("N_staged_sort_before", 1, kFirstStagedSort - 1));
  add(bench("N_staged_sort_first", 1, kFirstStagedSort));
  add(bench("N_staged_sort_last", 1, kLastStagedSort));
  add(bench("N_staged_sort_next", 1, kLastStagedSort + 1));
  // build grids of 2 | 4 cells a side (cluster_path) and 4 | 8 (l1_pairs: at
  // least 5): cell side >= 2 r + skin = 4
  add(boxed("grid_2", 2, 1, 15.9, 1, 16));
  add(boxed("grid_4", 2, 1, 16.0, 1, 16));
  add(boxed("grid_4_wide", 2, 1, 31.9, 1, 32));
  add(boxed("grid_8", 2, 1, 32.0, 1, 32));
  // mean degree n / L^2 pi 4^2 around 3 in 2-D, n / L^3 (4 / 3) pi 4^3 around 2 in 3-D
  add(boxed("deg2d_below_3", 2, 1, 131.0, 1, 1024));
  add(boxed("deg2d_above_3", 2, 1, 130.9, 1, 1024));
  add(boxed("deg3d_below_2", 3, 1, 51.6, 1, 1024));
  add(boxed("deg3d_above_2", 3, 1, 51.5, 1, 1024));
  // the other geometries
  add(boxed("dims3_periodic", 3, 1, 120.0, 2, 4096));
  add(boxed("dims3_open", 3, 0, 120.0, 2, 4096));
  add(boxed("dims3_open_dense", 3, 0, 51.5, 1, 1024));
  add(boxed("dims2_open", 2, 0, bench_box(1024), 4, 1024));
  add(boxed("dims2_open_many", 2, 0, bench_box(1024), 64, 1024));
  {
    Row r = bench("two_species", 1, 1024);
    r.n_species = 2, r.r0 = 1.0, r.r1 = 1.5;
    add(r);
    r = bench("two_species_many", 64, 1024);
    r.n_species = 2, r.r0 = 0.5, r.r1 = 1.5;
    add(r);
    r = bench("athermal", 1, 1024);  // kT = 0: no noise, no table
    r.kT = 0.0;
    add(r);
  }
  // a grid whose cell counts do not fit the check's workgroup
  {
    Row r = bench("lds_refused", 1, 100000);
    r.r0 = r.r1 = 0.01;
    add(r);
  }
  // one row per refusal of the parameter checks, in their order
  {
    Row r = bench("bad_dims", 1, 64);
    r.dims = 4;
    add(r);
    add(bench("bad_envs", 0, 64));
    add(bench("bad_n", 1, 0));
    r = bench("bad_species_0", 1, 64);
    r.n_species = 0;
    add(r);
    r = bench("bad_species_17", 1, 64);
    r.n_species = 17;
    add(r);
    r = bench("bad_box_0", 1, 64);
    r.box[1] = 0.0;
    add(r);
    r = bench("bad_box_tiny", 1, 64);
    r.box[0] = 1e-6;
    add(r);
    r = bench("bad_dt", 1, 64);
    r.dt = 0.0;
    add(r);
    r = bench("bad_gamma", 1, 64);
    r.gamma_r = 0.0;
    add(r);
    r = bench("bad_gamma_t", 1, 64);
    r.gamma_t = -1.0;
    add(r);
    r = bench("bad_radius_negative", 1, 64);
    r.r0 = -1.0;
    add(r);
    r = bench("bad_radius", 1, 64);
    r.r0 = r.r1 = 0x1p40;
    add(r);
    add(bench("bad_n_2_20", 1, (1 << 20) + 1));
  }
  // every override at unset, 0, 1 and x, on rows whose outcome it can change
  static char names[64][40];
  static char ovs[64][9];
  int kn = 0;
  auto sweep = [&](const char* what, int pos, Row base) {
    for (const char c : {'-', '0', '1', 'x'}) {
      std::snprintf(names[kn], sizeof(names[kn]), "%s_%c", what, c);
      std::strcpy(ovs[kn], "--------");
      ovs[kn][pos] = c;
      base.name = names[kn];
      base.ov = ovs[kn];
      add(base);
      ++kn;
    }
  };
  sweep("ov_cluster_head", 0, bench("", 1, 4096));
  sweep("ov_local_uf_4096", 1, bench("", 1, 4096));
  sweep("ov_local_uf_4097", 1, bench("", 1, 4097));
  sweep("ov_local_uf_big", 1, bench("", 1, kLastSmallBuild + 1));  // k_mwb_* or not
  sweep("ov_nlist_sparse", 2, bench("", 1, 1024));
  sweep("ov_nlist_dense", 2, boxed("", 2, 1, 130.9, 1, 1024));
  sweep("ov_nlist_open", 2, boxed("", 2, 0, 130.9, 1, 1024));  // periodic-only: never
  sweep("ov_noise_head", 3, bench("", 1, 4096));
  sweep("ov_noise_many", 3, bench("", 64, 1024));
  sweep("ov_env_build_head", 4, bench("", 1, 4096));
  sweep("ov_env_build_many", 4, bench("", 64, 1024));
  sweep("ov_wide_head", 5, bench("", 1, 4096));
  sweep("ov_rot_head", 6, bench("", 1, 4096));
  sweep("ov_defer_head", 7, bench("", 1, 4096));
  *count = k;
  return rows;
}

static swarm_params_t params_of(const Row& r) {
  swarm_params_t p;
  std::memset(&p, 0, sizeof(p));
  p.n_dims = r.dims;
  p.periodic = r.periodic;
  for (int a = 0; a < 3; ++a) p.box[a] = r.box[a];
  p.time_step = r.dt;
  p.kT = r.kT;
  p.wca_epsilon = 1.0;
  p.seed = 1;
  p.n_species = r.n_species;
  p.reuse_forces = 1;
  for (int s = 0; s < SWARM_MAX_SPECIES; ++s) {
    p.radius[s] = s == 0 ? r.r0 : r.r1;
    p.gamma_t[s] = r.gamma_t;
    p.gamma_r[s] = r.gamma_r;
    p.mass[s] = 1.0;
    p.rinertia[s] = 1.0;
  }
  return p;
}

static swarm::PlanOverrides overrides_of(const Row& r) {
  auto c = [&](int k) { return r.ov[k] == '-' ? (char)0 : r.ov[k]; };
  swarm::PlanOverrides ov;
  ov.cluster_path = c(0), ov.local_uf = c(1), ov.nlist = c(2), ov.noise_table = c(3);
  ov.env_build = c(4), ov.wide_run = c(5), ov.rot_helper = c(6), ov.defer_check = c(7);
  return ov;
}

struct AllocSum {
  int n = 0;
  unsigned long long bytes = 0, sum = 14695981039346656037ull;
};
static AllocSum alloc_sum(const EnginePlan& pl) {
  AllocSum a;
  for (int k = 0; k < swarm::kNumEngineBufs; ++k) {
    if (pl.count[k] == 0) continue;
    const unsigned long long b = (unsigned long long)pl.count[k] * swarm::kBufElemBytes[k];
    a.n += 1;
    a.bytes += b;
    a.sum = (a.sum ^ b) * 1099511628211ull;
  }
  return a;
}

// every EnginePlan field and the allocations' summary (a static buffer)
static const char* plan_line(const Row& r, const EnginePlan& pl) {
  static char line[1024];
  const AllocSum a = alloc_sum(pl);
  std::snprintf(line, sizeof(line),
              "%s: ok g=%d,%d,%d b=%d,%d,%d lat=%d cluster=%d nlist=%d big=%d chip=%d luf=%d "
              "mwb=%d onep=%d fill=%d noise=%d envb=%d wide=%d rot=%d l1=%d defer=%d cap=%d S=%d "
              "wmax=%d stage=%d nb=%d wpb=%d cd=%.9g allocs=%d bytes=%llu sum=%016llx\n",
              r.name, pl.lxg, pl.lyg, pl.lzg, pl.lxb, pl.lyb, pl.lzb, (int)pl.latency_bound,
              (int)pl.cluster_path, (int)pl.nlist_path, (int)pl.big_build, (int)pl.chip_sort,
              (int)pl.local_uf, (int)pl.mwb, (int)pl.one_pass, (int)pl.fill_singletons,
              (int)pl.noise_table, (int)pl.env_build, (int)pl.wide_run, (int)pl.rot_helper,
              (int)pl.l1_pairs, (int)pl.defer_check, pl.pair_cap, pl.S, pl.wmax, pl.sort_stage_k,
              pl.noise_blocks, pl.run_wpb, (double)(float)pl.cand_disp, a.n, a.bytes, a.sum);
  return line;
}

static void print_plan(const Row& r, const EnginePlan& pl) {
  std::fputs(plan_line(r, pl), stdout);
}

// What holds on every valid row, whatever the table says.
static void check_invariants(const Row& r, const EnginePlan& pl) {
  const bool two_d = r.dims == 2;
  if (pl.nlist_path) CHECK(pl.cluster_path && r.periodic);
  if (pl.l1_pairs) CHECK(pl.wide_run);
  if (pl.wide_run) CHECK(pl.noise_table);
  if (pl.noise_table) CHECK(pl.cluster_path && two_d && !pl.nlist_path);
  CHECK(!(pl.env_build && pl.l1_pairs));
  CHECK(pl.noise_blocks == 0 || pl.noise_blocks == 64);
  CHECK(pl.run_wpb == 1 || pl.run_wpb == 2 || pl.run_wpb == 4);
  if (pl.cluster_path) CHECK(pl.pair_cap >= r.n);
  if (pl.defer_check) CHECK(pl.l1_pairs);
  if (pl.mwb) CHECK(pl.big_build && pl.local_uf && two_d);
  CHECK(pl.wmax == pl.S / 64 && pl.S == swarm::slots_per_env(r.n, pl.one_pass));
  // the LDS of every launch the plan selects (the run kernels' is a constant
  // of swarm_integrator.cuh, not of the plan)
  const size_t st = swarm::kPairTablesBytes;
  if (two_d) {
    CHECK(swarm::global_lds_bytes(pl.lxg, pl.lyg, r.n, r.dims) + st <= kMaxLds);
    CHECK(swarm::check_lds_bytes(pl.lxg, pl.lyg, r.n, r.dims) + st <= kMaxLds);
  } else {
    CHECK((16 + ((size_t)1 << (pl.lxg + pl.lyg + pl.lzg)) + 1) * 4 + st <= kMaxLds);
  }
  if (pl.cluster_path) {
    const size_t ncb = (size_t)1 << (pl.lxb + pl.lyb + pl.lzb);
    if (!two_d) CHECK(swarm::check3_lds_bytes(pl.lxg, pl.lyg, pl.lzg) + st <= kMaxLds);
    if (pl.env_build) {
      CHECK(swarm::build_lds_words(r.n, pl.pair_cap) * 4 <= kMaxLds);
      CHECK(!pl.big_build);
    } else {
      CHECK(swarm::sort_lds_bytes(pl.lxb, pl.lyb, pl.lzb, pl.sort_stage_k) <= kMaxLds);
      if (pl.chip_sort) CHECK((16 + ncb + 1) * 4 <= kMaxLds);  // k_sort_scan
      if (pl.nlist_path || pl.mwb) {
        // (no one-workgroup cluster build)
      } else if (pl.big_build) {
        const bool local = two_d && pl.local_uf;
        const size_t packed = swarm::build_lds_words_packed(r.n) * 4;
        CHECK((!local && packed <= kMaxLds) || swarm::build_lds_words_big(r.n) * 4 <= kMaxLds);
      } else {
        CHECK(swarm::build_lds_words(r.n, pl.pair_cap) * 4 <= kMaxLds);
      }
    }
    if (pl.l1_pairs) CHECK(swarm::l1_role_lds_bytes() <= kMaxLds);
  }
  // buffers that exist on some paths only, and no others
  int n_alloc = 0;
  for (int k = 0; k < swarm::kNumEngineBufs; ++k) n_alloc += pl.count[k] != 0;
  const int optional = 3 * pl.chip_sort + pl.big_build + pl.mwb + pl.noise_table + 3 * pl.l1_pairs;
  CHECK(n_alloc == swarm::kNumEngineBufs - 9 + optional);
  CHECK(alloc_sum(pl).n == n_alloc);
}

static void check_thresholds() {
  g_row = "thresholds";
  CHECK(!swarm::build_is_big(kLastSmallBuild) && swarm::build_is_big(kLastSmallBuild + 1));
  auto staged = [](int n) {
    EnginePlan pl;
    const char* msg = "";
    const swarm_params_t p = params_of(bench("", 1, n));
    return swarm::plan_engine(p, 1, n, {}, swarm::kPairTablesBytes, &pl, &msg) == SWARM_OK &&
           pl.sort_stage_k > 0;
  };
  CHECK(swarm::build_lds_words_big(kLastClusterBuild) * 4 <= kMaxLds &&
        swarm::build_lds_words_big(kLastClusterBuild + 1) * 4 > kMaxLds);
  CHECK(!staged(kFirstStagedSort - 1) && staged(kFirstStagedSort));
  CHECK(staged(kLastStagedSort) && !staged(kLastStagedSort + 1));
  // env_lds_words against the three formulas it replaced, written out: the
  // global path's extra words (kRodTailWords of swarm_rod.cuh is 15), the
  // rod's and the ellipsoids' whole dynamic LDS
  for (const int n : {1, 2, 63, 64, 1024, 1131, 4096})
    for (const int ncell : {1, 4, 64, 4096}) {
      const size_t N = (size_t)n, C = (size_t)ncell;
      CHECK(swarm::env_lds_words(n, ncell, false, 1) - (16 + C + 1) == 8 * N + 2);
      CHECK(swarm::global_lds_extra_words(n, 2, ncell) == 8 * N + 2);
      CHECK(swarm::global_lds_extra_words(n, 3, ncell) == 0);
      CHECK(swarm::env_lds_words(n, ncell, false, 15) == 16 + C + 1 + 8 * N + 2 + 2 + 8 + 4);
      CHECK(swarm::env_lds_words(n, ncell, true, 0) == 16 + C + 1 + 1 + 10 * N);
    }
  // plan_no_cluster_windows clears these six flags and touches nothing else
  {
    EnginePlan pl;
    const char* msg = "";
    const swarm_params_t p = params_of(bench("", 1, 4096));
    CHECK(swarm::plan_engine(p, 1, 4096, {}, swarm::kPairTablesBytes, &pl, &msg) == SWARM_OK);
    CHECK(pl.cluster_path && pl.noise_table && pl.wide_run && pl.defer_check);
    pl.nlist_path = pl.env_build = true;  // (no one plan sets all six)
    EnginePlan want = pl;
    want.cluster_path = want.nlist_path = want.noise_table = false;
    want.wide_run = want.env_build = want.defer_check = false;
    swarm::plan_no_cluster_windows(pl);
    const Row r = bench("no_cluster_windows", 1, 4096);
    char got_line[1024], want_line[1024];
    std::snprintf(got_line, sizeof(got_line), "%s", plan_line(r, pl));
    std::snprintf(want_line, sizeof(want_line), "%s", plan_line(r, want));
    CHECK(std::strcmp(got_line, want_line) == 0);
    CHECK(std::memcmp(pl.count, want.count, sizeof(pl.count)) == 0);
    CHECK(!pl.cluster_path && !pl.nlist_path && !pl.noise_table && !pl.wide_run &&
          !pl.env_build && !pl.defer_check);
  }
  // the four parsing rules, over unset, '0', '1' and anything else
  for (const bool v : {false, true}) {
    CHECK(swarm::ov_clears(0, v) == v && !swarm::ov_clears('0', v) &&
          swarm::ov_clears('1', v) == v && swarm::ov_clears('x', v) == v);
    CHECK(swarm::ov_clears_or_sets(0, v) == v && !swarm::ov_clears_or_sets('0', v) &&
          swarm::ov_clears_or_sets('1', v) && swarm::ov_clears_or_sets('x', v) == v);
    CHECK(swarm::ov_sets_unless_0(0, v) == v && !swarm::ov_sets_unless_0('0', v) &&
          swarm::ov_sets_unless_0('1', v) && swarm::ov_sets_unless_0('x', v));
    CHECK(swarm::ov_only_1_sets(0, v) == v && !swarm::ov_only_1_sets('0', v) &&
          swarm::ov_only_1_sets('1', v) && !swarm::ov_only_1_sets('x', v));
  }
}

int main(int argc, char** argv) {
  int count = 0;
  const Row* rows = grid(&count);
  if (argc > 1 && std::strcmp(argv[1], "--rows") == 0) {
    for (int k = 0; k < count; ++k) {
      const Row& r = rows[k];
      std::printf("%s %d %d %.17g %.17g %.17g %d %.17g %.17g %.17g %.17g %.17g %.17g %d %d %s\n",
                  r.name, r.dims, r.periodic, r.box[0], r.box[1], r.box[2], r.n_species, r.r0,
                  r.r1, r.kT, r.dt, r.gamma_t, r.gamma_r, r.n_envs, r.n, r.ov);
    }
    return 0;
  }
  for (int k = 0; k < count; ++k) {
    const Row& r = rows[k];
    g_row = r.name;
    const swarm_params_t p = params_of(r);
    EnginePlan pl;
    const char* msg = "";
    const int rc = swarm::plan_engine(p, r.n_envs, r.n, overrides_of(r), swarm::kPairTablesBytes,
                                      &pl, &msg);
    if (rc) {
      std::printf("%s: refused %d %s\n", r.name, rc, msg);
      continue;
    }
    print_plan(r, pl);
    check_invariants(r, pl);
  }
  check_thresholds();
  if (failures) return 1;
  std::printf("plan: ok\n");
  return 0;
}
