// Stand-alone check of swarmrl_amd/csrc/swarm_pack.h (host compiler only,
// tests/test_pack_cpu.py): the packing contract between the cluster builds
// and the run kernels.  The builds' 64-lane layout step is restated here as a
// serial prefix sum over the header's per-class quantities; every cluster is
// then placed with pack_base and the placement checked: one wave per
// cluster, no shared slot, no empty wave, the slot bound of slots_per_env,
// the singletons in the free tail lanes first.  The packed words round-trip
// over the full range of each field.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "swarm_pack.h"

using namespace swarm;

static int failures = 0;
static const char* label = "";

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      if (failures < 40) std::printf("pack: line %d [%s]: %s\n", __LINE__, label, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

struct Cluster {
  int s, pairs;
};

struct Layout {
  int32_t tab[3 * kPackTableWords];
  int waves, nfree, waves2;  // waves2: waves of the classes >= 2
};

// The layout step of the builds (pack_layout_wave: lane w - 1 works on class
// w, two wave scans), serially.
static Layout layout(const int cnt[65], bool fill) {
  Layout l = {};
  int32_t* c = l.tab;
  int32_t* wave = l.tab + kPackTableWords;
  int32_t* free_ = l.tab + 2 * kPackTableWords;
  int nw[65], fsum = 0;
  for (int w = 1; w <= 64; ++w) {
    c[w] = cnt[w];
    const int per = pack_per_wave(w);
    nw[w] = pack_waves(cnt[w], per);
    free_[w] = fsum;
    fsum += pack_free_lanes(w, cnt[w], per, nw[w]);
  }
  l.nfree = fill ? fsum : 0;
  free_[65] = l.nfree;
  nw[1] = pack_singleton_waves(cnt[1], l.nfree);
  int wsum = 0;
  for (int w = 1; w <= 64; ++w) {
    wave[w] = wsum;
    wsum += nw[w];
  }
  l.waves = wsum;
  l.waves2 = wsum - nw[1];
  return l;
}

static void check_placement(const std::vector<Cluster>& cl, bool one_pass, bool fill) {
  int cnt[65] = {0};
  int n = 0;
  std::vector<int> cls(cl.size()), rank(cl.size());
  for (size_t k = 0; k < cl.size(); ++k) {
    const int s = cl[k].s, w = pack_class(s, cl[k].pairs, one_pass);
    CHECK(s >= 1 && s <= 64 && w >= s && w <= 64);
    CHECK(one_pass ? w <= 2 * s : w == s);
    cls[k] = w;
    rank[k] = cnt[w]++;
    n += s;
  }
  const Layout l = layout(cnt, fill);
  const PackTables t = pack_tables(l.tab);
  CHECK(t.cnt == l.tab && t.wave == l.tab + 68 && t.free == l.tab + 136);
  if (!fill) CHECK(l.nfree == 0);
  CHECK(64 * l.waves <= slots_per_env(n, one_pass));
  std::vector<int> owner(64 * (size_t)l.waves, -1);
  std::vector<int> in_wave(l.waves, 0);
  for (size_t k = 0; k < cl.size(); ++k) {
    const int w = cls[k], cb = pack_base(w, rank[k], t, l.nfree);
    CHECK(cb >= 0 && cb + w <= 64 * l.waves);
    CHECK(cb % 64 + w <= 64);
    if (cb < 0 || cb + w > 64 * l.waves) continue;
    CHECK(slot_wave(cb) == slot_wave(cb + w - 1) && slot_lane(cb) == cb % 64);
    ++in_wave[cb / 64];
    for (int m = 0; m < w; ++m) {
      CHECK(owner[cb + m] < 0);
      owner[cb + m] = (int)k;
    }
  }
  for (int w = 0; w < l.waves; ++w) CHECK(in_wave[w] > 0);
  if (fill && cnt[1] >= l.nfree) {
    // every lane of the waves of the classes >= 2 is taken (they follow the
    // singletons' own waves), and the rest of the singletons fill waves of 64
    const int own = l.waves - l.waves2;
    CHECK(own == (cnt[1] - l.nfree + 63) / 64);
    CHECK(t.wave[1] == 0);
    for (int k = 64 * own; k < 64 * l.waves; ++k) CHECK(owner[k] >= 0);
  }
  for (int r = 0; r < l.nfree; ++r) {
    int v = 2;  // linear search: the last class >= 2 whose range starts at or before r
    for (int u = 2; u <= 64; ++u)
      if (t.free[u] <= r) v = u;
    CHECK(free_class(t.free, r) == v);
  }
}

static void check_all(const std::vector<Cluster>& cl, const char* what) {
  label = what;
  for (int one_pass = 0; one_pass < 2; ++one_pass)
    for (int fill = 0; fill < 2; ++fill) check_placement(cl, one_pass != 0, fill != 0);
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

// A cluster multiset of n particles: sizes from a distribution with mean
// about `mean` (capped at 64 and at what is left), pairs between a tree's
// s - 1 and 3 s (a dense cluster), so that one-pass classes run up to 2 s.
static std::vector<Cluster> draw(int n, int mean) {
  std::vector<Cluster> cl;
  while (n > 0) {
    int s = 1;
    while (s < 64 && s < n && (int)(rnd() % (uint32_t)mean) != 0) ++s;
    cl.push_back({s, s - 1 + (int)(rnd() % (uint32_t)(2 * s + 2))});
    n -= s;
  }
  return cl;
}

static std::vector<Cluster> uniform(int count, int s, int pairs) {
  return std::vector<Cluster>((size_t)count, Cluster{s, pairs});
}

static void check_words() {
  label = "words";
  for (uint32_t spp = 0; spp < 256; ++spp)
    for (uint32_t a = 0; a < 64; ++a)
      for (uint32_t b = 0; b < 64; ++b) {
        const uint32_t w = wave_pair(a, b, spp);
        CHECK(wave_pair_a(w) == (int)a && wave_pair_b(w) == (int)b && wave_pair_spp(w) == (int)spp);
        CHECK(w != kPairEmpty && (w & kWavePairLanes) == wave_pair_lanes(a, b));
      }
  const uint32_t spps[] = {0, 1, 127, 254, 255};
  for (uint32_t spp : spps)
    for (uint32_t a = 0; a < (uint32_t)kBigMax; ++a)
      for (uint32_t b = 0; b < (uint32_t)kBigMax; ++b) {
        const uint32_t w = big_pair(a, b, spp);
        CHECK(big_pair_a(w) == (int)a && big_pair_b(w) == (int)b && big_pair_spp(w) == (int)spp);
        CHECK((w & kBigPairMembers) == big_pair_members(a, b));
      }
  for (uint32_t spp = 0; spp < 256; ++spp) {
    const uint32_t w = big_pair(1023, 1023, spp), w0 = big_pair(0, 0, spp);
    CHECK(big_pair_spp(w) == (int)spp && big_pair_a(w) == 1023 && big_pair_b(w) == 1023);
    CHECK(big_pair_spp(w0) == (int)spp && big_pair_a(w0) == 0 && big_pair_b(w0) == 0);
  }
  // the class word: every class, ranks up to the largest root index
  for (int w = 1; w <= 64; ++w)
    for (int r = 0; r < 65536; r += (r < 300 || r > 65200 ? 1 : 257)) {
      const int32_t b = class_word(r, w);
      CHECK(class_word_w(b) == w && class_word_rank(b) == r);
      CHECK(b >= 0 && b != kBigMark && !mwb_is_big(b));
    }
  for (int first = 0; first < 65536; ++first) {
    const int32_t b = mwb_big_word(first);
    CHECK(mwb_is_big(b) && mwb_big_first(b) == first);
  }
  for (int m = 0; m < kBigMax; ++m) CHECK(big_slot(m) < 0 && big_slot(big_slot(m)) == m);
  // the division wrapper over what the packing divides
  for (int d = 1; d <= 64; ++d)
    for (int n = 0; n < 70000; n += (n < 200 ? 1 : 97)) CHECK(pack_div(n, d) == n / d);
}

int main() {
  const int sizes[] = {1, 2, 63, 64, 65, 127, 200, 1000, 4096};
  const int means[] = {1, 2, 3, 6, 20, 200};
  for (int n : sizes)
    for (int mean : means)
      for (int rep = 0; rep < 12; ++rep) check_all(draw(n, mean), "random");

  check_all(uniform(4096, 1, 0), "all singletons");
  check_all(uniform(2048, 2, 1), "all dimers");
  check_all(uniform(2048, 2, 4), "all dimers, four lanes each one-pass");
  check_all(uniform(100, 33, 32), "all of class 33");
  check_all(uniform(100, 17, 33), "all of class 33 one-pass");
  check_all(uniform(64, 64, 63), "all of class 64");
  check_all(uniform(64, 32, 64), "all of class 64 one-pass");
  for (int s = 1; s <= 64; ++s) check_all(uniform(1, s, 3 * s), "one cluster");
  {  // 10 clusters of 33: 310 free lanes; fewer, as many, and more singletons
    const int singles[] = {0, 1, 309, 310, 311, 374, 375, 1000};
    for (int k : singles) {
      std::vector<Cluster> cl = uniform(10, 33, 32);
      for (int q = 0; q < k; ++q) cl.push_back({1, 0});
      check_all(cl, "singletons against free lanes");
    }
  }
  {  // free lanes in several classes, the last wave of a class part full
    std::vector<Cluster> cl = uniform(7, 5, 4);
    for (int q = 0; q < 3; ++q) cl.push_back({60, 59});
    for (int q = 0; q < 5; ++q) cl.push_back({21, 20});
    for (int q = 0; q < 90; ++q) cl.push_back({1, 0});
    check_all(cl, "mixed classes");
  }
  check_words();

  if (failures) {
    std::printf("pack: %d failures\n", failures);
    return 1;
  }
  std::printf("pack: ok\n");
  return 0;
}
