// Stand-alone check of swarmrl_amd/csrc/swarm_select.h (host compiler only,
// tests/test_select_cpu.py): the selectors hand a launch site the
// compile-time values its run-time flags name, in the order it wrote them.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "swarm_select.h"

namespace sel = swarm_select;

static int failures = 0;

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("select: line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// The flags as the callee sees them: compile-time values (each argument is a
// std::bool_constant, read through ::value), packed with flag i at bit i.
struct Seen {
  int count;
  unsigned bits;
};

struct Pack {
  template <class... Cs>
  Seen operator()(Cs...) const {
    static_assert((std::is_same_v<Cs, std::bool_constant<Cs::value>> && ...),
                  "bools passes std::bool_constant values");
    unsigned bits = 0, i = 0;
    ((bits |= (Cs::value ? 1u : 0u) << i++), ...);
    return {(int)sizeof...(Cs), bits};
  }
};

static bool bit(unsigned m, int i) { return (m >> i) & 1u; }

static void check_bools() {
  for (unsigned m = 0; m < 2; ++m) {
    const Seen s = sel::bools(Pack{}, bit(m, 0));
    CHECK(s.count == 1 && s.bits == m);
  }
  for (unsigned m = 0; m < 4; ++m) {
    const Seen s = sel::bools(Pack{}, bit(m, 0), bit(m, 1));
    CHECK(s.count == 2 && s.bits == m);
  }
  for (unsigned m = 0; m < 8; ++m) {
    const Seen s = sel::bools(Pack{}, bit(m, 0), bit(m, 1), bit(m, 2));
    CHECK(s.count == 3 && s.bits == m);
  }
  for (unsigned m = 0; m < 16; ++m) {
    const Seen s = sel::bools(Pack{}, bit(m, 0), bit(m, 1), bit(m, 2), bit(m, 3));
    CHECK(s.count == 4 && s.bits == m);
  }
  // a callee without a result, and one taking no flag at all
  int calls = 0;
  sel::bools([&](auto a, auto b) { calls += a && !b ? 1 : 100; }, true, false);
  sel::bools([&] { calls += 10; });
  CHECK(calls == 11);
}

template <int K>
static void check_each_bools() {
  std::vector<unsigned> seen;
  sel::each_bools<K>([&](auto... cs) {
    const Seen s = Pack{}(cs...);
    CHECK(s.count == K);
    seen.push_back(s.bits);
  });
  CHECK(seen.size() == (1u << K));
  std::vector<bool> hit(1u << K, false);
  for (unsigned b : seen) {
    CHECK(b < (1u << K) && !hit[b]);
    if (b < (1u << K)) hit[b] = true;
  }
}

static int bins_of(int nb) {
  return sel::bins(nb, [](auto v) { return (int)decltype(v)::value; });
}
static int chunk_of(int n) {
  return sel::sort_chunk(n, [](auto v) { return (int)decltype(v)::value; });
}
static int lanes_of(int g) {
  return sel::cone_lanes(g, [](auto v) { return (int)decltype(v)::value; });
}

int main() {
  check_bools();
  check_each_bools<1>();
  check_each_bools<2>();
  check_each_bools<3>();
  check_each_bools<4>();

  CHECK(bins_of(1) == 4);
  CHECK(bins_of(4) == 4);
  CHECK(bins_of(5) == 8);
  CHECK(bins_of(8) == 8);
  CHECK(bins_of(9) == 16);
  CHECK(bins_of(16) == 16);
  CHECK(bins_of(17) == 32);
  CHECK(bins_of(32) == 32);

  CHECK(chunk_of(1) == 4);
  CHECK(chunk_of(4096) == 4);
  CHECK(chunk_of(4097) == 16);
  CHECK(chunk_of(1 << 20) == 16);
  std::vector<int> chunks;
  sel::each_sort_chunk([&](auto v) { chunks.push_back(decltype(v)::value); });
  CHECK(chunks.size() == 2 && chunks[0] == chunk_of(4096) && chunks[1] == chunk_of(4097));

  CHECK(lanes_of(sel::kVisionGWide) == sel::kVisionGWide);
  CHECK(lanes_of(16) == 16);
  CHECK(sel::kVisionGWide != 16);

  static_assert(std::is_same_v<sel::Int<7>, std::integral_constant<int, 7>>, "Int");
  if (failures) return 1;
  std::printf("select: ok\n");
  return 0;
}
