// swarm_select.h -- run-time values to template arguments, in plain C++17
// (no HIP types: tests/test_select_cpu.py builds it into a host-only program).
//
// A launch site with template flags passes a generic lambda; the selector
// calls it once with the flags as std::integral_constant values, in the
// order the site wrote them.  The ladders of the host launch layers
// (swarm_engine_host.cuh, swarm_learn_host.cuh) are built from these, so a
// kernel's variant is chosen by one call that names every flag once
// ("Host launch layer").
#pragma once

#include <type_traits>
#include <utility>

namespace swarm_select {

template <int V>
using Int = std::integral_constant<int, V>;

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): the flags reach
// f as the same values in the same positions.  Returns what f returns.
template <class F>
decltype(auto) bools(F&& f) {
  return std::forward<F>(f)();
}
template <class F, class... Rest>
decltype(auto) bools(F&& f, bool b0, Rest... rest) {
  auto bind = [&](auto c0) -> decltype(auto) {
    return bools([&](auto... cs) -> decltype(auto) { return f(c0, cs...); }, rest...);
  };
  return b0 ? bind(std::true_type{}) : bind(std::false_type{});
}

// f over every one of the 2^K flag combinations, the first flag changing
// fastest, false first (the dynamic-LDS opt-in walks a kernel's variants with
// it: every value of the K flags it names; a new template flag still has to
// be added to the walk, as to the launch site).
template <int K, class F, class... Cs>
auto each_bools(F&& f, Cs... cs) {
  if constexpr (K == 0) {
    f(cs...);
  } else {
    each_bools<K - 1>(f, std::false_type{}, cs...);
    each_bools<K - 1>(f, std::true_type{}, cs...);
  }
}

// Cone bins per lane: the narrowest of 4 / 8 / 16 / 32 that holds nb
// (n_cones * n_types; the callers bound it by 32).
template <class F>
decltype(auto) bins(int nb, F&& f) {
  if (nb <= 4) return f(Int<4>{});
  if (nb <= 8) return f(Int<8>{});
  if (nb <= 16) return f(Int<16>{});
  return f(Int<32>{});
}

// Colloids per thread of the one-workgroup sorts (k_build_sort<CH> and the
// fused launches carrying it): 4 up to 4096 colloids per env, 16 above.
constexpr int kSortSmallMax = 4096;
template <class F>
decltype(auto) sort_chunk(int n, F&& f) {
  return n > kSortSmallMax ? f(Int<16>{}) : f(Int<4>{});
}
template <class F>
auto each_sort_chunk(F&& f) {
  f(Int<4>{});
  f(Int<16>{});
}

// Lanes per agent of the vision cone: kVisionGWide or 16.
constexpr int kVisionGWide = 4;
template <class F>
decltype(auto) cone_lanes(int g, F&& f) {
  return g == kVisionGWide ? f(Int<kVisionGWide>{}) : f(Int<16>{});
}

}  // namespace swarm_select
