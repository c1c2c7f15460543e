// swarm_pack.h -- the contract between the cluster build and the run kernels,
// stated once (DESIGN.md "The packing contract"): the lanes a cluster reserves
// (its packing class), the layout of the classes in 64-lane waves, a cluster's
// first slot, and the packed words the builds write and the run and check
// kernels read.  Results do not depend on the packing (fixed-point force
// sums); the run kernels trust it unchecked: every cluster lies in the lanes
// of one wave.  Plain C++17, no HIP types: a host compiler reads it alone
// (tests/csrc/pack_selftest.cpp), the device headers include it.
#pragma once

#include <stdint.h>

#include "swarm_sizes.h"

// (device: inlined at every use, like the hand-written copies these replace)
#ifdef __HIPCC__
#define SWARM_PACK_FN __host__ __device__ __forceinline__
#define SWARM_PACK_UNROLL _Pragma("unroll")
#else
#define SWARM_PACK_FN inline
#define SWARM_PACK_UNROLL
#endif

namespace swarm {

constexpr int kWaveLanes = 64;
// Three tables indexed by the class w = 1..64 (word 65 of the third: the
// total): cluster counts, first waves, free-lane bases, back to back in this
// order wherever a build keeps them (LDS, or sc.bmisc at kBmClass).
constexpr int kPackTableWords = 68;

// floor(n / d) for 0 <= n < 2^20 and 1 <= d < 2^20.  Device: a float
// reciprocal estimate (within one of the quotient in that range) and one
// correction, not the compiler's ~40-instruction integer division (the
// packing divides per cluster).  Host: the division itself; they agree on the
// stated range (here n <= 4 N + 64 with N < 2^16 particles, d <= 64).
SWARM_PACK_FN int pack_div(int n, int d) {
#if defined(__HIP_DEVICE_COMPILE__)
  int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
  const int r = n - q * d;
  q += (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
  return q;
#else
  return n / d;
#endif
}
SWARM_PACK_FN int pack_min(int a, int b) { return a < b ? a : b; }
SWARM_PACK_FN int pack_max(int a, int b) { return a > b ? a : b; }

// Lanes reserved for a cluster of s <= 64 particles (its packing class): its
// size, or with one-pass packing max(s, min(pairs, 64, 2 s)), so that the
// clusters of a wave have at most 64 pairs (one pair pass per sub-step)
// unless a cluster is denser than 2 pairs per particle.
SWARM_PACK_FN int pack_class(int s, int pairs, bool one_pass) {
  return one_pass ? pack_max(s, pack_min(pack_min(pairs, kWaveLanes), 2 * s)) : s;
}

// Class w with cnt clusters: clusters per wave, waves, and the tail lanes it
// leaves free in its waves (64 - per w in a full wave, more in its last one).
// The free lanes of the classes >= 2 take the singletons first; only the
// rest of them get waves of their own (the run kernel's cost is per wave).
SWARM_PACK_FN int pack_per_wave(int w) { return pack_div(kWaveLanes, w); }
SWARM_PACK_FN int pack_waves(int cnt, int per) { return pack_div(cnt + per - 1, per); }
SWARM_PACK_FN int pack_free_lanes(int w, int cnt, int per, int nw) {
  return w >= 2 && nw > 0
             ? (nw - 1) * (kWaveLanes - per * w) + (kWaveLanes - (cnt - (nw - 1) * per) * w)
             : 0;
}
SWARM_PACK_FN int pack_singleton_waves(int cnt, int nfree) {  // nfree: free lanes in all
  return (pack_max(cnt - nfree, 0) + 63) / 64;
}

struct PackTables {
  const int32_t *cnt, *wave, *free;  // per class: clusters, first wave, free-lane base
};
SWARM_PACK_FN PackTables pack_tables(const int32_t* t) {
  return {t, t + kPackTableWords, t + 2 * kPackTableWords};
}

// The packing class v whose free-lane range holds singleton rank r < nfree:
// the largest v >= 2 with freebase[v] <= r (its range is non-empty).
// freebase[2..65] is non-decreasing and freebase[65] = nfree > r, so v - 1 =
// #{u in [2, 65]: freebase[u] <= r}: counted in two rounds of eight
// independent reads (every 8th entry, then the eight from the last of
// those <= r) -- two LDS latencies where a binary search waits for six.
SWARM_PACK_FN int free_class(const int32_t* freebase, int r) {
  int k8 = -1;
  SWARM_PACK_UNROLL
  for (int q = 0; q < 8; ++q) k8 += freebase[2 + 8 * q] <= r ? 1 : 0;
  int v = 1 + 8 * k8;
  SWARM_PACK_UNROLL
  for (int q = 0; q < 8; ++q) v += freebase[2 + 8 * k8 + q] <= r ? 1 : 0;
  return v;
}

// First slot of the cluster of class s and class rank r (slot = 64 wave +
// lane; member m of the cluster sits in slot base + m).
SWARM_PACK_FN int pack_base(int s, int r, const PackTables& t, int nfree) {
  if (s == 1 && r < nfree) {
    // a singleton in a free lane: the class v whose range holds r, then
    // wave j of that class and the lane
    const int v = free_class(t.free, r), per = pack_per_wave(v);
    const int nw = pack_waves(t.cnt[v], per);
    const int ffull = kWaveLanes - per * v;
    const int k = r - t.free[v];
    int j, lane;
    if (k < (nw - 1) * ffull) {
      j = pack_div(k, ffull);
      lane = per * v + (k - j * ffull);
    } else {
      j = nw - 1;
      lane = (t.cnt[v] - (nw - 1) * per) * v + (k - (nw - 1) * ffull);
    }
    return (t.wave[v] + j) * 64 + lane;
  }
  if (s == 1) {  // a singleton in a wave of singletons
    const int r2 = r - nfree;
    return (t.wave[1] + r2 / 64) * 64 + r2 % 64;
  }
  const int per = pack_per_wave(s), rq = pack_div(r, per);
  return (t.wave[s] + rq) * 64 + (r - rq * per) * s;
}

// A particle's slot: 64 wave + lane, or for member m of a big cluster (wider
// than a wave, run by k_check's workgroup) -1 - m.
SWARM_PACK_FN int slot_wave(int slot) { return slot >> 6; }
SWARM_PACK_FN int slot_lane(int slot) { return slot & 63; }
SWARM_PACK_FN int big_slot(int m) { return -1 - m; }  // its own inverse

// The wave pair word: lane a | lane b << 6 | species pair << 12.
constexpr int kLaneBits = 6;
constexpr int kSppBits = 8;
constexpr uint32_t kLaneMask = (1u << kLaneBits) - 1;
constexpr uint32_t kSppMask = (1u << kSppBits) - 1;
constexpr uint32_t kWavePairLanes = (1u << 2 * kLaneBits) - 1;  // mask: both lanes of a word
constexpr uint32_t kPairEmpty = 0xffffffffu;  // no pair in this slot of a pass
SWARM_PACK_FN uint32_t wave_pair_lanes(uint32_t la, uint32_t lb) { return la | lb << kLaneBits; }
SWARM_PACK_FN uint32_t wave_pair(uint32_t la, uint32_t lb, uint32_t spp) {
  return la | (lb << kLaneBits) | (spp << 2 * kLaneBits);
}
SWARM_PACK_FN int wave_pair_a(uint32_t w) { return (int)(w & kLaneMask); }
SWARM_PACK_FN int wave_pair_b(uint32_t w) { return (int)((w >> kLaneBits) & kLaneMask); }
SWARM_PACK_FN int wave_pair_spp(uint32_t w) { return (int)((w >> 2 * kLaneBits) & kSppMask); }

// The big-cluster pair word: member a | member b << 10 | species pair << 20.
constexpr int kBigBits = 10;
constexpr uint32_t kBigMask = (1u << kBigBits) - 1;
constexpr uint32_t kBigPairMembers = (1u << 2 * kBigBits) - 1;  // mask: both members
SWARM_PACK_FN uint32_t big_pair_members(uint32_t ma, uint32_t mb) { return ma | mb << kBigBits; }
SWARM_PACK_FN uint32_t big_pair(uint32_t ma, uint32_t mb, uint32_t spp) {
  return ma | (mb << kBigBits) | (spp << 2 * kBigBits);
}
SWARM_PACK_FN int big_pair_a(uint32_t w) { return (int)(w & kBigMask); }
SWARM_PACK_FN int big_pair_b(uint32_t w) { return (int)((w >> kBigBits) & kBigMask); }
SWARM_PACK_FN int big_pair_spp(uint32_t w) { return (int)(w >> 2 * kBigBits); }

// The class word a root keeps between the class count and its base (packed
// and multi-workgroup builds): class rank | w << 24.  A big cluster's root
// holds an escape instead: kBigMark (one-workgroup builds), or kMwbBig | its
// first member in the big list (multi-workgroup build).
constexpr int kClassShift = 24;
constexpr int32_t kClassRankMask = (1 << kClassShift) - 1;
constexpr int kBigMark = -0x40000000;
constexpr uint32_t kMwbBig = 0x80000000u;
SWARM_PACK_FN int32_t class_word(int rank, int w) { return rank | (w << kClassShift); }
SWARM_PACK_FN int class_word_w(int32_t b) { return (b >> kClassShift) & 0x7f; }
SWARM_PACK_FN int class_word_rank(int32_t b) { return b & kClassRankMask; }
SWARM_PACK_FN int32_t mwb_big_word(int first) { return (int32_t)(kMwbBig | (uint32_t)first); }
SWARM_PACK_FN bool mwb_is_big(int32_t b) { return ((uint32_t)b & kMwbBig) != 0; }
SWARM_PACK_FN int mwb_big_first(int32_t b) { return (int)((uint32_t)b & ~kMwbBig); }

static_assert((1 << kLaneBits) == kWaveLanes, "a lane field names every lane of a wave");
static_assert((1 << kBigBits) >= kBigMax, "a member field names every big-cluster member");
static_assert((1 << kSppBits) >= SWARM_MAX_SPECIES * SWARM_MAX_SPECIES, "species-pair field");
// (strictly below 32 bits: a pair word never equals kPairEmpty)
static_assert(2 * kLaneBits + kSppBits < 32 && 2 * kBigBits + kSppBits <= 32, "32-bit words");
static_assert(kPairsPerWave % kWaveLanes == 0, "a wave's list is whole passes of a pair a lane");
// class words are non-negative (classes 1..64 in 7 bits below the sign), the escapes negative
static_assert(kWaveLanes <= 0x7f && (kWaveLanes << kClassShift) > 0, "class field");
static_assert(kBigMark < 0 && (int32_t)kMwbBig < 0, "the escapes are no class words");

}  // namespace swarm
