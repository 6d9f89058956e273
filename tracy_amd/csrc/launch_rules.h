// launch_rules.h -- the arithmetic on a PairDesc / FrontDesc that sizes a launch and says what the kernel timers are credited for it,
// each rule once for both paths: the host-planned drivers (dp_plan.h, capi.hip, pipeline.hip) and the stream-ordered pass
// (stream_plan.h, stream.hip: planning kernels and their host side).  These numbers decide which tier a trace takes (SD_SHAPE, SD_MEM,
// SD_PRELIM_BAND, kStreamNo) and what bench.py prices from the timers; where the two paths differ on purpose the difference is an
// argument.  No containers, no HIP calls: tests/cpp/launch_rules.cpp compares every rule with the formula written out.
#ifndef TRACY_AMD_LAUNCH_RULES_H
#define TRACY_AMD_LAUNCH_RULES_H

#include "band16.h"
#include "dp_lane.h"
#include "front.h"

namespace tracyhip {

struct Credit { uint64_t cells, bytes; };  // of one pair: the cells a kernel evaluates for it, the bytes it moves

// ---- band pairs ----
// list of a strip height (launch order 12, 8, 4); -1: no band kernel of that height
TR_HD int band_bucket(int K) { return K == 12 ? 0 : K == 8 ? 1 : K == 4 ? 2 : -1; }
// bytes of traceback words of a pair (kind 0; the origin form keeps none), rounded to 16
TR_HD uint64_t band_word_bytes(const PairDesc& d, int K, int kind) {
  return kind == 0 ? ((b16_store_words(d.m, d.n, K, band_dmin(d), band_dmax(d)) * b16_word_bytes(K) + 15u) & ~15ull) : 0;
}
// cells: the steps of its strips x the strip height; bytes: its words (kind 0), the substitution tables, the codes, the result
TR_HD Credit band_credit(const PairDesc& d, int K, int kind) {
  const uint64_t wds = b16_words(d.m, d.n, K, band_dmin(d), band_dmax(d));
  return Credit{wds * (uint64_t)K, (kind == 0 ? wds * b16_word_bytes(K) : 0) + 12ull * d.m + d.n + 4};
}

// ---- band launches: the code rows of four pairs + the tables of the strip height in LDS ----
constexpr uint32_t kBandLdsHard = 64u * 1024u;  // what a workgroup can have: run_band16 refuses a launch past it (ERR_RANGE), the stream-ordered pass its batch
constexpr uint32_t kBandLdsPlan = 60u * 1024u;  // R4, a planner's verdict on one pair: 4 KiB earlier, so a trace changes tier before a launch is refused (its tier depends on it)
// code columns staged per pair for a longest reference of n columns
TR_HD uint32_t band_code_cap(uint32_t n) { return (n + 7u) & ~3u; }
TR_HD bool band_lds_fits(uint32_t code_cap, int K, uint32_t limit_bytes) { return 4ull * code_cap + b16_table_bytes(K) <= limit_bytes; }

// ---- tiers of a pruned sweep (front.h): strips of KB rows on c* +- halfw below the kept row ----
// front_place_body: a sub-window is at most m_rest + 2 halfw + 2 columns
TR_HD uint32_t front_code_cap(uint32_t max_rest, int32_t halfw) { return (max_rest + 2u * (uint32_t)halfw + 16u) & ~3u; }
// ... and beside the codes and tables a CONT launch stages kB16RowCap entries of the kept row per pair
TR_HD bool front_tier_fits(int KB, int32_t halfw, uint32_t max_rest) {
  return 4ull * front_code_cap(max_rest, halfw) + b16_table_bytes(KB) + 32ull * kB16RowCap <= kBandLdsHard;
}
// bytes: tables, codes, the kept row (twice: place, certify)
TR_HD Credit front_credit(uint32_t m_rest, uint32_t n, int KB, int32_t halfw) {
  return Credit{(uint64_t)b16_strips(m_rest, KB) * KB * (uint64_t)(KB + 2 * halfw),
                12ull * m_rest + m_rest + 2ull * halfw + 4ull * (2 * halfw + KB) + 8ull * n};
}

// ---- sweeps ----
// a full sweep of m x n; a profile side moves its six float rows, a string side its bytes
TR_HD Credit sweep_pair_credit(uint32_t m, uint32_t n, bool a1_profile, bool a2_profile) {
  return Credit{(uint64_t)m * n, (a1_profile ? 24ull * m : m) + (a2_profile ? 24ull * n : n) + 4};
}
// the first `rows` rows of a profile x code pair with the last of them kept: the codes, and a dword per column of the kept row
TR_HD Credit prefix_credit(uint32_t m, uint32_t n, uint32_t rows) { return Credit{(uint64_t)(m < rows ? m : rows) * n, (uint64_t)rows + n + 4ull * n}; }

// ---- the order of the sweeps of a launch list: strip height, then the 16-term flag (profile x profile; 0 elsewhere), then cells, all
// descending -- long problems start early, short ones fill the tail.  The sites sort stably, and only a list not already in order. ----
struct SweepKey { int K; uint32_t flag; uint64_t cells; };
TR_HD bool sweep_before(const SweepKey& x, const SweepKey& y) {
  if (x.K != y.K) return x.K > y.K;
  if (x.flag != y.flag) return x.flag > y.flag;
  return x.cells > y.cells;
}
// "of a size": one strip height, one flag, cell counts within a quarter of the smallest -- such a list keeps the caller's order (the
// order only balances the tail of a launch).  A predicate of the keys alone, so pairs (run_dp) and traces (plan_common, mt x rn of
// the full sweeps it queues) take the same one; sums of slices add up with add(SizeSpan).
struct SizeSpan {
  bool any = false, one = true;
  int K = 0;
  uint32_t flag = 0;
  uint64_t lo = ~0ull, hi = 0;
  TR_HD void add(const SweepKey& k) {
    if (!any) { any = true; K = k.K; flag = k.flag; }
    one = one && k.K == K && k.flag == flag;
    lo = k.cells < lo ? k.cells : lo;
    hi = k.cells > hi ? k.cells : hi;
  }
  TR_HD void add(const SizeSpan& o) {
    if (!o.any) return;
    if (!any) { *this = o; return; }
    one = one && o.one && o.K == K && o.flag == flag;
    lo = o.lo < lo ? o.lo : lo;
    hi = o.hi > hi ? o.hi : hi;
  }
  TR_HD bool of_a_size() const { return one && hi <= lo + lo / 4; }
};

}  // namespace tracyhip
#endif
