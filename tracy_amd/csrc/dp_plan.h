// dp_plan.h -- what the host plans for the two drivers every pipeline launches through (capi.hip run_dp, run_band16) between the
// caller's pair list and the launches: the order, the chunks that fit the workspace, bits_off / scratch_off of every pair, the
// launches and what the timers are credited for them.  Free of HIP, so that it builds on its own and runs under a sanitizer
// (tests/cpp/dp_plan.cpp).
//
// Long lists are laid out in slices: `exec(n, fn)` calls fn(lo, hi, slice) over contiguous ascending slices of [0, n), at most
// kPlanSlices of them, in any order or at once, and cuts the same n the same way every time.  Production passes parallel_for
// (capi_internal.h), the test a serial one.
#ifndef TRACY_AMD_DP_PLAN_H
#define TRACY_AMD_DP_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "band16.h"
#include "chunk_cut.h"
#include "dp_kernels.h"
#include "launch_rules.h"

namespace tracyhip {

// stage: DP_PLAIN = score-only or full-matrix traceback; DP_CKPT = score-only pass that also writes wavefront
// checkpoints + last-row values (PairDesc::ckpt_off / lastrow_off set by the caller); DP_BAND = band traceback
// from those checkpoints (trace must be true); DP_PREFIX = prefix bound of the semiglobal score (rows 1 .. kPrefixLanes*K of
// profile x code pairs, 16-bit domain): d_scores receives max_j max(H, F) of that row.
// DP_ORIGIN = origin-tracking sweep of string x string pairs (DpCkpt::d_ends receives {lead, end} per pair, d_scores H(m,n)).
enum { DP_PLAIN = 0, DP_CKPT = 1, DP_BAND = 2, DP_PREFIX = 3, DP_ORIGIN = 4 };

constexpr uint32_t kPlanSlices = 8;
struct SerialExec {
  template <class Fn>
  void operator()(uint32_t n, Fn fn) const { fn(0u, n, 0u); }
};

// ---- the sweeps (run_dp) --------------------------------------------------------------------------------------------
struct SweepRun { uint32_t lo, hi; int K; uint32_t row4; };  // one launch: positions [lo, hi) of one strip height and one term count
struct SweepPlan {
  std::vector<uint32_t> order;   // pair index at every position
  std::vector<CutChunk> chunks;  // positions [lo, hi); words and scratch in their own units (traceback words, int2 rows)
  std::vector<SweepRun> runs;    // in launch order; no run crosses a chunk
  uint64_t max_words = 0, max_scratch = 0;  // of one chunk
  uint32_t max_pairs = 0;                   // ... and its most pairs
  uint64_t max_mn = 0;                      // largest m + n
  int64_t too_large = -1;                   // the first pair (in launch order) whose own traceback words pass the limit, else -1
  uint64_t need = 0;                        // ... and their bytes
};

// traceback words of a pair (a full-matrix traceback only) and its strip hand-over row (multi-pass pairs with cells only)
inline uint64_t sweep_words(const PairDesc& d, int K, bool planes) { return (planes && d.m && d.n) ? (uint64_t)num_passes(d.m, K) * steps_per_pass(d.n) * 64 : 0; }
inline uint64_t sweep_scratch(const PairDesc& d, int K) { return (d.m && d.n && num_passes(d.m, K) > 1) ? (uint64_t)d.n + 2 : 0; }

// order[i] = i, then sorted by sweep_before (launch_rules.h) over key(i): stably, and only a list that is not in order already.
// keep: the caller's order stays (a list "of a size")
template <class Key>
void order_sweeps(uint32_t n, Key key, bool keep, std::vector<uint32_t>& order) {
  order.resize(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  auto before = [&](uint32_t x, uint32_t y) { return sweep_before(key(x), key(y)); };
  if (!keep && !std::is_sorted(order.begin(), order.end(), before)) std::stable_sort(order.begin(), order.end(), before);
}
// run_dp's order.  Batches of a size -- the final alignments of a `tracy align` batch -- keep the caller's and save the host the sort
// between two kernels (profile x profile: 16-term pairs and 25-term pairs go to different launches, hence the flag)
inline void sweep_order(const PairDesc* desc, const int* k, uint32_t np, std::vector<uint32_t>& order) {
  auto key = [&](uint32_t i) { return SweepKey{k[i], desc[i].flags & PAIR_ROW4_ZERO, (uint64_t)desc[i].m * desc[i].n}; };
  SizeSpan span;
  for (uint32_t i = 0; i < np && span.one; ++i) span.add(key(i));
  order_sweeps(np, key, span.of_a_size(), order);
}

// The plan of one run_dp call.  hd (np entries: the pinned staging block) receives the descriptors in launch order with bits_off and
// scratch_off set.  Only the traceback words count against the limit (words x 4 for needle, x 8 otherwise); the scratch is summed.
// false: p.too_large / p.need say which pair did not fit.
template <class Exec>
bool sweep_plan(const PairDesc* desc, const int* k, uint32_t np, bool trace, bool needle, int stage, uint64_t limit, PairDesc* hd, SweepPlan& p, Exec exec) {
  p = SweepPlan();
  sweep_order(desc, k, np, p.order);
  const std::vector<uint32_t>& order = p.order;
  const bool planes = trace && stage == DP_PLAIN;
  const uint64_t word_bytes = needle ? 4 : 8;
  // sizes per slice; then one scan lays the pairs out: over the slices from their sums where everything fits one chunk (an all-pairs
  // job is 36 MB of descriptors), else serially through the cut
  struct Part { uint64_t words = 0, scratch = 0, mn = 0; int64_t bad = -1; };
  Part part[kPlanSlices];
  exec(np, [&](uint32_t lo, uint32_t hi, uint32_t t) {
    Part a;
    for (uint32_t j = lo; j < hi; ++j) {
      const PairDesc& d = desc[order[j]];
      const uint64_t words = sweep_words(d, k[order[j]], planes);
      if (a.bad < 0 && words * word_bytes > limit) a.bad = j;
      a.words += words;
      a.scratch += sweep_scratch(d, k[order[j]]);
      a.mn = std::max<uint64_t>(a.mn, (uint64_t)d.m + d.n);
    }
    part[t] = a;
  });
  uint64_t words_before[kPlanSlices], scratch_before[kPlanSlices], tot_words = 0, tot_scratch = 0;
  for (uint32_t t = 0; t < kPlanSlices; ++t) {
    if (part[t].bad >= 0 && p.too_large < 0) {
      p.too_large = order[part[t].bad];
      p.need = sweep_words(desc[p.too_large], k[p.too_large], planes) * word_bytes;
    }
    words_before[t] = tot_words; scratch_before[t] = tot_scratch;
    tot_words += part[t].words; tot_scratch += part[t].scratch;
    p.max_mn = std::max(p.max_mn, part[t].mn);
  }
  if (p.too_large >= 0) return false;
  auto lay = [&](uint32_t lo, uint32_t hi, ChunkCut& cut) {
    for (uint32_t j = lo; j < hi; ++j) {
      PairDesc d = desc[order[j]];
      const uint64_t words = sweep_words(d, k[order[j]], planes);
      cut.add(j, words * word_bytes, words, sweep_scratch(d, k[order[j]]));
      d.bits_off = cut.words_off;
      d.scratch_off = cut.scratch_off;
      hd[j] = d;
    }
  };
  if (tot_words * word_bytes <= limit) {
    exec(np, [&](uint32_t lo, uint32_t hi, uint32_t t) {
      ChunkCut cut(~0ull);
      cut.c.words = words_before[t]; cut.c.scratch = scratch_before[t];
      lay(lo, hi, cut);
    });
    p.chunks.push_back(CutChunk{0, np, tot_words * word_bytes, tot_words, tot_scratch});
  } else {
    ChunkCut cut(limit);
    lay(0, np, cut);
    p.chunks.swap(cut.finish());
  }
  for (const CutChunk& c : p.chunks) {
    p.max_words = std::max(p.max_words, c.words); p.max_scratch = std::max(p.max_scratch, c.scratch); p.max_pairs = std::max(p.max_pairs, c.hi - c.lo);
    for (uint32_t j = c.lo, e; j < c.hi; j = e) {  // one launch per run of equal K (and, profile x profile, equal term count)
      const int K = k[order[j]];
      const uint32_t row4 = hd[j].flags & PAIR_ROW4_ZERO;
      for (e = j; e < c.hi && k[order[e]] == K && (hd[e].flags & PAIR_ROW4_ZERO) == row4; ++e) {}
      p.runs.push_back(SweepRun{j, e, K, row4});
    }
  }
  return true;
}

// What the timers are credited for the launch of hd[lo, hi) at strip height K: the cells it evaluates and the bytes it moves.
inline void sweep_credit(const PairDesc* hd, uint32_t lo, uint32_t hi, int K, bool trace, int stage, bool a1_profile, bool a2_profile, uint64_t& cells, uint64_t& bytes) {
  cells = bytes = 0;
  for (uint32_t q = lo; q < hi; ++q) {
    const PairDesc& d = hd[q];
    const Credit full = sweep_pair_credit(d.m, d.n, a1_profile, a2_profile);
    uint64_t mn = stage == DP_PREFIX ? prefix_credit(d.m, d.n, (uint32_t)kPrefixLanes * K).cells : full.cells;
    if (trace && stage == DP_PLAIN && (d.flags & PAIR_BANDED)) {  // multi-pass band form: the cells its passes sweep, not the matrix
      mn = 0;
      for (uint32_t base = 0; base < d.m; base += 64u * K) {
        const uint32_t rows_here = std::min<uint32_t>(d.m - base, 64u * K);
        const int64_t c_lo = std::max<int64_t>(1, (int64_t)base + 1 + band_dmin(d)), c_hi = std::min<int64_t>(d.n, (int64_t)(base + rows_here) + band_dmax(d));
        if (c_hi >= c_lo) mn += (uint64_t)rows_here * (uint64_t)(c_hi - c_lo + 1);
      }
    }
    cells += mn;
    bytes += (trace ? mn / 2 : 0) + full.bytes;
  }
  if (stage == DP_BAND) bytes = 0;  // (the bands live in a per-pair buffer, no matrix-sized traffic)
}

// ---- the band kernels (run_band16) ----------------------------------------------------------------------------------
constexpr int kBandHeights = 3;
constexpr int kBandK[kBandHeights] = {12, 8, 4};  // launch order: the caller's order within one height (the pairs of a pipeline stage are of a size)
constexpr uint32_t kBandMultiMax = 24576;  // pairs: up to here a launch of several heights is few waves, and band16_multi_kernel takes them at once

inline bool band_in_domain(const PairDesc& d, int K) { return band_bucket(K) >= 0 && d.m != 0 && d.n != 0 && b16_window(K, band_dmin(d), band_dmax(d)) <= b16_max_window(K); }
struct BandTally {  // the pairs of one height in one launch: count, longest reference, word bytes, and what the timers are credited
  uint32_t n = 0, nmax = 0;
  uint64_t word_bytes = 0, cells = 0, bytes = 0;
  void add(const PairDesc& d, int K, int kind, uint64_t wb, bool credit) {
    n += 1;
    nmax = std::max(nmax, d.n);
    word_bytes += wb;
    if (!credit) return;
    const Credit c = band_credit(d, K, kind);
    cells += c.cells;
    bytes += c.bytes;
  }
  void add(const BandTally& o) { n += o.n; nmax = std::max(nmax, o.nmax); word_bytes += o.word_bytes; cells += o.cells; bytes += o.bytes; }
};
struct BandLaunch {
  int K;                                             // 12, 8, 4: one height (launch_band16); 0: up to three at once (launch_band16_multi)
  uint32_t first[kBandHeights], count[kBandHeights]; // per height the positions [first, first + count)
  uint32_t nmax, code_cap;
  uint64_t cells, bytes;                             // timer credit
  bool fits;                                         // its code rows fit the staging area (else the call answers ERR_RANGE, naming nmax)
};
struct BandPlan {
  BandTally part[kPlanSlices][kBandHeights], all[kBandHeights];
  std::vector<uint64_t> wb;  // per pair of the job: bytes of traceback words
  bool bad = false;          // a pair outside the kernels' domain
  uint32_t np = 0;           // pairs with a strip height
  uint64_t total_bytes = 0;
  std::vector<int> hk;       // strip height at every position
  std::vector<CutChunk> chunks;
  std::vector<BandLaunch> launches;
  uint64_t max_bytes = 0;    // of one chunk
  int64_t too_large = -1;    // a pair whose own words pass the limit, else -1
  uint64_t need = 0;
};

// the launches of the positions from `lo` on that `t` counts per height
inline void band_launches(const BandTally* t, uint32_t lo, std::vector<BandLaunch>& out) {
  uint32_t first[kBandHeights], used = 0;
  BandTally sum;
  for (int b = 0; b < kBandHeights; ++b) { first[b] = lo + sum.n; used += t[b].n != 0; sum.add(t[b]); }
  const uint32_t cap_all = band_code_cap(sum.nmax);
  if (sum.n <= kBandMultiMax && used > 1 && band_lds_fits(cap_all, 12, kBandLdsHard)) {  // few waves, several heights: band16_multi_kernel
    BandLaunch l{0, {first[0], first[1], first[2]}, {t[0].n, t[1].n, t[2].n}, sum.nmax, cap_all, sum.cells, sum.bytes, true};
    out.push_back(l);
    return;
  }
  for (int b = 0; b < kBandHeights; ++b) {
    if (t[b].n == 0) continue;
    BandLaunch l{kBandK[b], {first[b], first[b], first[b]}, {0, 0, 0}, t[b].nmax, band_code_cap(t[b].nmax), t[b].cells, t[b].bytes, false};
    l.count[b] = t[b].n;
    l.fits = band_lds_fits(l.code_cap, l.K, kBandLdsHard);
    out.push_back(l);
  }
}

// First half: domain, word bytes and the sums per height (the limit may depend on total_bytes).  k[i] == 0: pair i is not of this job.
template <class Exec>
void band_sizes(const PairDesc* desc, const int* k, uint32_t nall, int kind, bool credit, BandPlan& p, Exec exec) {
  p = BandPlan();
  p.wb.resize(nall);
  bool bad[kPlanSlices] = {};
  exec(nall, [&](uint32_t lo, uint32_t hi, uint32_t t) {
    for (uint32_t i = lo; i < hi; ++i) {
      const int K = k[i];
      p.wb[i] = 0;
      if (K == 0) continue;
      const PairDesc& d = desc[i];
      if (!band_in_domain(d, K)) { bad[t] = true; continue; }
      p.wb[i] = band_word_bytes(d, K, kind);
      p.part[t][band_bucket(K)].add(d, K, kind, p.wb[i], credit);
    }
  });
  for (uint32_t t = 0; t < kPlanSlices; ++t) {
    p.bad = p.bad || bad[t];
    for (int b = 0; b < kBandHeights; ++b) p.all[b].add(p.part[t][b]);
  }
  for (int b = 0; b < kBandHeights; ++b) { p.np += p.all[b].n; p.total_bytes += p.all[b].word_bytes; }
}

// Second half, everything in one chunk: positions and word offsets from the scan over (strip height, slice)
template <class Exec>
void band_place_whole(const PairDesc* desc, const int* k, uint32_t nall, PairDesc* hd, BandPlan& p, Exec exec) {
  uint32_t pos0[kBandHeights][kPlanSlices], pos = 0;
  uint64_t off0[kBandHeights][kPlanSlices], off = 0;
  for (int b = 0; b < kBandHeights; ++b)
    for (uint32_t t = 0; t < kPlanSlices; ++t) { pos0[b][t] = pos; off0[b][t] = off; pos += p.part[t][b].n; off += p.part[t][b].word_bytes; }
  p.hk.resize(p.np);
  exec(nall, [&](uint32_t lo, uint32_t hi, uint32_t t) {
    uint32_t pp[kBandHeights];
    uint64_t oo[kBandHeights];
    for (int b = 0; b < kBandHeights; ++b) { pp[b] = pos0[b][t]; oo[b] = off0[b][t]; }
    for (uint32_t i = lo; i < hi; ++i) {
      const int K = k[i];
      if (K == 0) continue;
      const int b = band_bucket(K);
      PairDesc d = desc[i];
      d.bits_off = oo[b];
      oo[b] += p.wb[i];
      hd[pp[b]] = d;
      p.hk[pp[b]] = K;
      ++pp[b];
    }
  });
  p.chunks.push_back(CutChunk{0, p.np, p.total_bytes, 0, 0});
  band_launches(p.all, 0, p.launches);
  p.max_bytes = p.total_bytes;
}
// ... the words do not fit the workspace at once: chunks of consecutive pairs (serial; rare).  false: p.too_large / p.need.
inline bool band_place_cut(const PairDesc* desc, const int* k, uint32_t nall, int kind, bool credit, uint64_t limit, PairDesc* hd, BandPlan& p) {
  p.hk.resize(p.np);
  ChunkCut cut(limit);
  BandTally t[kBandHeights];
  uint32_t pos = 0;
  for (int b = 0; b < kBandHeights; ++b)
    for (uint32_t i = 0; i < nall; ++i) {
      if (k[i] != kBandK[b]) continue;
      const size_t closed = cut.chunks.size();
      if (!cut.add(pos, p.wb[i])) { p.too_large = i; p.need = p.wb[i]; return false; }
      if (cut.chunks.size() != closed) {
        band_launches(t, cut.chunks.back().lo, p.launches);
        for (BandTally& x : t) x = BandTally();
      }
      PairDesc d = desc[i];
      d.bits_off = cut.bytes_off;
      hd[pos] = d;
      p.hk[pos] = kBandK[b];
      ++pos;
      t[b].add(d, kBandK[b], kind, p.wb[i], credit);
    }
  band_launches(t, cut.c.lo, p.launches);
  p.chunks.swap(cut.finish());
  for (const CutChunk& c : p.chunks) p.max_bytes = std::max(p.max_bytes, c.bytes);
  return true;
}
// hd: p.np entries (the pinned staging block)
template <class Exec>
bool band_place(const PairDesc* desc, const int* k, uint32_t nall, int kind, bool credit, uint64_t limit, PairDesc* hd, BandPlan& p, Exec exec) {
  if (p.total_bytes > limit) return band_place_cut(desc, k, nall, kind, credit, limit, hd, p);
  band_place_whole(desc, k, nall, hd, p, exec);
  return true;
}

}  // namespace tracyhip
#endif
