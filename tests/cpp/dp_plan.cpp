// dp_plan.cpp -- a stand-alone run of tracy_amd/csrc/dp_plan.h and chunk_cut.h (no HIP, its own main; tests/test_dp_plan_host.py
// builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o dp_plan tests/cpp/dp_plan.cpp
// The plans of run_dp and run_band16 against a restatement written here (a greedy cut, the sort key, the sizes, the launch rules
// spelled out again; only the kernels' own size functions of band16.h are taken as given), on seeded random jobs and on the edges:
// the chunks tile the list and fit the limit, no two pairs of a chunk share traceback words or scratch, an oversized pair is named
// with its bytes, the runs tile the chunks and are uniform, the order is the stated one, and a layout split over 1, 2, 3, 8 slices
// run in reverse equals the serial one.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/dp_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { if (failures < 50) std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
  uint32_t in(uint32_t lo, uint32_t hi) { return lo + next() % (hi - lo + 1); }
};
// the slices of [0, n) in reverse order
struct SplitExec {
  uint32_t s;
  template <class Fn>
  void operator()(uint32_t n, Fn fn) const {
    for (uint32_t t = s; t-- > 0;) fn((uint32_t)((uint64_t)n * t / s), (uint32_t)((uint64_t)n * (t + 1) / s), t);
  }
};
struct Job { std::vector<PairDesc> desc; std::vector<int> k; };
static void push(Job& j, uint32_t m, uint32_t n, int K, uint32_t flags = 0, int32_t dmin = 0, int32_t dmax = 0) {
  PairDesc d{};
  d.m = m; d.n = n; d.flags = flags; d.out = (uint32_t)j.desc.size(); d.a1_off = 7 * j.desc.size(); d.ckpt_off = band_pack(dmin, dmax);
  j.desc.push_back(d);
  j.k.push_back(K);
}
static bool same_desc(const PairDesc& a, const PairDesc& b) { return std::memcmp(&a, &b, sizeof(PairDesc)) == 0; }

// ---- the restatement ----
struct Item { uint64_t bytes, words, scratch; bool rides; };
struct MChunk { uint32_t lo, hi; uint64_t bytes, words, scratch; };
enum NonEmpty { HOLDS_ITEM, SUM_NONZERO };
// greedy cut; -1 or the first item too large on its own.  off: per item {words, scratch, bytes} before it
static int64_t model_cut(const std::vector<Item>& it, uint64_t limit, NonEmpty rule, std::vector<MChunk>& ch, std::vector<Item>& off) {
  ch.clear(); off.assign(it.size(), Item{0, 0, 0, false});
  MChunk c{0, 0, 0, 0, 0};
  uint32_t held = 0;
  for (uint32_t j = 0; j < it.size(); ++j) {
    if (it[j].rides) { c.hi = j + 1; continue; }
    if (it[j].bytes > limit) return j;
    const bool nonempty = rule == HOLDS_ITEM ? held != 0 : c.bytes != 0;
    if (nonempty && c.bytes + it[j].bytes > limit) { c.hi = j; ch.push_back(c); c = MChunk{j, j, 0, 0, 0}; held = 0; }
    off[j] = Item{c.bytes, c.words, c.scratch, false};
    c.bytes += it[j].bytes; c.words += it[j].words; c.scratch += it[j].scratch; c.hi = j + 1; ++held;
  }
  if (c.hi > c.lo) ch.push_back(c);
  return -1;
}
static bool same_chunks(const std::vector<MChunk>& m, const std::vector<CutChunk>& c) {
  if (m.size() != c.size()) return false;
  for (size_t i = 0; i < m.size(); ++i)
    if (m[i].lo != c[i].lo || m[i].hi != c[i].hi || m[i].bytes != c[i].bytes || m[i].words != c[i].words || m[i].scratch != c[i].scratch) return false;
  return true;
}
// [off, off + len) of the items of one chunk: disjoint and inside [0, sum)
static void check_ranges(std::vector<std::pair<uint64_t, uint64_t>> r, uint64_t sum) {
  std::sort(r.begin(), r.end());
  uint64_t end = 0;
  for (auto& x : r) {
    if (x.second == 0) continue;
    CHECK(x.first >= end);
    end = x.first + x.second;
  }
  CHECK(end <= sum);
}

// ---- the cutter alone ----
static void check_cutter(Rng& rng) {
  for (int round = 0; round < 400; ++round) {
    const uint32_t n = rng.in(0, 40);
    const uint64_t limit = round % 7 == 0 ? 0 : rng.in(1, 60);
    std::vector<Item> it(n);
    for (Item& x : it) {
      const uint32_t kind = rng.in(0, 5);  // many items of no cost, some that are not there at all
      x = Item{kind < 2 ? 0 : (uint64_t)rng.in(1, (uint32_t)std::max<uint64_t>(limit, 1)), rng.in(0, 9), rng.in(0, 9), kind == 0 && round % 2};
      if (x.bytes > limit) x.bytes = 0;
    }
    std::vector<MChunk> a, b;
    std::vector<Item> oa, ob;
    CHECK(model_cut(it, limit, HOLDS_ITEM, a, oa) == -1);
    CHECK(model_cut(it, limit, SUM_NONZERO, b, ob) == -1);
    ChunkCut cut(limit);
    for (uint32_t j = 0; j < n; ++j) {
      if (it[j].rides) { cut.ride(j); continue; }
      CHECK(cut.add(j, it[j].bytes, it[j].words, it[j].scratch));
      CHECK(cut.bytes_off == oa[j].bytes && cut.words_off == oa[j].words && cut.scratch_off == oa[j].scratch);
      CHECK(cut.bytes_off == ob[j].bytes && cut.words_off == ob[j].words && cut.scratch_off == ob[j].scratch);
    }
    const std::vector<CutChunk>& c = cut.finish();
    CHECK(same_chunks(a, c));  // "holds an item" ...
    CHECK(same_chunks(b, c));  // ... and "its counted sum is not zero" cut alike
    uint32_t at = 0;
    for (const CutChunk& x : c) { CHECK(x.lo == at && x.hi > x.lo && x.bytes <= limit); at = x.hi; }
    CHECK(at == n);
  }
  ChunkCut cut(10);
  CHECK(cut.add(0, 0) && cut.add(1, 10) && !cut.add(2, 11));
  CHECK(cut.refused == 2 && cut.refused_bytes == 11);
  CHECK(cut.finish().size() == 1);
  CHECK(ChunkCut(5).finish().empty());
}

// ---- the sweep plan ----
static uint32_t m_passes(uint32_t m, int K) { return (m + 64u * (uint32_t)K - 1u) / (64u * (uint32_t)K); }
static uint64_t m_words(const PairDesc& d, int K, bool planes) { return (planes && d.m && d.n) ? (uint64_t)m_passes(d.m, K) * (d.n + 63ull) * 64 : 0; }
static uint64_t m_scratch(const PairDesc& d, int K) { return (d.m && d.n && m_passes(d.m, K) > 1) ? d.n + 2ull : 0; }

template <class Exec>
static bool run_sweep(const Job& job, bool trace, bool needle, int stage, uint64_t limit, std::vector<PairDesc>& hd, SweepPlan& p, Exec exec) {
  hd.assign(job.desc.size(), PairDesc{});
  return sweep_plan(job.desc.data(), job.k.data(), (uint32_t)job.desc.size(), trace, needle, stage, limit, hd.data(), p, exec);
}

// returns the number of chunks, 0 where the plan refused a pair
static size_t check_sweep(const Job& job, bool trace, bool needle, int stage, uint64_t limit) {
  const uint32_t np = (uint32_t)job.desc.size();
  const bool planes = trace && stage == DP_PLAIN;
  const uint64_t wb = needle ? 4 : 8;
  std::vector<PairDesc> hd;
  SweepPlan p;
  const bool ok = run_sweep(job, trace, needle, stage, limit, hd, p, SerialExec());
  // the order: a permutation; the caller's for a similar list, else sorted (stably) by K, flag, m * n, all descending
  CHECK(p.order.size() == np);
  std::vector<int> seen(np, 0);
  for (uint32_t x : p.order) { CHECK(x < np); if (x < np) ++seen[x]; }
  for (uint32_t i = 0; i < np; ++i) CHECK(seen[i] == 1);
  auto row4 = [&](uint32_t i) { return job.desc[i].flags & PAIR_ROW4_ZERO; };
  auto cells = [&](uint32_t i) { return (uint64_t)job.desc[i].m * job.desc[i].n; };
  bool similar = true;
  uint64_t cmin = ~0ull, cmax = 0;
  for (uint32_t i = 0; i < np; ++i) {
    similar = similar && job.k[i] == job.k[0] && row4(i) == row4(0);
    cmin = std::min(cmin, cells(i)); cmax = std::max(cmax, cells(i));
  }
  similar = similar && cmax <= cmin + cmin / 4;
  for (uint32_t j = 0; j + 1 < np; ++j) {
    const uint32_t x = p.order[j], y = p.order[j + 1];
    if (similar) { CHECK(x == j && y == j + 1); continue; }
    const bool equal = job.k[x] == job.k[y] && row4(x) == row4(y) && cells(x) == cells(y);
    const bool before = job.k[x] != job.k[y] ? job.k[x] > job.k[y] : row4(x) != row4(y) ? row4(x) > row4(y) : cells(x) > cells(y);
    CHECK(equal ? x < y : before);
  }
  // the cut, along that order
  std::vector<Item> it(np);
  uint64_t max_mn = 0;
  for (uint32_t j = 0; j < np; ++j) {
    const PairDesc& d = job.desc[p.order[j]];
    const uint64_t w = m_words(d, job.k[p.order[j]], planes);
    it[j] = Item{w * wb, w, m_scratch(d, job.k[p.order[j]]), false};
    max_mn = std::max<uint64_t>(max_mn, (uint64_t)d.m + d.n);
  }
  std::vector<MChunk> mc;
  std::vector<Item> off;
  const int64_t big = model_cut(it, limit, HOLDS_ITEM, mc, off);
  if (big >= 0) {
    CHECK(!ok && p.too_large == (int64_t)p.order[big] && p.need == it[big].bytes);
    return 0;
  }
  CHECK(ok && p.too_large == -1);
  if (!ok) return 0;
  CHECK(same_chunks(mc, p.chunks));
  CHECK(p.max_mn == max_mn);
  uint32_t at = 0;
  uint64_t max_words = 0, max_scr = 0;
  uint32_t max_pairs = 0;
  size_t r = 0;
  for (const CutChunk& c : p.chunks) {
    CHECK(c.lo == at && c.hi > c.lo && c.hi <= np);
    at = c.hi;
    CHECK(c.bytes <= limit && c.bytes == c.words * wb);
    max_words = std::max(max_words, c.words); max_scr = std::max(max_scr, c.scratch); max_pairs = std::max(max_pairs, c.hi - c.lo);
    std::vector<std::pair<uint64_t, uint64_t>> rw, rs;
    for (uint32_t j = c.lo; j < c.hi && j < np; ++j) {
      PairDesc want = job.desc[p.order[j]];
      want.bits_off = off[j].words; want.scratch_off = off[j].scratch;
      CHECK(same_desc(hd[j], want));
      rw.emplace_back(hd[j].bits_off, it[j].words);
      rs.emplace_back(hd[j].scratch_off, it[j].scratch);
    }
    check_ranges(rw, c.words);
    check_ranges(rs, c.scratch);
    // the runs of this chunk: they tile it, each of one height and one flag, and neighbours differ
    uint32_t q = c.lo;
    for (; r < p.runs.size() && p.runs[r].lo < c.hi; ++r) {
      const SweepRun& run = p.runs[r];
      CHECK(run.lo == q && run.hi > run.lo && run.hi <= c.hi);
      for (uint32_t j = run.lo; j < run.hi && j < np; ++j) CHECK(job.k[p.order[j]] == run.K && row4(p.order[j]) == run.row4);
      if (run.lo > c.lo) CHECK(job.k[p.order[run.lo - 1]] != run.K || row4(p.order[run.lo - 1]) != run.row4);
      q = run.hi;
    }
    CHECK(q == c.hi);
  }
  CHECK(at == np && r == p.runs.size());
  CHECK(p.max_words == max_words && p.max_scratch == max_scr && p.max_pairs == max_pairs);
  // the layout over slices, run in reverse, is the serial one
  for (uint32_t s : {1u, 2u, 3u, 8u}) {
    std::vector<PairDesc> hd2;
    SweepPlan p2;
    CHECK(run_sweep(job, trace, needle, stage, limit, hd2, p2, SplitExec{s}));
    CHECK(p2.order == p.order && same_chunks(mc, p2.chunks) && p2.runs.size() == p.runs.size());
    CHECK(p2.max_words == p.max_words && p2.max_scratch == p.max_scratch && p2.max_mn == p.max_mn && p2.max_pairs == p.max_pairs);
    for (uint32_t j = 0; j < np; ++j) CHECK(same_desc(hd[j], hd2[j]));
    for (size_t i = 0; i < p.runs.size() && i < p2.runs.size(); ++i)
      CHECK(p.runs[i].lo == p2.runs[i].lo && p.runs[i].hi == p2.runs[i].hi && p.runs[i].K == p2.runs[i].K && p.runs[i].row4 == p2.runs[i].row4);
  }
  return p.chunks.size();
}

static void sweep_tests(Rng& rng) {
  static const int heights[3] = {4, 8, 16};
  for (int round = 0; round < 300; ++round) {
    Job job;
    const uint32_t np = rng.in(1, 120);
    const bool one_k = round % 5 == 0;
    for (uint32_t i = 0; i < np; ++i)
      push(job, rng.in(0, 20) ? rng.in(1, 2500) : 0, rng.in(0, 20) ? rng.in(1, 700) : 0, heights[one_k ? 0 : rng.in(0, 2)], rng.in(0, 1) ? PAIR_ROW4_ZERO : 0u);
    uint64_t big = 0, total = 0;
    for (uint32_t i = 0; i < np; ++i) { const uint64_t b = m_words(job.desc[i], job.k[i], true) * 8; big = std::max(big, b); total += b; }
    check_sweep(job, false, false, DP_PLAIN, ~0ull);
    check_sweep(job, false, false, DP_CKPT, 1);        // no traceback words: one chunk under any limit, the scratch is only summed
    CHECK(check_sweep(job, true, false, DP_BAND, 1) == 1);
    CHECK(check_sweep(job, true, false, DP_PLAIN, ~0ull) == 1);
    CHECK(check_sweep(job, true, false, DP_PLAIN, total) == 1);
    check_sweep(job, true, false, DP_PLAIN, big + rng.in(0, 1000) * (total - big) / 1000);
    check_sweep(job, true, false, DP_PLAIN, big);
    check_sweep(job, true, true, DP_PLAIN, big / 2 + rng.in(0, 1000) * (total - big) / 2000);  // needle: 4-byte words
    if (big) CHECK(check_sweep(job, true, false, DP_PLAIN, big - 1) == 0);
  }
  {  // a similar list keeps the caller's order, although it is not sorted
    Job job;
    for (uint32_t m : {400u, 480u, 410u, 500u, 405u}) push(job, m, 100, 8);
    std::vector<PairDesc> hd;
    SweepPlan p;
    CHECK(run_sweep(job, false, false, DP_PLAIN, ~0ull, hd, p, SerialExec()));
    for (uint32_t j = 0; j < 5; ++j) CHECK(p.order[j] == j);
    check_sweep(job, true, false, DP_PLAIN, ~0ull);
    push(job, 501, 100, 8);  // ... 501 > 400 + 100: sorted now
    CHECK(run_sweep(job, false, false, DP_PLAIN, ~0ull, hd, p, SerialExec()));
    CHECK(p.order[0] == 5 && p.order[1] == 3 && p.order[5] == 0);
    check_sweep(job, true, false, DP_PLAIN, ~0ull);
  }
  // one pair; no rows or no columns; the last height of one pass and the first of two
  for (int K : heights)
    for (uint32_t m : {0u, 1u, 64u * K - 1, 64u * K, 64u * K + 1, 128u * K, 128u * K + 1})
      for (uint32_t n : {0u, 1u, 333u}) {
        Job one;
        push(one, m, n, K);
        const uint64_t bytes = m_words(one.desc[0], K, true) * 8;
        CHECK(check_sweep(one, true, false, DP_PLAIN, bytes) == 1);  // a limit of exactly its bytes
        if (bytes) CHECK(check_sweep(one, true, false, DP_PLAIN, bytes - 1) == 0);
        std::vector<PairDesc> hd;
        SweepPlan p;
        CHECK(run_sweep(one, true, false, DP_PLAIN, ~0ull, hd, p, SerialExec()));
        CHECK(p.chunks[0].scratch == ((m > 64u * K && n) ? n + 2ull : 0ull));
        Job three = one;
        push(three, m, n, K);
        push(three, m, n, K);
        CHECK(check_sweep(three, true, false, DP_PLAIN, bytes) == (bytes ? 3u : 1u));  // every pair its own chunk
      }
}

// ---- the band plan ----
struct MLaunch { int K; uint32_t first[3], count[3], nmax, cap; uint64_t cells, bytes; bool fits; };
static const int kHeights[3] = {12, 8, 4};
static uint32_t m_cap(uint32_t nmax) { return (nmax + 7u) / 4u * 4u; }
static bool m_fits(uint32_t cap, int K) { return 4ull * cap + 6ull * K * 64 * 2 <= 65536; }
static void model_launches(const std::vector<PairDesc>& hd, const std::vector<int>& hk, uint32_t lo, uint32_t hi, int kind, bool credit, std::vector<MLaunch>& out) {
  auto one = [&](int K, bool every) {
    MLaunch l{every ? 0 : K, {lo, lo, lo}, {0, 0, 0}, 0, 0, 0, 0, false};
    for (uint32_t j = lo; j < hi; ++j) {
      if (!every && hk[j] != K) continue;
      const int b = hk[j] == 12 ? 0 : hk[j] == 8 ? 1 : 2;
      if (l.count[b]++ == 0) l.first[b] = j;
      l.nmax = std::max(l.nmax, hd[j].n);
      if (!credit) continue;
      const uint64_t wds = b16_words(hd[j].m, hd[j].n, hk[j], band_dmin(hd[j]), band_dmax(hd[j]));
      l.cells += wds * (uint64_t)hk[j];
      l.bytes += (kind == 0 ? wds * (hk[j] == 4 ? 2 : hk[j] == 8 ? 4 : 8) : 0) + 12ull * hd[j].m + hd[j].n + 4;
    }
    l.cap = m_cap(l.nmax);
    l.fits = m_fits(l.cap, every ? 12 : K);
    return l;
  };
  const MLaunch all = one(0, true);
  const int used = (all.count[0] != 0) + (all.count[1] != 0) + (all.count[2] != 0);
  if (hi - lo <= 24576u && used > 1 && all.fits) { out.push_back(all); return; }
  for (int K : kHeights) {
    const MLaunch l = one(K, false);
    if (l.count[0] + l.count[1] + l.count[2]) out.push_back(l);
  }
}
static bool same_launches(const std::vector<MLaunch>& m, const std::vector<BandLaunch>& l) {
  if (m.size() != l.size()) return false;
  for (size_t i = 0; i < m.size(); ++i) {
    if (m[i].K != l[i].K || m[i].nmax != l[i].nmax || m[i].cap != l[i].code_cap || m[i].cells != l[i].cells || m[i].bytes != l[i].bytes || m[i].fits != l[i].fits) return false;
    for (int b = 0; b < 3; ++b)
      if (m[i].count[b] != l[i].count[b] || (m[i].count[b] && m[i].first[b] != l[i].first[b])) return false;
  }
  return true;
}
static bool same_plan(const BandPlan& a, const std::vector<PairDesc>& ha, const BandPlan& b, const std::vector<PairDesc>& hb) {
  if (a.np != b.np || a.hk != b.hk || a.max_bytes != b.max_bytes || a.chunks.size() != b.chunks.size() || a.launches.size() != b.launches.size()) return false;
  for (uint32_t j = 0; j < a.np; ++j) if (!same_desc(ha[j], hb[j])) return false;
  for (size_t i = 0; i < a.chunks.size(); ++i)
    if (a.chunks[i].lo != b.chunks[i].lo || a.chunks[i].hi != b.chunks[i].hi || a.chunks[i].bytes != b.chunks[i].bytes) return false;
  for (size_t i = 0; i < a.launches.size(); ++i) {
    const BandLaunch &x = a.launches[i], &y = b.launches[i];
    if (x.K != y.K || x.nmax != y.nmax || x.code_cap != y.code_cap || x.cells != y.cells || x.bytes != y.bytes || x.fits != y.fits) return false;
    for (int h = 0; h < 3; ++h) if (x.first[h] != y.first[h] || x.count[h] != y.count[h]) return false;
  }
  return true;
}

enum Place { PLACE, PLACE_CUT };
template <class Exec>
static bool run_band(const Job& job, int kind, bool credit, uint64_t limit, Place how, std::vector<PairDesc>& hd, BandPlan& p, Exec exec) {
  const uint32_t nall = (uint32_t)job.desc.size();
  band_sizes(job.desc.data(), job.k.data(), nall, kind, credit, p, exec);
  if (p.bad) return false;
  hd.assign(p.np, PairDesc{});
  return how == PLACE_CUT ? band_place_cut(job.desc.data(), job.k.data(), nall, kind, credit, limit, hd.data(), p)
                          : band_place(job.desc.data(), job.k.data(), nall, kind, credit, limit, hd.data(), p, exec);
}

// returns the number of chunks, 0 where the plan refused a pair
static size_t check_band(const Job& job, int kind, bool credit, uint64_t limit, std::vector<BandLaunch>* launches = nullptr) {
  const uint32_t nall = (uint32_t)job.desc.size();
  std::vector<PairDesc> hd;
  BandPlan p;
  const bool ok = run_band(job, kind, credit, limit, PLACE, hd, p, SerialExec());
  CHECK(!p.bad);
  // launch order: by height 12, 8, 4, the caller's order within one
  std::vector<uint32_t> pos;
  for (int K : kHeights)
    for (uint32_t i = 0; i < nall; ++i) if (job.k[i] == K) pos.push_back(i);
  const uint32_t np = (uint32_t)pos.size();
  CHECK(p.np == np);
  std::vector<Item> it(np);
  uint64_t total = 0;
  for (uint32_t j = 0; j < np; ++j) {
    const PairDesc& d = job.desc[pos[j]];
    const int K = job.k[pos[j]];
    const uint64_t bytes = kind == 0 ? (b16_store_words(d.m, d.n, K, band_dmin(d), band_dmax(d)) * (K == 4 ? 2 : K == 8 ? 4 : 8) + 15) / 16 * 16 : 0;
    CHECK(p.wb[pos[j]] == bytes);
    it[j] = Item{bytes, 0, 0, false};
    total += bytes;
  }
  CHECK(p.total_bytes == total);
  std::vector<MChunk> mc;
  std::vector<Item> off;
  const int64_t big = model_cut(it, limit, HOLDS_ITEM, mc, off);
  if (big >= 0) {
    CHECK(!ok && p.too_large == (int64_t)pos[big] && p.need == it[big].bytes);
    return 0;
  }
  CHECK(ok);
  if (!ok) return 0;
  CHECK(mc.size() == p.chunks.size());
  std::vector<MLaunch> ml;
  uint32_t at = 0;
  uint64_t max_bytes = 0;
  for (size_t i = 0; i < p.chunks.size() && i < mc.size(); ++i) {
    const CutChunk& c = p.chunks[i];
    CHECK(c.lo == at && c.hi > c.lo && c.hi <= np && c.lo == mc[i].lo && c.hi == mc[i].hi && c.bytes == mc[i].bytes && c.bytes <= limit);
    at = c.hi;
    max_bytes = std::max(max_bytes, c.bytes);
    std::vector<std::pair<uint64_t, uint64_t>> rw;
    for (uint32_t j = c.lo; j < c.hi && j < np; ++j) {
      PairDesc want = job.desc[pos[j]];
      want.bits_off = off[j].bytes;
      CHECK(same_desc(hd[j], want) && p.hk[j] == job.k[pos[j]]);
      rw.emplace_back(hd[j].bits_off, it[j].bytes);
    }
    check_ranges(rw, c.bytes);
    model_launches(hd, p.hk, c.lo, c.hi, kind, credit, ml);
  }
  CHECK(at == np && p.max_bytes == max_bytes);
  CHECK(same_launches(ml, p.launches));
  for (uint32_t s : {1u, 2u, 3u, 8u}) {
    std::vector<PairDesc> hd2;
    BandPlan p2;
    CHECK(run_band(job, kind, credit, limit, PLACE, hd2, p2, SplitExec{s}));
    CHECK(same_plan(p, hd, p2, hd2));
  }
  if (launches) *launches = p.launches;
  return p.chunks.size();
}
// a job that fits one chunk: the scan over the slices and the cut give the same plan
static void check_band_identity(const Job& job, int kind, bool credit) {
  std::vector<PairDesc> h0, h1, h2;
  BandPlan p0, p1, p2;
  CHECK(run_band(job, kind, credit, ~0ull, PLACE, h0, p0, SerialExec()));
  CHECK(run_band(job, kind, credit, p0.total_bytes, PLACE, h1, p1, SerialExec()));
  CHECK(run_band(job, kind, credit, p0.total_bytes, PLACE_CUT, h2, p2, SerialExec()));
  CHECK(p0.chunks.size() == 1 && same_plan(p0, h0, p1, h1) && same_plan(p0, h0, p2, h2));
}
static void push_band(Job& j, Rng& rng, int K, uint32_t m, uint32_t n) {
  const int32_t width = (int32_t)rng.in(0, K == 4 ? 71 : K == 8 ? 127 : 183), dmin = -(int32_t)rng.in(0, (uint32_t)width);
  push(j, m, n, K, 0, dmin, dmin + width);
}
static uint32_t last_n_that_fits(int K) {
  uint32_t n = 1;
  while (m_fits(m_cap(n + 1), K)) ++n;
  return n;
}

static void band_tests(Rng& rng) {
  for (int round = 0; round < 200; ++round) {
    Job job;
    const uint32_t nall = rng.in(1, 150), subset = rng.in(1, 7);
    for (uint32_t i = 0; i < nall; ++i) {
      int K = kHeights[rng.in(0, 2)];
      if (!(subset >> (K == 12 ? 0 : K == 8 ? 1 : 2) & 1)) K = 0;  // (pairs of height 0 are not of the job)
      if (K) push_band(job, rng, K, rng.in(1, 900), rng.in(1, 900));
      else push(job, rng.in(0, 5), rng.in(0, 5), 0);
    }
    const bool credit = round % 2;
    BandPlan sz;
    band_sizes(job.desc.data(), job.k.data(), nall, 0, false, sz, SerialExec());
    if (sz.np == 0) { CHECK(sz.total_bytes == 0 && !sz.bad); continue; }
    uint64_t big = 0;
    for (uint64_t b : sz.wb) big = std::max(big, b);
    CHECK(check_band(job, 0, credit, ~0ull) == 1);
    check_band(job, 0, credit, big);
    check_band(job, 0, credit, big + rng.in(0, 1000) * (sz.total_bytes - big) / 1000);
    CHECK(check_band(job, 0, credit, big - 1) == 0);
    CHECK(check_band(job, 1, credit, 0) == 1);  // the origin form keeps no words
    check_band_identity(job, 0, credit);
    check_band_identity(job, 1, credit);  // (the cut with items of no cost only, under a limit of zero)
  }
  // every subset of the three heights, two pairs each: several heights go at once, one goes alone
  for (uint32_t subset = 0; subset < 8; ++subset) {
    Job job;
    for (int rep = 0; rep < 2; ++rep)
      for (int b = 2; b >= 0; --b) if (subset >> b & 1) push_band(job, rng, kHeights[b], 100 + 10 * b, 120 + rep);
    if (!subset) {  // no pair of the job: the driver returns before it places anything
      push(job, 5, 5, 0);
      BandPlan p;
      band_sizes(job.desc.data(), job.k.data(), 1, 0, true, p, SerialExec());
      CHECK(p.np == 0 && !p.bad && p.total_bytes == 0);
      continue;
    }
    std::vector<BandLaunch> l;
    const int used = (subset & 1) + (subset >> 1 & 1) + (subset >> 2 & 1);
    CHECK(check_band(job, 0, true, ~0ull, &l) == 1);
    CHECK(l.size() == 1 && (l[0].K == 0) == (used > 1));
    check_band_identity(job, 0, true);
  }
  // 24576 pairs of two heights go at once, 24577 height by height (descriptors only)
  for (uint32_t np : {24576u, 24577u}) {
    Job job;
    for (uint32_t i = 0; i < np; ++i) push(job, 50, 60, i % 3 ? 8 : 12, 0, -5, 15);
    std::vector<BandLaunch> l;
    CHECK(check_band(job, 0, true, ~0ull, &l) == 1);
    CHECK(l.size() == (np == 24576u ? 1u : 2u) && (l[0].K == 0) == (np == 24576u));
    check_band_identity(job, 0, false);
  }
  // the longest reference whose code rows fit beside the tables of its height, and the next
  for (int K : kHeights) {
    const uint32_t n = last_n_that_fits(K);
    CHECK(n > 14000 && n < 15700);
    for (uint32_t d : {0u, 1u}) {
      Job job;
      push(job, 64, n + d, K, 0, -10, 10);
      std::vector<BandLaunch> l;
      CHECK(check_band(job, 0, false, ~0ull, &l) == 1);
      CHECK(l.size() == 1 && l[0].K == K && l[0].nmax == n + d && l[0].fits == (d == 0));
    }
  }
  {  // several heights whose longest reference fits its own height's launch but not the common one: height by height
    Job job;
    push(job, 64, last_n_that_fits(4), 4, 0, -10, 10);
    push(job, 64, 100, 12, 0, -10, 10);
    std::vector<BandLaunch> l;
    CHECK(check_band(job, 0, true, ~0ull, &l) == 1);
    CHECK(l.size() == 2 && l[0].K == 12 && l[1].K == 4 && l[0].fits && l[1].fits && l[0].code_cap < l[1].code_cap);
  }
  // outside the kernels' domain: another height, no rows, no columns, a band too wide for the height
  for (int what = 0; what < 4; ++what) {
    Job job;
    push(job, 50, 60, 8, 0, -5, 15);
    push(job, what == 1 ? 0 : 50, what == 2 ? 0 : 60, what == 0 ? 16 : 4, 0, -5, what == 3 ? 67 : 15);
    BandPlan p;
    band_sizes(job.desc.data(), job.k.data(), 2, 0, false, p, SerialExec());
    CHECK(p.bad);
  }
}

int main() {
  Rng rng{0x9e3779b97f4a7c15ull};
  check_cutter(rng);
  sweep_tests(rng);
  band_tests(rng);
  if (failures) { std::printf("dp_plan: %d FAILED\n", failures); return 1; }
  std::printf("dp_plan: ok\n");
  return 0;
}
