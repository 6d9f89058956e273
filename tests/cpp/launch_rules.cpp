// launch_rules.cpp -- a stand-alone run of tracy_amd/csrc/launch_rules.h (no HIP, its own main; tests/test_launch_rules_host.py
// builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o launch_rules tests/cpp/launch_rules.cpp
// Every rule of the header against the formula written out here as each site had it before the header existed (run_band16's plan and
// the scan kernels of the stream-ordered pass, run_front_once and the planning kernels, run_prefix_keep_cq / run_ckpt_prefix /
// s_orient_plan_kernel, and the three sites that order sweeps): only the kernels' own size functions of band16.h are taken as given.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../tracy_amd/csrc/dp_plan.h"
#include "../../tracy_amd/csrc/stream_plan.h"

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

// ---- band pairs ----
static void band_pair_tests() {
  const uint32_t sizes[] = {1, 2, 63, 64, 65, 900, 14000};
  CHECK(band_bucket(12) == 0 && band_bucket(8) == 1 && band_bucket(4) == 2 && band_bucket(0) == -1 && band_bucket(15) == -1 && band_bucket(16) == -1);
  uint64_t checked = 0;
  for (int K : {4, 8, 12})
    for (uint32_t m : sizes)
      for (uint32_t n : sizes)
        for (int32_t w = 1; b16_window(K, 0, w - 1) <= b16_max_window(K); ++w)
          for (int32_t dmin : {-(w / 2), 0, (int32_t)n - (int32_t)m - w / 2, -w + 1}) {
            const int32_t dmax = dmin + w - 1;
            CHECK(b16_window(K, dmin, dmax) <= b16_max_window(K));
            PairDesc d{};
            d.m = m; d.n = n; d.ckpt_off = band_pack(dmin, dmax);
            for (int kind : {0, 1}) {
              // dp_plan.h band_word_bytes / stream.hip s_word_bytes
              const uint64_t wb_host = kind == 0 ? ((b16_store_words(d.m, d.n, K, band_dmin(d), band_dmax(d)) * b16_word_bytes(K) + 15u) & ~15ull) : 0;
              const unsigned long long wb_dev = kind == 0 ? ((b16_store_words(d.m, d.n, K, band_dmin(d), band_dmax(d)) * b16_word_bytes(K) + 15ull) & ~15ull) : 0ull;
              CHECK(band_word_bytes(d, K, kind) == wb_host && wb_host == wb_dev && wb_host % 16 == 0);
              // BandTally::add / s_scan_place_kernel
              const uint64_t wds = b16_words(d.m, d.n, K, band_dmin(d), band_dmax(d));
              const uint64_t cells = wds * (uint64_t)K;
              const uint64_t bytes = (kind == 0 ? wds * b16_word_bytes(K) : 0) + 12ull * d.m + d.n + 4;
              const unsigned long long bytes_dev = (kind == 0 ? wds * b16_word_bytes(K) : 0ull) + 12ull * d.m + d.n + 4ull;
              const Credit c = band_credit(d, K, kind);
              CHECK(c.cells == cells && c.bytes == bytes && bytes == bytes_dev);
              ++checked;
            }
          }
  CHECK(checked > 100000);
}

// ---- band launches ----
static void code_cap_tests() {
  int flips_hard[3] = {0, 0, 0}, flips_plan[3] = {0, 0, 0};
  uint32_t last_hard[3] = {0, 0, 0};
  const int Ks[3] = {12, 8, 4};
  for (uint32_t n = 0; n <= 70000; ++n) {
    const uint32_t cap = (n + 7u) & ~3u;
    CHECK(band_code_cap(n) == cap);
    for (int i = 0; i < 3; ++i) {
      const int K = Ks[i];
      const bool hard = 4ull * cap + b16_table_bytes(K) <= 64u * 1024u;                    // dp_plan.h band_lds_fits
      const bool plan = 4ull * ((n + 7u) & ~3u) + b16_table_bytes(K) <= 60u * 1024u;      // stream_plan.h s_fits_lds
      CHECK(band_lds_fits(band_code_cap(n), K, kBandLdsHard) == hard);
      CHECK(band_lds_fits(band_code_cap(n), K, kBandLdsPlan) == plan && s_fits_lds(n, K) == plan);
      CHECK(!plan || hard);
      if (n) {
        const uint32_t pcap = (n - 1 + 7u) & ~3u;
        flips_hard[i] += hard != (4ull * pcap + b16_table_bytes(K) <= 64u * 1024u);
        flips_plan[i] += plan != (4ull * pcap + b16_table_bytes(K) <= 60u * 1024u);
      }
      if (hard) last_hard[i] = n;
    }
    // StreamCall::size_ncap: the longest trace and its margins at K = 12
    CHECK(band_code_cap(n + 200u) == ((n + 200u + 7u) & ~3u));
  }
  for (int i = 0; i < 3; ++i) CHECK(flips_hard[i] == 1 && flips_plan[i] == 1);  // both limits are crossed inside the range, once
  CHECK(last_hard[0] == 14076);  // K = 12: the first reference run_band16 answers ERR_RANGE for has 14 077 columns
}

// ---- tiers of a pruned sweep ----
static uint64_t parent_s_front_cells(uint32_t m_rest) { return (uint64_t)b16_strips(m_rest, 8) * 8u * (8u + 2u * 60u); }
static uint64_t parent_s_front_bytes(uint32_t m_rest, uint32_t n) { return 12ull * m_rest + m_rest + 2ull * 60 + 4ull * (2 * 60 + 8) + 8ull * n; }
static void front_tests(Rng& rng) {
  CHECK(kFrontK1 == 8 && kFrontHalfW1 == 60 && kFrontK == 12 && kFrontHalfW == 90);
  const int KBs[2] = {kFrontK1, kFrontK};
  const int32_t halfws[2] = {kFrontHalfW1, kFrontHalfW};
  for (int i = 0; i < 2; ++i) {
    const int KB = KBs[i];
    const int32_t halfw = halfws[i];
    int flips = 0;
    bool prev = true;
    for (uint32_t max_rest = 1; max_rest <= 16000; ++max_rest) {
      const uint64_t code_cap = (max_rest + 2u * (uint32_t)halfw + 16u) & ~3u;                           // stream.hip front_tier_fits, front_tier; capi.hip run_front_once
      const bool fits = 4ull * code_cap + b16_table_bytes(KB) + 32ull * kB16RowCap <= 64u * 1024u;
      CHECK(front_code_cap(max_rest, halfw) == code_cap && front_tier_fits(KB, halfw, max_rest) == fits);
      flips += fits != prev;
      prev = fits;
    }
    CHECK(flips == 1 && !prev);  // (rests beyond ~14 k rows find no LDS)
    for (int it = 0; it < 400; ++it) {
      const uint32_t m_rest = it < 40 ? (uint32_t)it + 1 : rng.in(1, 16000), n = it % 7 == 0 ? rng.in(0, 3) : rng.in(1, 70000);
      const uint64_t c0 = (uint64_t)b16_strips(m_rest, KB) * KB * (uint64_t)(KB + 2 * halfw);            // run_front_once
      const uint64_t b0 = 12ull * m_rest + m_rest + 2ull * halfw + 4ull * (2 * halfw + KB) + 8ull * n;
      const Credit c = front_credit(m_rest, n, KB, halfw);
      CHECK(c.cells == c0 && c.bytes == b0);
      if (i == 0) CHECK(c.cells == parent_s_front_cells(m_rest) && c.bytes == parent_s_front_bytes(m_rest, n));
    }
  }
  for (uint32_t m = 1; m <= 16000; ++m) CHECK(parent_s_front_cells(m) == front_credit(m, m % 977u, 8, 60).cells);
}

// ---- sweeps and prefixes ----
static void sweep_credit_tests(Rng& rng) {
  for (int it = 0; it < 2000; ++it) {
    const uint32_t m = it % 11 == 0 ? rng.in(0, 2) : rng.in(1, 20000), n = it % 13 == 0 ? rng.in(0, 2) : rng.in(1, 70000);
    for (int a1 = 0; a1 < 2; ++a1)
      for (int a2 = 0; a2 < 2; ++a2) {
        const Credit c = sweep_pair_credit(m, n, a1 != 0, a2 != 0);  // dp_plan.h sweep_credit
        CHECK(c.cells == (uint64_t)m * n && c.bytes == (a1 ? 24ull * m : m) + (a2 ? 24ull * n : n) + 4);
      }
    const Credit c = sweep_pair_credit(m, n, true, false);  // run_ckpt_prefix, s_orient_plan_kernel
    CHECK(c.cells == (uint64_t)m * n && c.bytes == 24ull * m + n + 4);
  }
  std::vector<uint32_t> rows = {kFrontRows};
  for (int K : {4, 8, 12, 15, 16}) rows.push_back((uint32_t)kPrefixLanes * (uint32_t)K);
  for (uint32_t R : rows)
    for (uint32_t m : {0u, 1u, R / 2, R - 1, R, R + 1, 2 * R, 900u, 14000u})
      for (uint32_t n : {0u, 1u, 63u, 900u, 10000u, 70000u}) {
        const Credit c = prefix_credit(m, n, R);
        CHECK(c.cells == (uint64_t)std::min<uint32_t>(m, R) * n);  // run_prefix_keep_cq, run_ckpt_prefix, sweep_credit (DP_PREFIX)
        CHECK(c.cells == (uint64_t)(m < R ? m : R) * n);           // s_orient_plan_kernel
        CHECK(c.bytes == (uint64_t)R + n + 4ull * n);              // run_prefix_keep_cq
        CHECK(c.bytes == (uint64_t)R + 5ull * n);                  // s_orient_plan_kernel, s_allele_plan0_kernel
        if (m >= R) CHECK(c.cells == (uint64_t)R * n);             // s_allele_plan0_kernel (eligible alleles are longer than the prefix)
      }
}

// ---- the order: the three sites as they were ----
struct Item { uint32_t m, n, flags; int K; };
// dp_plan.h sweep_order
static void parent_run_dp_order(const std::vector<PairDesc>& desc, const std::vector<int>& k, std::vector<uint32_t>& order) {
  const uint32_t np = (uint32_t)desc.size();
  order.resize(np);
  for (uint32_t i = 0; i < np; ++i) order[i] = i;
  auto before = [&](uint32_t x, uint32_t y) {
    if (k[x] != k[y]) return k[x] > k[y];
    const uint32_t fx = desc[x].flags & PAIR_ROW4_ZERO, fy = desc[y].flags & PAIR_ROW4_ZERO;
    if (fx != fy) return fx > fy;
    return (uint64_t)desc[x].m * desc[x].n > (uint64_t)desc[y].m * desc[y].n;
  };
  bool similar = true;
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t i = 0; i < np && similar; ++i) {
    const uint64_t c = (uint64_t)desc[i].m * desc[i].n;
    lo = std::min(lo, c); hi = std::max(hi, c);
    similar = k[i] == k[0] && (desc[i].flags & PAIR_ROW4_ZERO) == (desc[0].flags & PAIR_ROW4_ZERO);
  }
  similar = similar && hi <= lo + lo / 4;
  if (!similar && !std::is_sorted(order.begin(), order.end(), before)) std::stable_sort(order.begin(), order.end(), before);
}
// capi.hip run_ckpt_prefix
static void parent_ckpt_prefix_order(const std::vector<PairDesc>& full, const std::vector<int>& fullk, std::vector<uint32_t>& order) {
  const size_t nf = full.size();
  order.assign(nf, 0);
  for (uint32_t i = 0; i < nf; ++i) order[i] = i;
  auto before = [&](uint32_t x, uint32_t y) {
    if (fullk[x] != fullk[y]) return fullk[x] > fullk[y];
    return (uint64_t)full[x].m * full[x].n > (uint64_t)full[y].m * full[y].n;
  };
  if (!std::is_sorted(order.begin(), order.end(), before)) std::stable_sort(order.begin(), order.end(), before);
}
// stream.hip plan_common's pass over the lengths (per slice, then over the slices) and its sweep_order; false: `similar`, the order stays empty
static bool parent_stream_order(const std::vector<uint32_t>& mt, const std::vector<uint32_t>& rn, const std::vector<int>& kof, uint32_t slices,
                                std::vector<uint32_t>& order) {
  const uint32_t nt = (uint32_t)mt.size();
  struct Part { uint64_t cmin, cmax; int k0; bool onek; };
  std::vector<Part> part(slices, Part{~0ull, 0, 0, true});
  for (uint32_t s = 0; s < slices; ++s) {
    const uint32_t lo = (uint32_t)((uint64_t)nt * s / slices), hi = (uint32_t)((uint64_t)nt * (s + 1) / slices);
    Part x{~0ull, 0, 0, true};
    for (uint32_t t = lo; t < hi; ++t) {
      const int K = kof[t];
      if (t == lo) x.k0 = K;
      x.onek = x.onek && K == x.k0;
      const uint64_t c = (uint64_t)mt[t] * rn[t];
      x.cmin = std::min(x.cmin, c); x.cmax = std::max(x.cmax, c);
    }
    part[s] = x;
  }
  bool similar = true;
  uint64_t cmin = ~0ull, cmax = 0;
  int k0 = 0;
  for (const Part& x : part) {
    if (x.cmax == 0 && x.cmin == ~0ull) continue;
    if (!k0) k0 = x.k0;
    similar = similar && x.onek && x.k0 == k0;
    cmin = std::min(cmin, x.cmin); cmax = std::max(cmax, x.cmax);
  }
  similar = similar && cmax <= cmin + cmin / 4;
  order.clear();
  if (similar) return false;
  order.resize(nt);
  for (uint32_t t = 0; t < nt; ++t) order[t] = t;
  auto before = [&](uint32_t x, uint32_t y) {
    if (kof[x] != kof[y]) return kof[x] > kof[y];
    return (uint64_t)mt[x] * rn[x] > (uint64_t)mt[y] * rn[y];
  };
  if (!std::is_sorted(order.begin(), order.end(), before)) std::stable_sort(order.begin(), order.end(), before);
  return true;
}

static int kept = 0, sorted_lists = 0;
static void check_order(const std::vector<Item>& items) {
  const uint32_t n = (uint32_t)items.size();
  std::vector<PairDesc> desc(n);
  std::vector<int> k(n);
  std::vector<uint32_t> mt(n), rn(n);
  for (uint32_t i = 0; i < n; ++i) {
    desc[i] = PairDesc{};
    desc[i].m = mt[i] = items[i].m; desc[i].n = rn[i] = items[i].n; desc[i].flags = items[i].flags; k[i] = items[i].K;
  }
  std::vector<uint32_t> want, got, ident(n);
  for (uint32_t i = 0; i < n; ++i) ident[i] = i;
  // run_dp
  parent_run_dp_order(desc, k, want);
  sweep_order(desc.data(), k.data(), n, got);
  CHECK(got == want);
  kept += n > 1 && want == ident;
  sorted_lists += want != ident;
  // run_ckpt_prefix (no flag; never "of a size")
  parent_ckpt_prefix_order(desc, k, want);
  order_sweeps(n, [&](uint32_t i) { return SweepKey{k[i], 0u, (uint64_t)desc[i].m * desc[i].n}; }, false, got);
  CHECK(got == want);
  // plan_common: the span summed per slice as its pass does, then stream.hip's sweep_order
  for (uint32_t slices : {1u, 3u, 8u}) {
    const bool sorted = parent_stream_order(mt, rn, k, slices, want);
    SizeSpan span;
    for (uint32_t s = 0; s < slices; ++s) {
      SizeSpan x;
      for (uint32_t t = (uint32_t)((uint64_t)n * s / slices); t < (uint32_t)((uint64_t)n * (s + 1) / slices); ++t) x.add(SweepKey{k[t], 0u, (uint64_t)mt[t] * rn[t]});
      span.add(x);
    }
    CHECK(span.of_a_size() == !sorted);
    got.clear();
    if (!span.of_a_size()) order_sweeps(n, [&](uint32_t t) { return SweepKey{k[t], 0u, (uint64_t)mt[t] * rn[t]}; }, false, got);
    CHECK(got == want);
  }
}
static void order_tests(Rng& rng) {
  const int Ks[4] = {4, 8, 12, 15};
  check_order({});
  for (int it = 0; it < 3000; ++it) {
    const uint32_t n = it < 40 ? (uint32_t)it / 4 : rng.in(1, 300);
    const int shape = it % 8;  // 0-2: anything; 3: one K, many ties; 4: sorted; 5: reverse-sorted; 6, 7: one K at the 25 % edge
    std::vector<Item> items(n);
    const int oneK = Ks[rng.in(0, 3)];
    const uint32_t flagmask = shape < 3 && it % 3 == 0 ? (PAIR_ROW4_ZERO | PAIR_A2_REVCOMP) : PAIR_A2_REVCOMP;
    for (Item& x : items) {
      x.K = (shape == 3 || shape >= 6) ? oneK : Ks[rng.in(0, 3)];
      x.flags = rng.next() & flagmask;
      x.m = shape == 3 ? 10 * rng.in(1, 3) : rng.in(1, 1100);
      x.n = shape == 3 ? 100 * rng.in(1, 2) : rng.in(1, 12000);
    }
    auto key = [](const Item& x) { return SweepKey{x.K, x.flags & PAIR_ROW4_ZERO, (uint64_t)x.m * x.n}; };
    if (shape == 4 || shape == 5) {
      std::stable_sort(items.begin(), items.end(), [&](const Item& x, const Item& y) { return sweep_before(key(x), key(y)); });
      if (shape == 5) std::reverse(items.begin(), items.end());
    }
    if (shape >= 6 && n) {  // cells lo .. lo + lo / 4 (kept) or one more (sorted), the extremes anywhere in the list
      const uint32_t lo = rng.in(1, 40000), hi = lo + lo / 4 + (shape == 7 ? 1 : 0);
      for (Item& x : items) { x.m = 1; x.n = rng.in(lo, lo + lo / 4); x.flags = 0; }
      const uint32_t at = rng.in(0, n - 1);
      items[at].n = lo;
      if (n > 1) items[(at + 1 + rng.in(0, n - 2)) % n].n = hi;
    }
    check_order(items);
  }
  CHECK(kept > 200 && sorted_lists > 1000);  // both outcomes occur
  // the comparator itself: K, then the flag, then cells, all descending; equal keys are not before each other
  CHECK(sweep_before(SweepKey{12, 0, 1}, SweepKey{8, 2, 100}) && !sweep_before(SweepKey{8, 2, 100}, SweepKey{12, 0, 1}));
  CHECK(sweep_before(SweepKey{8, 2, 1}, SweepKey{8, 0, 100}) && sweep_before(SweepKey{8, 2, 5}, SweepKey{8, 2, 4}));
  CHECK(!sweep_before(SweepKey{8, 2, 5}, SweepKey{8, 2, 5}));
}

int main() {
  Rng rng{0x9e3779b97f4a7c15ull};
  band_pair_tests();
  code_cap_tests();
  front_tests(rng);
  sweep_credit_tests(rng);
  order_tests(rng);
  if (failures) { std::printf("launch_rules: %d checks FAILED\n", failures); return 1; }
  std::printf("launch_rules: ok\n");
  return 0;
}
