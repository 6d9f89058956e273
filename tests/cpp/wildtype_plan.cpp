// wildtype_plan.cpp -- a stand-alone run of tracy_amd/csrc/wildtype_plan.h (no HIP, its own main; tests/test_wildtype_plan_host.py
// builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o wildtype_plan tests/cpp/wildtype_plan.cpp
// It plans batches of the lengths the device tests use, plus 1 and 64 k +- 1, under several workspace limits and checks: both orders
// are permutations, every run is uniform in strip height and term count, every chunk's planes and boundary rows fit the limit, the
// chunks cover every trace once in both orders, and a trace whose own planes exceed the limit gives the out-of-memory verdict.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tracy_amd/csrc/wildtype_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static std::vector<WtTrace> make_traces(const std::vector<uint32_t>& full, uint32_t trim) {
  std::vector<WtTrace> tr;
  uint32_t i = 0;
  for (uint32_t mf : full)
    for (int rep = 0; rep < 3; ++rep, ++i) {
      uint32_t l = trim, r = trim;
      if ((uint64_t)l + r >= mf) l = r = 0;  // createProfile's clamp
      const uint32_t n = mf - (mf / 8) * (uint32_t)rep / 2;
      tr.push_back(WtTrace{mf, mf - l - r, n ? n : 1, (i * 7u + rep) % 3u ? 1u : 0u});
    }
  return tr;
}

static void check_plan(const std::vector<WtTrace>& tr, uint64_t limit, uint32_t strands, size_t min_chunks) {
  const uint32_t nt = (uint32_t)tr.size();
  WtPlan p;
  if (!wildtype_plan(tr.data(), nt, limit, strands, p)) {
    std::printf("FAILED: no plan under %llu bytes: trace %lld needs %llu\n", (unsigned long long)limit, (long long)p.too_large, (unsigned long long)p.need);
    ++failures;
    return;
  }
  CHECK(p.too_large == -1);
  CHECK(p.trace_order.size() == nt && p.score_order.size() == nt && p.k_trace.size() == nt && p.k_score.size() == nt);
  CHECK(p.chunks.size() >= min_chunks);
  // permutations
  for (const std::vector<uint32_t>* o : {&p.trace_order, &p.score_order}) {
    std::vector<int> seen(nt, 0);
    for (uint32_t t : *o) { CHECK(t < nt); if (t < nt) ++seen[t]; }
    for (uint32_t t = 0; t < nt; ++t) CHECK(seen[t] == 1);
  }
  // the strip heights are those of the rows at every position
  for (uint32_t j = 0; j < nt; ++j) {
    CHECK(p.k_trace[j] == wt_strip_height(tr[p.trace_order[j]].mf));
    CHECK(p.k_score[j] == wt_strip_height(tr[p.score_order[j]].mt));
  }
  // chunks: consecutive, cover [0, nt), hold the same traces in both orders, fit the limit; the offsets of a trace lie inside its chunk
  uint32_t at = 0;
  for (const WtChunk& c : p.chunks) {
    CHECK(c.lo == at && c.hi > c.lo && c.hi <= nt);
    at = c.hi;
    CHECK(c.words * 8 + c.scratch * 8 <= limit);
    std::vector<int> in_trace(nt, 0), in_score(nt, 0);
    uint64_t words = 0, scr = 0;
    for (uint32_t j = c.lo; j < c.hi; ++j) {
      const uint32_t t = p.trace_order[j];
      ++in_trace[t];
      ++in_score[p.score_order[j]];
      CHECK(p.bits_off[t] == words && p.scratch_off[t] == scr);  // laid out in trace order, without holes
      words += wt_plane_words(tr[t].mf, tr[t].n);
      scr += wt_boundary_rows(tr[t].mf, tr[t].mt, tr[t].n, strands);
    }
    CHECK(words == c.words && scr == c.scratch);
    for (uint32_t t = 0; t < nt; ++t) CHECK(in_trace[t] == in_score[t]);
    // inside a chunk each order is sorted: runs of equal (strip height, term count) never come back
    for (int which = 0; which < 2; ++which) {
      const std::vector<uint32_t>& o = which ? p.score_order : p.trace_order;
      const std::vector<int>& k = which ? p.k_score : p.k_trace;
      std::vector<int> closed;  // keys 2 k + row4 of the runs that ended
      for (uint32_t j = c.lo; j < c.hi; ++j) {
        const int key = 2 * k[j] + (int)tr[o[j]].row4;
        if (j > c.lo) {
          const int prev = 2 * k[j - 1] + (int)tr[o[j - 1]].row4;
          if (key != prev) { closed.push_back(prev); CHECK(key < prev); }
        }
        for (int q : closed) CHECK(q != key);
      }
    }
  }
  CHECK(at == nt);
  // the boundary rows hold what the launches use: `strands` rows for a multi-pass score sweep, one for a multi-pass traceback
  for (uint32_t t = 0; t < nt; ++t) {
    const uint64_t have = wt_boundary_rows(tr[t].mf, tr[t].mt, tr[t].n, strands);
    if (wt_passes(tr[t].mt, wt_strip_height(tr[t].mt)) > 1) CHECK(have >= (uint64_t)strands * (tr[t].n + 2ull));
    if (wt_passes(tr[t].mf, wt_strip_height(tr[t].mf)) > 1) CHECK(have >= tr[t].n + 2ull);
  }
}

int main() {
  // the rule itself: 4 rows per lane up to 256 rows, 8 up to 512, 4 (three passes) up to 768, 8 from 769 on
  CHECK(wt_strip_height(0) == 4 && wt_strip_height(1) == 4 && wt_strip_height(256) == 4 && wt_strip_height(257) == 8);
  CHECK(wt_strip_height(512) == 8 && wt_strip_height(513) == 4 && wt_strip_height(768) == 4 && wt_strip_height(769) == 8);
  CHECK(wt_passes(560, 4) == 3 && wt_passes(460, 8) == 1 && wt_passes(869, 8) == 2);
  CHECK(wt_plane_words(869, 869) == 2ull * (869 + 63) * 64);

  const std::vector<uint32_t> small{140, 300, 356, 560, 612, 820, 869, 1};
  const std::vector<WtTrace> a = make_traces(small, 50);
  for (uint32_t strands = 1; strands <= 2; ++strands) {
    check_plan(a, ~0ull >> 1, strands, 1);
    check_plan(a, 4ull << 20, strands, 3);
    check_plan(a, 1ull << 20, strands, 8);  // (the largest trace alone takes 954 368 + 13 936 bytes)
  }
  const std::vector<uint32_t> large{65535, 65536, 65537, 869, 1};
  const std::vector<WtTrace> b = make_traces(large, 50);
  check_plan(b, ~0ull >> 1, 2, 1);
  check_plan(b, 10ull << 30, 2, 2);  // (65 537 rows: 257 passes of 4, 8.6 GB of planes for one trace)
  // a trace whose own planes exceed the limit: the verdict names it and what it needs
  {
    WtPlan p;
    CHECK(!wildtype_plan(a.data(), (uint32_t)a.size(), 900000, 2, p));
    CHECK(p.too_large >= 0 && a[(size_t)p.too_large].mf >= 820);
    CHECK(p.need > 900000 && p.need == wt_plane_words(a[(size_t)p.too_large].mf, a[(size_t)p.too_large].n) * 8 +
                                            wt_boundary_rows(a[(size_t)p.too_large].mf, a[(size_t)p.too_large].mt, a[(size_t)p.too_large].n, 2) * 8);
    WtPlan q;
    CHECK(!wildtype_plan(b.data(), (uint32_t)b.size(), 1ull << 30, 2, q) && q.too_large >= 0 && b[(size_t)q.too_large].mf >= 65535);
  }
  // no traces
  {
    WtPlan p;
    CHECK(wildtype_plan(nullptr, 0, 1, 2, p) && p.chunks.empty() && p.trace_order.empty());
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("wildtype_plan: ok\n");
  return 0;
}
