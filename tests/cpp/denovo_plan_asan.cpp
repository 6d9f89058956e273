// denovo_plan_asan.cpp -- a stand-alone run of tracy_amd/csrc/denovo_plan.h under the sanitizers (not a pytest test):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o denovo_plan_asan tests/cpp/denovo_plan_asan.cpp
// Seeded strand tables, scores and distance matrices (ties, negative scores, K = 0 .. 12) through denovo_strands, denovo_overlap_ok and
// denovo_tree; every result is checked for what must hold of it whatever the input (tests/test_emu_denovo.py compares the values
// with the oracle).  Exit code 0 and "ok": no sanitizer report, no broken invariant.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../tracy_amd/csrc/denovo_plan.h"

using namespace tracyhip;

#define REQUIRE(x)                                                        \
  do {                                                                    \
    if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } \
  } while (0)

int main() {
  std::mt19937 rng(20240611u);
  uint64_t flips = 0, early = 0, kept = 0;
  for (int iter = 0; iter < 3000; ++iter) {
    const uint32_t K = (uint32_t)(iter % 13);
    const int lo = iter % 5 == 0 ? -30 : 0, hi = iter % 3 == 0 ? 5 : 50;
    std::uniform_int_distribution<int> val(lo, hi);
    std::vector<int32_t> T(denovo_table_size(K) + 1, 0);
    for (uint32_t i = 0; i < K; ++i)
      for (uint32_t j = 0; j < K; ++j)
        for (uint32_t o = 0; o < 4; ++o) T[denovo_table_index(K, i, j, o >> 1, o & 1)] = i == j ? 0x7fffffff : val(rng);  // (the diagonal must not be read)
    std::vector<uint8_t> rev;
    std::vector<int32_t> d;
    denovo_strands(T.data(), K, rev, d);
    REQUIRE(rev.size() == K && d.size() == (size_t)K * K);
    for (uint32_t i = 0; i < K; ++i) {
      REQUIRE(rev[i] <= 1 && d[(size_t)i * K + i] == 0);
      flips += rev[i];
      for (uint32_t j = 0; j < K; ++j) {
        REQUIRE(d[(size_t)i * K + j] == d[(size_t)j * K + i]);
        if (i != j) REQUIRE(d[(size_t)i * K + j] >= lo && d[(size_t)i * K + j] <= hi);
      }
    }
    // the distance matrix of the chosen strands, as denovo.hip reads it from the table
    std::vector<int32_t> dist((size_t)K * K, 0);
    for (uint32_t i = 0; i < K; ++i)
      for (uint32_t j = i + 1; j < K; ++j) dist[(size_t)i * K + j] = T[denovo_table_index(K, i, j, rev[i], rev[j])];
    DenovoTree t;
    denovo_tree(dist.data(), (int32_t)K, t);
    if (K == 0) { REQUIRE(t.order.empty()); continue; }
    REQUIRE(t.root >= 0 && t.root < 2 * (int32_t)K + 1 && t.maxh == t.height[t.root]);
    std::vector<int> seen(K, 0);
    for (uint32_t x : t.order) { REQUIRE(x < K && !seen[x]); seen[x] = 1; }
    REQUIRE(!t.order.empty() && t.order.size() <= K);
    early += t.order.size() < K;
    for (int32_t v = (int32_t)K; v <= t.root; ++v) {
      REQUIRE(t.p[v][1] >= 0 && t.p[v][2] > t.p[v][1] && t.p[v][2] < v);
      REQUIRE(t.height[v] == std::max(t.height[t.p[v][1]], t.height[t.p[v][2]]) + 1);
      if (t.below_root[v]) REQUIRE(t.below_root[t.p[v][1]] && t.below_root[t.p[v][2]]);
    }
    // the overlap verdict on scores around its threshold
    std::uniform_int_distribution<int> na(0, 400);
    for (int k = 0; k < 8; ++k) {
      const int32_t n = na(rng), size = 1 + na(rng);
      const float mf = (float)(rng() % 1001) / 1000.0f;
      const bool a = denovo_overlap_ok(n, 3 * n, size, mf, 3, -5), b = denovo_overlap_ok(n, -5 * n - 1, size, mf, 3, -5);
      REQUIRE(!b && (!a || (n > 25 && 10 * (int64_t)n > size)));
      kept += a;
    }
  }
  REQUIRE(flips > 1000 && early > 50 && kept > 1000);
  std::printf("ok: %llu flips, %llu early stops, %llu overlaps kept\n", (unsigned long long)flips, (unsigned long long)early, (unsigned long long)kept);
  return 0;
}
