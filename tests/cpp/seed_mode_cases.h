// seed_mode_cases.h -- the counting-table rules of tracy_amd/csrc/seed.h (seed_table_capacity, seed_slot_of, seed_table_insert,
// seed_table_best over the one-thread memory policy SeedMemPlain) against findMaxFreq of tracy_amd/host/seed.hpp, for
// tests/cpp/seed_mode.cpp (C entry points of tests/test_seed_mode_host.py) and tests/cpp/seed_mode_asan.cpp (the same runs under the
// sanitizers).
#ifndef TRACY_AMD_TESTS_SEED_MODE_CASES_H
#define TRACY_AMD_TESTS_SEED_MODE_CASES_H

#include <algorithm>
#include <cstdint>
#include <random>
#include <vector>

#include "../../tracy_amd/csrc/seed.h"
#include "../../tracy_amd/host/seed.hpp"

namespace seed_mode {

using namespace tracyhip;

// findMaxFreq of `votes` by the table rules, in the order given: capacity 0 = seed_table_capacity(n).  false: a vote found no slot
inline bool table_mode(const std::vector<int64_t>& votes, uint64_t capacity, uint32_t& freq, int64_t& value) {
  if (capacity == 0) capacity = seed_table_capacity(votes.size());
  std::vector<SeedSlot> tab(capacity);
  seed_table_clear<SeedMemPlain>(tab.data(), capacity, 0, 1);
  bool ok = true;
  for (int64_t v : votes) ok = seed_table_insert<SeedMemPlain>(tab.data(), capacity, v) && ok;
  freq = 0;
  value = 0;
  // (scanned in two interleaved halves, as lanes fold their shares: the tie rule must not depend on who saw a slot first)
  uint32_t l1 = 0;
  int64_t v1 = 0;
  seed_table_best<SeedMemPlain>(tab.data(), capacity, 1, 2, l1, v1);
  seed_table_best<SeedMemPlain>(tab.data(), capacity, 0, 2, freq, value);
  seed_better(freq, value, l1, v1);
  return ok;
}

inline void host_mode(std::vector<int64_t> votes, uint32_t& freq, int64_t& value) { freq = tracy_amd::findMaxFreq(votes, value); }

// `n` values that all start their probe in slot `slot` of a table of `capacity` slots, from `from` upwards
inline std::vector<int64_t> colliding(uint64_t capacity, uint64_t slot, int64_t from, size_t n) {
  std::vector<int64_t> out;
  for (int64_t v = from; out.size() < n; ++v)
    if (seed_slot_of(v, capacity - 1) == slot) out.push_back(v);
  return out;
}

// Every list of the suite; returns the number of lists on which table and host disagree (or a vote found no slot), `lists` counts them
inline uint64_t run_all(uint32_t seed, uint64_t& lists) {
  std::mt19937_64 rng(seed);
  uint64_t bad = 0;
  lists = 0;
  auto check = [&](std::vector<int64_t> votes, uint64_t capacity) {
    uint32_t hf, tf;
    int64_t hv, tv;
    host_mode(votes, hf, hv);
    for (int order = 0; order < 4; ++order) {  // as given, reversed, sorted, shuffled: one answer
      if (order == 1) std::reverse(votes.begin(), votes.end());
      if (order == 2) std::sort(votes.begin(), votes.end());
      if (order == 3) std::shuffle(votes.begin(), votes.end(), rng);
      const bool ok = table_mode(votes, capacity, tf, tv);
      if (!ok || tf != hf || tv != hv) ++bad;
      ++lists;
    }
  };
  const int64_t far = (int64_t)1 << 62;
  check({}, 0);
  check({0}, 0);
  check({-65535}, 0);
  check({far}, 0);
  for (size_t n : {2u, 31u, 32u, 33u, 1000u, 5000u}) {
    check(std::vector<int64_t>(n, 12345), 0);                    // all equal
    check(std::vector<int64_t>(n, -65535), 0);
    std::vector<int64_t> d(n);
    for (size_t i = 0; i < n; ++i) d[i] = (int64_t)i * 7 - 65535;  // all distinct: the smallest wins with a count of 1
    check(d, 0);
    check(d, 2 * n < kSeedTableMin ? kSeedTableMin : seed_table_capacity(n));
  }
  for (int rep = 0; rep < 40; ++rep) {  // 30-way ties of 400 .. 472 votes among noise, near 0, below 0 and near 2^62
    const int64_t base = rep % 3 == 0 ? -65535 : rep % 3 == 1 ? far - 70000 : (int64_t)(rng() % 1000000000);
    const uint32_t top = 400 + (uint32_t)(rng() % 73);
    std::vector<int64_t> v;
    for (int c = 0; c < 30; ++c)
      for (uint32_t i = 0; i < top; ++i) v.push_back(base + (int64_t)c * 601);
    for (int i = 0; i < 500; ++i) v.push_back(base + (int64_t)(rng() % 20000));
    check(v, 0);
  }
  for (int rep = 0; rep < 200; ++rep) {  // seeded lists of every size around the table's steps, few to many distinct values
    const size_t n = (size_t)(rng() % 700);
    const uint64_t span = 1 + rng() % (rep % 2 ? 8 : 4000);
    const int64_t base = rep % 4 == 0 ? -65535 : rep % 4 == 1 ? far : (int64_t)(rng() % 50000000);
    std::vector<int64_t> v(n);
    for (auto& x : v) x = base + (int64_t)(rng() % span);
    check(v, 0);
  }
  for (uint64_t capacity : {kSeedTableMin, (uint64_t)256, (uint64_t)4096}) {  // long probe chains: every value starts in one slot
    for (uint64_t slot : {(uint64_t)0, capacity - 1, capacity / 2}) {         // (the last slot: the chain wraps)
      const size_t n = capacity / 2;                                          // exactly 2 x n slots
      std::vector<int64_t> v = colliding(capacity, slot, -65535, n);
      check(v, capacity);
      std::vector<int64_t> w = v;
      for (size_t i = 0; i < n / 4; ++i) w[n - 1 - i] = v[i % 3];            // ties among the chain's first values
      check(w, capacity);
      std::vector<int64_t> u = colliding(capacity, slot, far, n);
      check(u, capacity);
    }
  }
  return bad;
}

}  // namespace seed_mode
#endif
