// seed_mode_asan.cpp -- a stand-alone run of the counting-table rules of tracy_amd/csrc/seed.h under the sanitizers (not a pytest test):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o seed_mode_asan tests/cpp/seed_mode_asan.cpp -lz -pthread
// The lists of tests/cpp/seed_mode_cases.h (empty and single lists, all equal, all distinct, 30-way ties, values from -65 535 to 2^62,
// probe chains that start in one slot and wrap, tables of 64 slots and of exactly 2 n, four insertion orders each) through
// seed_table_clear / seed_table_insert / seed_table_best, every answer compared with findMaxFreq of tracy_amd/host/seed.hpp.
// Exit code 0 and "ok": no sanitizer report, no list on which the two disagree.
#include <cstdio>

#include "seed_mode_cases.h"

int main() {
  uint64_t total = 0, bad = 0;
  for (uint32_t seed : {20261019u, 1u, 77u}) {
    uint64_t lists = 0;
    bad += seed_mode::run_all(seed, lists);
    total += lists;
  }
  if (bad) {
    std::fprintf(stderr, "%llu of %llu lists disagree with findMaxFreq\n", (unsigned long long)bad, (unsigned long long)total);
    return 1;
  }
  std::printf("ok: %llu lists, table == findMaxFreq on every one\n", (unsigned long long)total);
  return 0;
}
