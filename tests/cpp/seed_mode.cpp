// seed_mode.cpp -- the counting-table rules of tracy_amd/csrc/seed.h on one host thread and findMaxFreq of tracy_amd/host/seed.hpp
// behind C entry points, for tests/test_seed_mode_host.py.  Lists of int64 in, {frequency, value} out.
#include "seed_mode_cases.h"

extern "C" {
// the table's answer for votes[0 .. n) inserted in that order (capacity 0: seed_table_capacity(n)); 1: every vote found a slot
int sm_table_mode(uint64_t n, const int64_t* votes, uint64_t capacity, int64_t* out) {
  uint32_t f;
  int64_t v;
  const bool ok = seed_mode::table_mode(std::vector<int64_t>(votes, votes + n), capacity, f, v);
  out[0] = f;
  out[1] = v;
  return ok ? 1 : 0;
}
void sm_host_mode(uint64_t n, const int64_t* votes, int64_t* out) {
  uint32_t f;
  int64_t v;
  seed_mode::host_mode(std::vector<int64_t>(votes, votes + n), f, v);
  out[0] = f;
  out[1] = v;
}
uint64_t sm_capacity(uint64_t votes) { return tracyhip::seed_table_capacity(votes); }
uint64_t sm_slot_of(int64_t v, uint64_t capacity) { return tracyhip::seed_slot_of(v, capacity - 1); }
int64_t sm_empty() { return tracyhip::kSeedSlotEmpty; }
// the built-in suite (seed_mode_cases.h): lists that disagree, *lists = lists run
uint64_t sm_run_all(uint32_t seed, uint64_t* lists) { return seed_mode::run_all(seed, *lists); }
}
