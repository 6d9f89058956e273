// ragged_plan.h -- the HIP-free pieces of a batch call over ragged traces with host payloads (basecall_plan.h, pad_plan.h and their .hip
// files): the span of an array that a chunk of consecutive traces touches, the test that an offset + length stays within 64 bits, the
// layout of a staging buffer, and the merger of the copies that bring each trace's reported entries back.  tests/cpp/basecall_plan.cpp
// and tests/cpp/pad_plan.cpp run them under the sanitizers.
#ifndef TRACY_AMD_RAGGED_PLAN_H
#define TRACY_AMD_RAGGED_PLAN_H

#include <algorithm>
#include <cstdint>
#include <utility>

namespace tracyhip {

struct Span {  // elements [lo, hi) of one array that a chunk touches
  uint64_t lo = ~0ull, hi = 0;
  void add(uint64_t a, uint64_t len) { lo = std::min(lo, a); hi = std::max(hi, a + len); }
  uint64_t size() const { return hi > lo ? hi - lo : 0; }
  Span with(uint64_t a, uint64_t len) const { Span s = *this; s.add(a, len); return s; }
};

// off + len stays within 64 bits
inline bool offset_fits(uint64_t off, uint64_t len) { return off <= ~0ull - len; }

// byte offsets of the parts of a staging buffer, each aligned to 16; total() has 16 spare bytes
struct Layout {
  uint64_t at[8] = {0};
  int n = 0;
  uint64_t add(uint64_t bytes) { at[n + 1] = at[n] + ((bytes + 15) & ~15ull); return at[n++]; }
  uint64_t total() const { return at[n] + 16; }
};

// The copies that bring regions of N staged result arrays back to the caller's.  The arrays of a group share their offsets, counted
// in elements, and differ in element width; width 0: the array is null and never copied.  add() takes one trace's reported entries:
// `len` elements at `rel` of the staged arrays go to `dst` of the caller's.  Regions that follow each other on both sides travel as
// one run.  A finished run goes to emit(k, src byte offset, dst byte offset, bytes) once per array; what emit returns is an error
// unless it is 0 (hipError_t on the device side, int in the host test), and add() / flush() hand it on.
template <int N, class Emit>
struct RunMerger {
  using Err = decltype(std::declval<Emit&>()(0, uint64_t(), uint64_t(), uint64_t()));
  uint32_t width[N];
  Emit emit;
  uint64_t rel = 0, dst = 0, len = 0;
  Err flush() {  // (an error ends the run: the caller gives up)
    Err e = Err();
    for (int k = 0; k < N && len && e == Err(); ++k)
      if (width[k]) e = emit(k, rel * width[k], dst * width[k], len * width[k]);
    len = 0;
    return e;
  }
  Err add(uint64_t r, uint64_t d, uint64_t l) {
    Err e = Err();
    if (len && l && (r != rel + len || d != dst + len)) e = flush();
    if (!len) { rel = r; dst = d; }
    len += l;
    return e;
  }
};

}  // namespace tracyhip
#endif
