// ragged_plan.h -- the HIP-free pieces of a batch call over ragged items (traces, files, alignments) with host payloads (basecall_plan.h,
// pad_plan.h, render_plan.h, read_plan.h, alntext_plan.h and their .hip files): the span of an array that a chunk of consecutive items
// touches, the test that an offset + length stays within 64 bits, the cut of a batch into chunks by their spans, the layout of a staging
// buffer, and the merger of the copies that bring each item's reported entries back.  tests/cpp/span_cut.cpp and the *_plan.cpp programs
// beside it run them under the sanitizers.
//
// There are two cuts.  chunk_cut.h's ChunkCut adds up a size per item: what a chunk holds is the sum over its items.  cut_spans here is
// for chunks whose size is that of the spans they touch: items may overlap, repeat or leave gaps in the caller's arrays, so the size of a
// chunk is not a sum over its items and the open chunk has to be widened and measured anew for every item.
#ifndef TRACY_AMD_RAGGED_PLAN_H
#define TRACY_AMD_RAGGED_PLAN_H

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace tracyhip {

struct Span {  // elements [lo, hi) of one array that a chunk touches
  uint64_t lo = ~0ull, hi = 0;
  void add(uint64_t a, uint64_t len) { lo = std::min(lo, a); hi = std::max(hi, a + len); }
  uint64_t size() const { return hi > lo ? hi - lo : 0; }
  Span with(uint64_t a, uint64_t len) const { Span s = *this; s.add(a, len); return s; }
};

// off + len stays within 64 bits
inline bool offset_fits(uint64_t off, uint64_t len) { return off <= ~0ull - len; }

// The greedy cut of items 0 .. n-1 into chunks of consecutive items.  Chunk: any struct with t0, t1 (items [t0, t1)) that starts empty.
// fits(t): the offsets + lengths of item t stay within 64 bits; widen(chunk, t): the chunk's spans and counters with item t in it;
// over(chunk, limit): the chunk is more than one launch may take (its bytes pass the limit, or its tiles a cap).  A chunk closes in front
// of the item that would put it over; an item alone goes whatever it takes.  false: item *bad_t does not fit (the chunks closed in
// front of it stay in the list, the open one does not join them).  The cut runs per item in front of every launch: the callers' lambdas
// capture by value (a few pointers and flags, which then sit in registers across the loop) and the template is `inline`, so that a cut
// costs what the written-out loops did.
template <class Chunk, class Fits, class Widen, class Over>
inline bool cut_spans(uint32_t n, uint64_t limit, std::vector<Chunk>& chunks, uint32_t* bad_t, Fits fits, Widen widen, Over over) {
  chunks.clear();
  Chunk cur;
  for (uint32_t t = 0; t < n; ++t) {
    if (!fits(t)) {
      *bad_t = t;
      return false;
    }
    Chunk nx = cur;
    nx.t1 = t + 1;
    widen(nx, t);
    if (cur.t1 > cur.t0 && over(nx, limit)) {
      chunks.push_back(cur);
      cur = Chunk{};
      cur.t0 = t;
      --t;  // the item opens the next chunk
      continue;
    }
    cur = nx;
  }
  if (cur.t1 > cur.t0) chunks.push_back(cur);
  return true;
}

// byte offsets of the parts of a staging buffer, each aligned to 16; total() has 16 spare bytes
struct Layout {
  uint64_t at[16] = {0};
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
