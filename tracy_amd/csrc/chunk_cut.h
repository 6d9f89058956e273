// chunk_cut.h -- the additive greedy cut every workspace plan of the library uses, free of HIP (tests/cpp/dp_plan.cpp).
//
// Items arrive in order.  Each counts `bytes` against the limit and adds to up to two running sums (words, scratch) whose values
// before the item are its offsets inside its chunk.  A chunk of consecutive items closes before an item when it already holds one
// and the counted bytes would pass the limit; an item whose own bytes pass the limit is refused (the caller words the error).
//
// "Holds an item" and "has a non-zero sum" are the same test here: a chunk whose counted sum is zero cannot be overflowed by an
// admissible item (0 + bytes <= limit), so items of no cost at the head of a chunk never close it, whichever of the two is asked.
// Items that are not there at all (a group without work) `ride` along: they widen the range and count as nothing.
#ifndef TRACY_AMD_CHUNK_CUT_H
#define TRACY_AMD_CHUNK_CUT_H

#include <cstdint>
#include <vector>

namespace tracyhip {

struct CutChunk {
  uint32_t lo, hi;                 // items [lo, hi)
  uint64_t bytes, words, scratch;  // the counted sum and the two running sums
};

struct ChunkCut {
  uint64_t limit;
  std::vector<CutChunk> chunks;  // the closed chunks; chunks.size() is the index of the open one
  CutChunk c{0, 0, 0, 0, 0};     // the open chunk: c.words / c.scratch after add() are the sums INCLUDING the item
  uint64_t words_off = 0, scratch_off = 0, bytes_off = 0;  // of the item add() took last
  bool held = false;
  int64_t refused = -1;  // the item add() refused, and its bytes
  uint64_t refused_bytes = 0;

  explicit ChunkCut(uint64_t limit_) : limit(limit_) {}
  // item j (every index once, ascending, through add or ride).  false: it does not fit on its own.
  bool add(uint32_t j, uint64_t bytes, uint64_t words = 0, uint64_t scratch = 0) {
    if (bytes > limit) { refused = j; refused_bytes = bytes; return false; }
    if (held && c.bytes + bytes > limit) {
      chunks.push_back(c);
      c = CutChunk{j, j, 0, 0, 0};
    }
    bytes_off = c.bytes; words_off = c.words; scratch_off = c.scratch;
    c.bytes += bytes; c.words += words; c.scratch += scratch;
    c.hi = j + 1;
    held = true;
    return true;
  }
  void ride(uint32_t j) { c.hi = j + 1; }
  // closes the last chunk (none for an empty list) and hands the list over
  std::vector<CutChunk>& finish() {
    if (c.hi > c.lo) chunks.push_back(c);
    c = CutChunk{c.hi, c.hi, 0, 0, 0};
    held = false;
    return chunks;
  }
};

}  // namespace tracyhip
#endif
