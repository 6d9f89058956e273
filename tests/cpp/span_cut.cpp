// span_cut.cpp -- a stand-alone run of cut_spans of tracy_amd/csrc/ragged_plan.h (no HIP, its own main; tests/test_emu_basecall.py
// builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o span_cut tests/cpp/span_cut.cpp
// A toy chunk with one span (bytes) and one tile counter, over hand-made items, so that every verdict of the cut has a case whose answer
// can be read off the items: no item, one item over the limit, a close by bytes, a close by the tile cap, an item inside the open
// chunk's span that costs nothing, and an item whose offset + length leaves 64 bits.
#include <cstdio>
#include <vector>

#include "../../tracy_amd/csrc/ragged_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

struct Item { uint64_t off, len, tiles; };
struct ToyChunk {
  uint32_t t0 = 0, t1 = 0;
  Span span;
  uint64_t tiles = 0;
};
constexpr uint64_t kTileCap = 10;

static bool cut(const std::vector<Item>& items, uint64_t limit, std::vector<ToyChunk>& chunks, uint32_t* bad_t) {
  return cut_spans(
      (uint32_t)items.size(), limit, chunks, bad_t, [&](uint32_t t) { return offset_fits(items[t].off, items[t].len); },
      [&](ToyChunk& c, uint32_t t) { c.span.add(items[t].off, items[t].len); c.tiles += items[t].tiles; },
      [&](const ToyChunk& c, uint64_t lim) { return c.span.size() > lim || c.tiles > kTileCap; });
}

static bool is(const ToyChunk& c, uint32_t t0, uint32_t t1, uint64_t lo, uint64_t hi, uint64_t tiles) {
  return c.t0 == t0 && c.t1 == t1 && c.span.lo == lo && c.span.hi == hi && c.tiles == tiles;
}

int main() {
  std::vector<ToyChunk> chunks(3);  // (what a list held before is gone)
  uint32_t bad = 77;

  CHECK(cut({}, 100, chunks, &bad) && chunks.empty() && bad == 77);

  // one item over the limit goes alone, and so does each of two
  CHECK(cut({{0, 500, 1}}, 100, chunks, &bad) && chunks.size() == 1 && is(chunks[0], 0, 1, 0, 500, 1));
  CHECK(cut({{0, 500, 1}, {500, 500, 1}}, 100, chunks, &bad) && chunks.size() == 2 && is(chunks[0], 0, 1, 0, 500, 1) && is(chunks[1], 1, 2, 500, 1000, 1));

  // a close by bytes: 40 + 40 fit 100, the third item would make 120; the gap in front of the fourth counts as bytes of its span
  CHECK(cut({{0, 40, 1}, {40, 40, 1}, {80, 40, 1}, {200, 10, 1}}, 100, chunks, &bad));
  CHECK(chunks.size() == 3 && is(chunks[0], 0, 2, 0, 80, 2) && is(chunks[1], 2, 3, 80, 120, 1) && is(chunks[2], 3, 4, 200, 210, 1));
  // ... exactly at the limit stays
  CHECK(cut({{0, 40, 1}, {40, 60, 1}}, 100, chunks, &bad) && chunks.size() == 1 && is(chunks[0], 0, 2, 0, 100, 2));

  // a close by the tile cap alone: the bytes would fit many times
  CHECK(cut({{0, 1, 6}, {1, 1, 4}, {2, 1, 1}, {3, 1, 11}, {4, 1, 1}}, 1000, chunks, &bad));
  CHECK(chunks.size() == 4 && is(chunks[0], 0, 2, 0, 2, 10) && is(chunks[1], 2, 3, 2, 3, 1) && is(chunks[2], 3, 4, 3, 4, 11) && is(chunks[3], 4, 5, 4, 5, 1));

  // items inside the open chunk's span, and one repeated, do not grow it: five items of 60 bytes each in a chunk of 100
  CHECK(cut({{0, 60, 1}, {40, 60, 1}, {20, 60, 1}, {40, 60, 1}, {0, 0, 1}, {50, 60, 1}}, 100, chunks, &bad));
  CHECK(chunks.size() == 2 && is(chunks[0], 0, 5, 0, 100, 5) && is(chunks[1], 5, 6, 50, 110, 1));
  // ... in descending order the span grows downwards
  CHECK(cut({{90, 10, 1}, {50, 10, 1}, {0, 10, 1}, {0, 1, 1}}, 60, chunks, &bad));
  CHECK(chunks.size() == 2 && is(chunks[0], 0, 2, 50, 100, 2) && is(chunks[1], 2, 4, 0, 10, 2));

  // limit 1: every item with bytes is alone; unlimited: one chunk up to the tile cap
  CHECK(cut({{0, 4, 1}, {4, 4, 1}, {8, 4, 1}}, 1, chunks, &bad) && chunks.size() == 3 && is(chunks[1], 1, 2, 4, 8, 1));
  CHECK(cut({{0, 4, 1}, {4, 4, 1}, {8, 4, 1}}, ~0ull, chunks, &bad) && chunks.size() == 1 && is(chunks[0], 0, 3, 0, 12, 3));

  // the first item that does not fit is the one reported (the later one is not looked at), and the open chunk does not join the list
  bad = 77;
  CHECK(!cut({{0, 10, 1}, {10, 10, 1}, {~0ull - 3, 4, 1}, {~0ull, 9, 1}}, 100, chunks, &bad) && bad == 2 && chunks.empty());
  CHECK(!cut({{~0ull, 1, 1}}, 100, chunks, &bad) && bad == 0 && chunks.empty());
  CHECK(cut({{~0ull - 4, 4, 1}}, 100, chunks, &bad) && chunks.size() == 1);  // (offset + length = 2^64 - 1 fits)
  // ... chunks closed in front of it stay: the caller gives up on `false` and reads none of them
  CHECK(!cut({{0, 80, 1}, {80, 80, 1}, {~0ull, 2, 1}}, 100, chunks, &bad) && bad == 2 && chunks.size() == 1 && is(chunks[0], 0, 1, 0, 80, 1));

  if (failures) {
    std::printf("span_cut: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("span_cut: ok\n");
  return 0;
}
