// wildtype_plan.h -- what the host plans for a wildtype job of tracyhip_align_traces (wildtype.hip) between the class read-back and the
// launches, free of HIP so that it builds on its own and runs under a sanitizer (tests/cpp/wildtype_plan.cpp).
//
// Per trace the call runs two dynamic programs of DIFFERENT heights against its wildtype (n columns): the orientation scores over the
// trimmed view (mt rows) and the traceback over the full profile (mf rows).  Strip height and pass count follow the rows, so the same
// trace may sit in a run of strips of 4 for its scores and of 8 for its traceback (mt = 200, mf = 300), or score in one pass of 8 and
// trace back in three of 4 (mt = 460, mf = 560).  Hence two launch orders:
//   trace order   every trace by (strip height of mf descending, 16-term body first); the chunks are cut along it: consecutive
//                 traces whose traceback planes (full height) and boundary rows fit the workspace limit
//   score order   the traces of each chunk again, by (strip height of mt descending, 16-term body first)
// Positions [lo, hi) of both orders hold the same traces, so one chunk is one range of either descriptor list.
#ifndef TRACY_AMD_WILDTYPE_PLAN_H
#define TRACY_AMD_WILDTYPE_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "chunk_cut.h"

namespace tracyhip {

// choose_k (capi.hip) for profile x profile: the cheaper of 8 and 4 rows per lane by passes x height, 8 on a tie
inline uint32_t wt_passes(uint32_t m, int K) { return (m + 64u * (uint32_t)K - 1u) / (64u * (uint32_t)K); }
inline int wt_strip_height(uint32_t m) {
  const uint32_t mm = m ? m : 1;
  return (uint64_t)wt_passes(mm, 4) * 4 < (uint64_t)wt_passes(mm, 8) * 8 ? 4 : 8;
}
// traceback words of mf rows against n columns (dp_lane.h word_index: 64 words per step, n + 63 steps per pass)
inline uint64_t wt_plane_words(uint32_t mf, uint32_t n) { return (uint64_t)wt_passes(mf, wt_strip_height(mf)) * ((uint64_t)n + 63u) * 64u; }
// boundary rows in int2 units: one per strand of the score launch where the trimmed height takes several passes, and the traceback's
// where the full height does.  The traceback runs behind the scores of its chunk and reuses their space.
inline uint64_t wt_boundary_rows(uint32_t mf, uint32_t mt, uint32_t n, uint32_t strands) {
  const uint64_t row = (uint64_t)n + 2u;
  const uint64_t sc = wt_passes(mt, wt_strip_height(mt)) > 1 ? strands * row : 0;
  const uint64_t tr = wt_passes(mf, wt_strip_height(mf)) > 1 ? row : 0;
  return std::max(sc, tr);
}

struct WtTrace {   // one trace as the plan sees it
  uint32_t mf;     // rows of the full profile
  uint32_t mt;     // rows of the trimmed view (createProfile's clamp applied)
  uint32_t n;      // columns of its wildtype
  uint32_t row4;   // row 4 ('N') is zero in the trace AND in its wildtype: the 16-term score body
};
struct WtChunk {
  uint32_t lo, hi;         // range of both orders
  uint64_t words, scratch; // traceback words (8 bytes each), boundary rows (int2: 8 bytes each)
};
struct WtPlan {
  std::vector<uint32_t> trace_order, score_order;  // trace index at every position
  std::vector<int> k_trace, k_score;               // strip height at every position of the two orders
  std::vector<uint64_t> bits_off, scratch_off;     // per TRACE: where its planes / boundary rows start inside its chunk
  std::vector<WtChunk> chunks;
  int64_t too_large = -1;                          // a trace whose own planes and rows exceed the limit (the call answers out of memory), else -1
  uint64_t need = 0;                               // ... and what it needs, in bytes
};

// strands: 2 (both orientation scores) or 1 (caller-oriented profiles).  false: plan.too_large / plan.need say which trace did not fit.
inline bool wildtype_plan(const WtTrace* tr, uint32_t nt, uint64_t limit, uint32_t strands, WtPlan& p) {
  p = WtPlan();
  p.trace_order.resize(nt);
  for (uint32_t i = 0; i < nt; ++i) p.trace_order[i] = i;
  std::stable_sort(p.trace_order.begin(), p.trace_order.end(), [&](uint32_t x, uint32_t y) {
    const int kx = wt_strip_height(tr[x].mf), ky = wt_strip_height(tr[y].mf);
    if (kx != ky) return kx > ky;
    return tr[x].row4 > tr[y].row4;
  });
  p.bits_off.assign(nt, 0);
  p.scratch_off.assign(nt, 0);
  ChunkCut cut(limit);
  for (uint32_t j = 0; j < nt; ++j) {
    const WtTrace& t = tr[p.trace_order[j]];
    const uint64_t words = wt_plane_words(t.mf, t.n);
    const uint64_t scr = wt_boundary_rows(t.mf, t.mt, t.n, strands);
    if (!cut.add(j, words * 8 + scr * 8, words, scr)) {
      p.too_large = p.trace_order[j];
      p.need = cut.refused_bytes;
      return false;
    }
    p.bits_off[p.trace_order[j]] = cut.words_off;
    p.scratch_off[p.trace_order[j]] = cut.scratch_off;
  }
  for (const CutChunk& c : cut.finish()) p.chunks.push_back(WtChunk{c.lo, c.hi, c.words, c.scratch});
  p.score_order = p.trace_order;
  for (const WtChunk& ch : p.chunks)
    std::stable_sort(p.score_order.begin() + ch.lo, p.score_order.begin() + ch.hi, [&](uint32_t x, uint32_t y) {
      const int kx = wt_strip_height(tr[x].mt), ky = wt_strip_height(tr[y].mt);
      if (kx != ky) return kx > ky;
      return tr[x].row4 > tr[y].row4;
    });
  p.k_trace.resize(nt);
  p.k_score.resize(nt);
  for (uint32_t j = 0; j < nt; ++j) {
    p.k_trace[j] = wt_strip_height(tr[p.trace_order[j]].mf);
    p.k_score[j] = wt_strip_height(tr[p.score_order[j]].mt);
  }
  return true;
}

}  // namespace tracyhip
#endif
