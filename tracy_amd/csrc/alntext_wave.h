// alntext_wave.h -- the text of ONE tile of one alignment on ONE wave: plotAlignment (fmindex.h:329-427), the two-record FASTA
// (sage.h:328-339) and the alignment tail of traceAlignJsonOut (json.h:208-216), byte for byte what tracy_amd/host/sage_out.hpp prints
// from the two gapped rows for every alignment it answers.
//
// As in render_wave.h a text is a sequence of SECTIONS, a section a sequence of ITEMS of at most kAlnMaxItem bytes, and a TILE is
// kAlnTile consecutive items of one section, in the order of the text: a tile owns one contiguous piece of the text.
//     PLOT   name0 + '\n' | row 0 ungapped | name1 + '\n' | row 1 ungapped | score line, rule, '\n' | the blocks | spacer, two rules, "\n\n"
//     FASTA  '>' name0 '\n' | row 0 '\n' | '>' name1 " (forward)\n" | row 1 '\n'
//     JSON   ,\n"refchr": " name1 ",\n"refpos": P,\n"altalign": " | row 0 ",\n"refalign": " | row 1 ",\n"forward": F\n}\n
// In front of them every form has a section of one item and no bytes that CHECKS what only the data can tell.
// An ungapped row has one item per COLUMN (a letter, and a '\n' behind every fald-th letter; a gap prints nothing) and a last item, the
// closing '\n' unless the letters fill their last line.  The blocks are cut into items in the order of the text: per block three lines of
// (label | one item per column | '\n'), the last line's '\n' doubled.  linelimit and the tile are independent: a tile starts anywhere
// in a line and may hold many blocks (linelimit 1: 28 of them) or a 256th of one line.
//
// What depends on the DATA in front of an item is the number of letters (bytes other than '-') of a row in front of a column:
//     the line breaks of an ungapped row      letters of that row in front of the column
//     the two counters of a block             letters of row 0 / row 1 in front of the block's first column; their digits decide the bytes
//                                             of a label only for key 3, where setw(9) overflows at 10^9
//     the mirrored check                      letters of row 1 in all
// A tile's ANCHOR is the first column it may ask about: its first column (ungapped rows), the first column of the block of its first
// item (blocks).  AlnTileState keeps the letters of both rows in front of a column and only moves forward from the anchor.
//
// Four bodies, one wave each:
//     alntext_letters_body per COLUMN tile (kAlnTile columns; PLOT only): the letters of both rows in it, into col_letters
//     alntext_count_body   per tile: the letters of both rows in front of its anchor (the sum of the column tiles in front of it, then at
//                          most four steps inside one) into tile_aux, then the bytes of its items (the same alntext_item text as the
//                          emit pass, into a counting sink); the check tile: "row 1 has more letters than ref_len"
//     alntext_scan_body    per alignment: the exclusive sum over its tiles in place (tile offsets), text_len and the status
//     alntext_emit_body    per tile: 64 items at a time into the LDS image of render_wave.h (render_flush: congruent to the destination
//                          modulo 16, whole 16-byte stores, head and tail byte-wise); the anchor counts come from tile_aux.  Every byte
//                          of the text is written exactly once, by the tile that owns it; no atomics.
// Answered: aln_answerable (host-known) and, for a mirrored PLOT, the check.  Anything else is DEFERRED: status and text_len 0.
// No read depends on a row byte: row bytes are printed and compared with '-' and with each other, never used as an index.
//
// W: the wave of dev_wave.h (lane, ballot, bcast, sum, excl_sum, sync, lds).
#ifndef TRACY_AMD_ALNTEXT_WAVE_H
#define TRACY_AMD_ALNTEXT_WAVE_H

#include <cstdint>

#include "dp_lane.h"      // TR_HD
#include "render_wave.h"  // render_digits, RenderCount / RenderWrite, render_flush

namespace tracyhip {

constexpr int32_t kAlnStatusOk = 0, kAlnStatusDeferred = 1, kAlnStatusTooSmall = 2;  // TRACYHIP_ALNTEXT_*
constexpr uint32_t kAlnPlot = 0, kAlnFasta = 1, kAlnJson = 2;                        // TRACYHIP_ALNTEXT_PLOT / FASTA / JSON
constexpr uint32_t kAlnMaxCols = 1u << 22;
constexpr uint32_t kAlnMaxName = 65535;
constexpr uint32_t kAlnMaxLine = 65535;   // linelimit
constexpr uint32_t kAlnTile = 256;        // items per tile
constexpr uint32_t kAlnMaxItem = 48;      // bytes of the longest item: the "refpos" item of the JSON is 38 (alntext_plan.cpp tries the extremes)
constexpr uint32_t kAlnLdsBytes = 64 * kAlnMaxItem + 16;  // the LDS image: a step's items behind up to 15 bytes left over
constexpr uint32_t kAlnAnswerable = 1u, kAlnForward = 2u;  // AlnDesc::flags

enum AlnSection : uint32_t {
  AS_CHECK, AS_NAME0, AS_UNG0, AS_NAME1, AS_UNG1, AS_MIDRULE, AS_BLOCKS, AS_TAIL,  // PLOT
  AS_FNAME0, AS_FROW0, AS_FNAME1, AS_FROW1,                                        // FASTA
  AS_JHEAD, AS_JROW0, AS_JROW1,                                                    // JSON
  AS_NONE
};

struct AlnDesc {  // per alignment, built by the host (alntext_plan.h)
  uint64_t rows_off, name0_off, name1_off;
  uint64_t text_off, text_cap;
  uint32_t cols, name0_len, name1_len, ref_len;
  int32_t ref_pos, score;
  uint32_t tile_first;  // of the launch's tiles; the alignment owns aln_tiles() of them (none where the host can tell it is not answered)
  uint32_t flags;       // kAlnAnswerable | kAlnForward
  uint32_t col_first;   // of the launch's column tiles; an answered alignment of a PLOT owns aln_tiles_of(cols) of them
  uint32_t pad_;
};
struct AlnOut {
  int32_t status;
  uint32_t text_len;
};
struct AlnArgs {
  const uint8_t *rows0, *rows1, *names;
  const AlnDesc* al;
  AlnOut* out;
  uint32_t* tile_bytes;  // per tile: its bytes (count), then its offset in the alignment's text (scan)
  uint32_t* tile_aux;    // per tile two words: the letters of row 0 / row 1 in front of its anchor; the check tile: "row 1 is too long", -
  uint32_t* col_letters; // per column tile two words: the letters of row 0 / row 1 in it (PLOT only)
  uint8_t* text;         // null: sizes only
  uint32_t n, ntiles, ncoltiles, form, key, linelimit;
};

// what the host can tell (the mirrored check is the data's): the reference's int32 / size_t arithmetic has no wrap to reproduce
TR_HD bool aln_answerable(uint32_t cols, uint32_t name0_len, uint32_t name1_len, int32_t ref_pos, uint32_t ref_len) {
  if (cols > kAlnMaxCols || name0_len > kAlnMaxName || name1_len > kAlnMaxName || ref_pos < 0) return false;
  return (uint64_t)ref_pos + (ref_len > cols ? ref_len : cols) + 1u < (1ull << 31);
}

struct AlnShape {  // what the cut into sections, items and tiles depends on
  uint32_t form, linelimit, cols, name0_len, name1_len;
};
TR_HD uint32_t aln_tiles_of(uint32_t items) { return (items + kAlnTile - 1) / kAlnTile; }
TR_HD uint32_t aln_nblocks(uint32_t cols, uint32_t L) { return (cols + L - 1) / L; }
// items of the blocks: per block three lines of a label, its columns and a line end
TR_HD uint32_t aln_block_items(uint32_t cols, uint32_t L) {
  const uint32_t full = cols / L, rem = cols - full * L;
  return full * 3u * (L + 2u) + (rem ? 3u * (rem + 2u) : 0u);  // (at most 9 x cols)
}
TR_HD uint32_t aln_nsections(uint32_t form) { return form == kAlnPlot ? 8u : form == kAlnFasta ? 5u : 4u; }
TR_HD AlnSection aln_section(uint32_t form, uint32_t k) {
  if (k == 0) return AS_CHECK;
  if (form == kAlnPlot) return (AlnSection)(AS_CHECK + k);
  if (form == kAlnFasta) return (AlnSection)(AS_FNAME0 + k - 1);
  return (AlnSection)(AS_JHEAD + k - 1);
}
TR_HD uint32_t aln_items(AlnSection s, const AlnShape& h) {
  const uint32_t fald = h.linelimit + 14u;
  switch (s) {
    case AS_CHECK: return 1;
    case AS_NAME0: return h.name0_len + 1;
    case AS_NAME1: return h.name1_len + 1;
    case AS_UNG0: case AS_UNG1: case AS_FROW0: case AS_FROW1: case AS_JROW0: case AS_JROW1: return h.cols + 1;
    case AS_MIDRULE: return fald + 3;       // the score line | '#', fald - 1 dashes, '\n' | '\n'
    case AS_BLOCKS: return aln_block_items(h.cols, h.linelimit);
    case AS_TAIL: return 2 * fald + 4;      // the spacer | two rules | "\n\n"
    case AS_FNAME0: return h.name0_len + 2;
    case AS_FNAME1: case AS_JHEAD: return h.name1_len + 2;
    default: return 0;
  }
}
TR_HD uint32_t aln_tiles(const AlnShape& h) {
  uint32_t t = 0;
  for (uint32_t k = 0; k < aln_nsections(h.form); ++k) t += aln_tiles_of(aln_items(aln_section(h.form, k), h));
  return t;
}
struct AlnTileAt {
  AlnSection sec;
  uint32_t i0, i1;  // items
};
TR_HD AlnTileAt aln_locate(const AlnShape& h, uint32_t tile) {
  for (uint32_t k = 0; k < aln_nsections(h.form); ++k) {
    const AlnSection s = aln_section(h.form, k);
    const uint32_t items = aln_items(s, h), tiles = aln_tiles_of(items);
    if (tile < tiles) {
      const uint32_t i0 = tile * kAlnTile;
      return AlnTileAt{s, i0, items - i0 < kAlnTile ? items : i0 + kAlnTile};
    }
    tile -= tiles;
  }
  return AlnTileAt{AS_NONE, 0, 0};
}

// item k of the blocks: block b from column s on with wb columns, line 0 / 1 / 2 (row 0, bars, row 1), place p in the line: 0 the label,
// 1 .. wb the columns, wb + 1 the line end
struct AlnBlockAt {
  uint32_t b, s, wb, line, p;
};
TR_HD AlnBlockAt aln_block_at(uint32_t k, uint32_t cols, uint32_t L) {
  const uint32_t per = 3u * (L + 2u);
  AlnBlockAt a;
  a.b = k / per;  // (the blocks in front of a short last one are all whole)
  const uint32_t r = k - a.b * per;
  a.s = a.b * L;
  a.wb = cols - a.s < L ? cols - a.s : L;
  a.line = r / (a.wb + 2u);
  a.p = r - a.line * (a.wb + 2u);
  return a;
}

struct AlnView {  // one alignment
  const uint8_t *r0, *r1, *nm0, *nm1;
  uint32_t cols, n0, n1, L, fald, key, ref_len;
  int32_t ref_pos, score;
  bool forward, mirrored;
};
TR_HD AlnShape aln_shape(const AlnArgs& a, const AlnDesc& d) { return AlnShape{a.form, a.linelimit, d.cols, d.name0_len, d.name1_len}; }
TR_HD AlnView aln_view(const AlnArgs& a, const AlnDesc& d) {
  AlnView v;
  v.r0 = a.rows0 + d.rows_off; v.r1 = a.rows1 + d.rows_off;
  v.nm0 = a.names + d.name0_off; v.nm1 = a.names + d.name1_off;
  v.cols = d.cols; v.n0 = d.name0_len; v.n1 = d.name1_len;
  v.L = a.linelimit; v.fald = a.linelimit + 14u; v.key = a.key; v.ref_len = d.ref_len;
  v.ref_pos = d.ref_pos; v.score = d.score;
  v.forward = (d.flags & kAlnForward) != 0;
  v.mirrored = a.form == kAlnPlot && !v.forward && a.key != 3;
  return v;
}

#define TRACYHIP_ALN_LIT(s, text) (s).lit(text, (uint32_t)sizeof(text) - 1u)

// `x` right-aligned in `w` places, never cut (std::setw)
template <class Sink>
TR_HD void aln_setw(Sink& s, uint32_t x, uint32_t w) {
  for (uint32_t d = render_digits(x); d < w; ++d) s.ch(' ');
  s.num((int32_t)x);  // (below 2^31: aln_answerable)
}
template <class Sink>
TR_HD void aln_rule(Sink& s, uint32_t r, uint32_t fald) {  // place r of '#', fald - 1 dashes, '\n'
  s.ch(r == 0 ? '#' : r == fald ? '\n' : '-');
}

// item i of section `sec` into sink s.  An ungapped row: aux0 = the letters of that row in front of column i; a label of the blocks:
// aux0 / aux1 = the letters of row 0 / row 1 in front of the block
template <class Sink>
TR_HD void alntext_item(const AlnView& v, AlnSection sec, uint32_t i, uint32_t aux0, uint32_t aux1, Sink& s) {
  switch (sec) {
    case AS_NAME0: s.ch(i < v.n0 ? v.nm0[i] : (uint8_t)'\n'); return;
    case AS_NAME1: s.ch(i < v.n1 ? v.nm1[i] : (uint8_t)'\n'); return;
    case AS_UNG0:
    case AS_UNG1: {
      if (i == v.cols) {
        if (aux0 % v.fald != 0) s.ch('\n');
        return;
      }
      const uint8_t c = sec == AS_UNG0 ? v.r0[i] : v.r1[i];
      if (c == '-') return;
      s.ch(c);
      if ((aux0 + 1u) % v.fald == 0) s.ch('\n');
      return;
    }
    case AS_MIDRULE:
      if (i == 0) {
        TRACYHIP_ALN_LIT(s, "\nAlignment score: ");
        s.num(v.score);
        s.ch('\n');
      } else if (i <= v.fald + 1u) aln_rule(s, i - 1u, v.fald);
      else s.ch('\n');
      return;
    case AS_BLOCKS: {
      const AlnBlockAt at = aln_block_at(i, v.cols, v.L);
      if (at.p == 0) {
        if (at.line == 1) { TRACYHIP_ALN_LIT(s, "              "); return; }
        if (at.line == 0) {
          if (v.key != 3) { TRACYHIP_ALN_LIT(s, "Alt"); aln_setw(s, 1u + aux0, 10); }
          else { TRACYHIP_ALN_LIT(s, "Alt1"); aln_setw(s, 1u + aux0, 9); }
        } else {
          const uint32_t ri = (uint32_t)v.ref_pos + 1u + aux1;
          if (v.key == 3) { TRACYHIP_ALN_LIT(s, "Alt2"); aln_setw(s, ri, 9); }
          else {
            TRACYHIP_ALN_LIT(s, "Ref");
            // mirrored: pos + size - (ri - pos) + 1; the check tile has seen aux1 <= ref_len
            aln_setw(s, v.forward ? ri : (uint32_t)v.ref_pos + v.ref_len - aux1, 10);
          }
        }
        s.ch(' ');
        return;
      }
      if (at.p == at.wb + 1u) {
        s.ch('\n');
        if (at.line == 2) s.ch('\n');
        return;
      }
      const uint32_t j = at.s + at.p - 1u;
      if (at.line == 0) s.ch(v.r0[j]);
      else if (at.line == 2) s.ch(v.r1[j]);
      else s.ch(v.r0[j] == v.r1[j] ? '|' : ' ');
      return;
    }
    case AS_TAIL: {
      if (i == 0) {
        const uint32_t blocks = aln_nblocks(v.cols, v.L);
        for (uint32_t k = blocks < 6 ? 4u * (6u - blocks) : 0u; k > 0; --k) s.ch('\n');
        return;
      }
      if (i == 2u * v.fald + 3u) { TRACYHIP_ALN_LIT(s, "\n\n"); return; }
      const uint32_t r = i - 1u;
      aln_rule(s, r <= v.fald ? r : r - (v.fald + 1u), v.fald);
      return;
    }
    case AS_FNAME0:
      s.ch(i == 0 ? (uint8_t)'>' : i <= v.n0 ? v.nm0[i - 1] : (uint8_t)'\n');
      return;
    case AS_FNAME1:
      if (i == 0) s.ch('>');
      else if (i <= v.n1) s.ch(v.nm1[i - 1]);
      else if (v.forward) TRACYHIP_ALN_LIT(s, " (forward)\n");
      else TRACYHIP_ALN_LIT(s, " (reverse)\n");
      return;
    case AS_FROW0: s.ch(i < v.cols ? v.r0[i] : (uint8_t)'\n'); return;
    case AS_FROW1: s.ch(i < v.cols ? v.r1[i] : (uint8_t)'\n'); return;
    case AS_JHEAD:
      if (i == 0) TRACYHIP_ALN_LIT(s, ",\n\"refchr\": \"");
      else if (i <= v.n1) s.ch(v.nm1[i - 1]);
      else {
        TRACYHIP_ALN_LIT(s, "\",\n\"refpos\": ");
        s.num((int32_t)((uint32_t)v.ref_pos + 1u));
        TRACYHIP_ALN_LIT(s, ",\n\"altalign\": \"");
      }
      return;
    case AS_JROW0:
      if (i < v.cols) s.ch(v.r0[i]);
      else TRACYHIP_ALN_LIT(s, "\",\n\"refalign\": \"");
      return;
    case AS_JROW1:
      if (i < v.cols) s.ch(v.r1[i]);
      else {
        TRACYHIP_ALN_LIT(s, "\",\n\"forward\": ");
        s.ch(v.forward ? '1' : '0');
        TRACYHIP_ALN_LIT(s, "\n}\n");
      }
      return;
    default: return;
  }
}

// the alignment that owns tile `tile`: the last one whose tile_first is <= tile among those that own a tile (tile_first does not fall)
TR_HD uint32_t aln_owner_of(const AlnDesc* al, uint32_t n, uint32_t tile) {
  uint32_t lo = 0, hi = n;  // first alignment whose tile_first is > tile
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (al[mid].tile_first <= tile) lo = mid + 1; else hi = mid;
  }
  return lo - 1;  // (alignments without a tile share the tile_first of the next one and sit below it: lo - 1 is the owner)
}

// The letters of both rows in front of column `col`; it only moves forward.  Every member is called by the whole wave.
struct AlnTileState {
  uint32_t col = 0, n0 = 0, n1 = 0;
  // the anchor of a tile: the first column its items may ask about
  TR_HD static uint32_t anchor(const AlnView& v, const AlnTileAt& at) {
    if (at.sec == AS_UNG0 || at.sec == AS_UNG1) return at.i0;
    if (at.sec == AS_BLOCKS) return aln_block_at(at.i0, v.cols, v.L).s;
    return 0;
  }
  template <class W>
  TR_HD void advance(W& w, const AlnView& v, uint32_t target) {  // target <= cols, the same in every lane
    const uint32_t lane = w.lane();
    while (col < target) {
      const uint32_t j = col + lane;
      const bool in = j < target;
      n0 += (uint32_t)__builtin_popcountll(w.ballot(in && v.r0[j] != '-'));
      n1 += (uint32_t)__builtin_popcountll(w.ballot(in && v.r1[j] != '-'));
      col = target - col < 64 ? target : col + 64;
    }
  }
  // from nothing to column `target`: the column tiles in front of it (col_letters of this alignment), then the steps inside one
  template <class W>
  TR_HD void seek(W& w, const AlnView& v, const uint32_t* col_letters, uint32_t target) {
    const uint32_t lane = w.lane(), whole = target / kAlnTile;
    uint32_t s0 = 0, s1 = 0;
    for (uint32_t k = lane; k < whole; k += 64) { s0 += col_letters[2 * k]; s1 += col_letters[2 * k + 1]; }
    n0 = w.sum(s0); n1 = w.sum(s1);
    col = whole * kAlnTile;
    advance(w, v, target);
  }
  // aux0 / aux1 of item i of this step (the steps of a tile in order)
  template <class W>
  TR_HD void aux(W& w, const AlnView& v, const AlnTileAt& at, uint32_t i, bool valid, uint32_t& aux0, uint32_t& aux1) {
    const uint32_t lane = w.lane();
    aux0 = aux1 = 0;
    if (at.sec == AS_UNG0 || at.sec == AS_UNG1) {
      const uint8_t* row = at.sec == AS_UNG0 ? v.r0 : v.r1;
      const uint64_t m = w.ballot(valid && i < v.cols && row[i] != '-');
      uint32_t& own = at.sec == AS_UNG0 ? n0 : n1;
      aux0 = own + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      own += (uint32_t)__builtin_popcountll(m);
    } else if (at.sec == AS_BLOCKS) {
      AlnBlockAt b{};
      if (valid) b = aln_block_at(i, v.cols, v.L);
      uint64_t labels = w.ballot(valid && b.p == 0 && b.line != 1);  // in the order of the lanes their blocks do not fall
      while (labels) {
        const uint32_t l = (uint32_t)__builtin_ctzll(labels);
        advance(w, v, w.bcast(b.s, l));
        if (lane == l) { aux0 = n0; aux1 = n1; }
        labels &= labels - 1;
      }
    }
  }
};

// the alignment that owns column tile `ct` (PLOT): as aln_owner_of over col_first
TR_HD uint32_t aln_col_owner_of(const AlnDesc* al, uint32_t n, uint32_t ct) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (al[mid].col_first <= ct) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// ---- launch 1 (PLOT): one wave per column tile ----
template <class W>
TR_HD void alntext_letters_body(W& w, const AlnArgs& a, uint32_t ct) {
  const AlnDesc d = a.al[aln_col_owner_of(a.al, a.n, ct)];
  const AlnView v = aln_view(a, d);
  const uint32_t c0 = (ct - d.col_first) * kAlnTile;
  AlnTileState st;
  st.col = c0;
  st.advance(w, v, v.cols - c0 < kAlnTile ? v.cols : c0 + kAlnTile);
  if (w.lane() == 0) { a.col_letters[2 * ct] = st.n0; a.col_letters[2 * ct + 1] = st.n1; }
}

// ---- launch 2: one wave per tile ----
template <class W>
TR_HD void alntext_count_body(W& w, const AlnArgs& a, uint32_t tile) {
  const uint32_t lane = w.lane();
  const uint32_t t = aln_owner_of(a.al, a.n, tile);
  const AlnDesc d = a.al[t];
  const AlnView v = aln_view(a, d);
  const AlnTileAt at = aln_locate(aln_shape(a, d), tile - d.tile_first);
  AlnTileState st;
  if (at.sec == AS_CHECK) {
    if (v.mirrored) st.seek(w, v, a.col_letters + 2 * (size_t)d.col_first, v.cols);
    if (lane == 0) { a.tile_bytes[tile] = 0; a.tile_aux[2 * tile] = st.n1 > v.ref_len ? 1u : 0u; a.tile_aux[2 * tile + 1] = 0; }
    return;
  }
  if (a.form == kAlnPlot) st.seek(w, v, a.col_letters + 2 * (size_t)d.col_first, AlnTileState::anchor(v, at));
  const uint32_t front0 = st.n0, front1 = st.n1;
  uint32_t bytes = 0;
  for (uint32_t i0 = at.i0; i0 < at.i1; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool valid = i < at.i1;
    uint32_t aux0, aux1;
    st.aux(w, v, at, i, valid, aux0, aux1);
    RenderCount c;
    if (valid) alntext_item(v, at.sec, i, aux0, aux1, c);
    bytes += c.n;
  }
  bytes = w.sum(bytes);
  if (lane == 0) { a.tile_bytes[tile] = bytes; a.tile_aux[2 * tile] = front0; a.tile_aux[2 * tile + 1] = front1; }
}

// ---- launch 3: one wave per alignment ----
template <class W>
TR_HD void alntext_scan_body(W& w, const AlnArgs& a, uint32_t t) {
  const uint32_t lane = w.lane();
  const AlnDesc d = a.al[t];
  if (!(d.flags & kAlnAnswerable)) {  // (the whole wave)
    if (lane == 0) a.out[t] = AlnOut{kAlnStatusDeferred, 0};
    return;
  }
  const uint32_t tiles = aln_tiles(aln_shape(a, d));
  const bool bad = a.tile_aux[2 * d.tile_first] != 0;  // (the check tile is the first)
  uint32_t total = 0;  // (below 2^31: alntext_bound)
  for (uint32_t k0 = 0; k0 < tiles; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool in = k < tiles;
    const uint32_t b = in ? a.tile_bytes[d.tile_first + k] : 0u;
    const uint32_t before = total + w.excl_sum(b);
    if (in) a.tile_bytes[d.tile_first + k] = before;
    total += w.sum(b);
  }
  if (bad) {
    if (lane == 0) a.out[t] = AlnOut{kAlnStatusDeferred, 0};
    return;
  }
  const bool small = a.text != nullptr && (uint64_t)total > d.text_cap;
  if (lane == 0) a.out[t] = AlnOut{small ? kAlnStatusTooSmall : kAlnStatusOk, total};
}

// ---- launch 4: one wave per tile ----
template <class W>
TR_HD void alntext_emit_body(W& w, const AlnArgs& a, uint32_t tile) {
  const uint32_t lane = w.lane();
  const uint32_t t = aln_owner_of(a.al, a.n, tile);
  if (a.out[t].status != kAlnStatusOk) return;  // (the whole wave)
  const AlnDesc d = a.al[t];
  const AlnView v = aln_view(a, d);
  const AlnTileAt at = aln_locate(aln_shape(a, d), tile - d.tile_first);
  if (at.sec == AS_CHECK) return;
  uint8_t* img = reinterpret_cast<uint8_t*>(w.lds());
  uint8_t* dst = a.text + d.text_off + a.tile_bytes[tile];
  uint32_t lo = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u), hi = lo;
  uint8_t* base = dst - lo;
  AlnTileState st;
  st.col = AlnTileState::anchor(v, at); st.n0 = a.tile_aux[2 * tile]; st.n1 = a.tile_aux[2 * tile + 1];
  for (uint32_t i0 = at.i0; i0 < at.i1; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool valid = i < at.i1;
    uint32_t aux0, aux1;
    st.aux(w, v, at, i, valid, aux0, aux1);
    RenderCount c;
    if (valid) alntext_item(v, at.sec, i, aux0, aux1, c);
    const uint32_t off = w.excl_sum(c.n), step = w.sum(c.n);
    if (valid) {
      RenderWrite wr{img + hi + off};
      alntext_item(v, at.sec, i, aux0, aux1, wr);
    }
    hi += step;
    w.sync();
    render_flush(w, img, base, lo, hi, i0 + 64 >= at.i1);
  }
}

// ---- tracyhip_reference_slices: one wave per tile of kSliceTile output bytes ----
constexpr uint32_t kSliceTile = 1024;
struct SliceDesc {  // per slice, built by the host (alntext_plan.h)
  uint64_t ref_off, out_off;
  uint32_t ref_len, begin, len;
  uint32_t tile_first;  // of the launch's tiles; the slice owns ceil(len / kSliceTile) of them
  uint32_t forward, pad_;
};
struct SliceArgs {
  const uint8_t* refs;
  uint8_t* out;
  const SliceDesc* sl;
  uint32_t n, ntiles;
};
// reverseComplement's byte rule (fmindex.h:11-25): 0 = not a letter it complements
TR_HD uint8_t slice_complement(uint8_t c) {
  switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    case 'N': case 'n': return 'N';
    default: return 0;
  }
}
TR_HD uint32_t slice_owner_of(const SliceDesc* sl, uint32_t n, uint32_t tile) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sl[mid].tile_first <= tile) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}
template <class W>
TR_HD void slice_body(W& w, const SliceArgs& a, uint32_t tile) {
  const uint32_t lane = w.lane();
  const SliceDesc d = a.sl[slice_owner_of(a.sl, a.n, tile)];
  const uint8_t* ref = a.refs + d.ref_off;
  uint8_t* out = a.out + d.out_off;
  const uint32_t j0 = (tile - d.tile_first) * kSliceTile;
  const uint32_t j1 = d.len - j0 < kSliceTile ? d.len : j0 + kSliceTile;
  for (uint32_t j = j0 + lane; j < j1; j += 64) {
    const uint32_t k = d.begin + j;  // place in the oriented reference (begin + len <= ref_len: the host has looked)
    uint8_t c = ref[k];
    if (!d.forward) {
      const uint8_t m = slice_complement(ref[d.ref_len - 1u - k]);
      if (m) c = m;  // (any other letter: the place keeps the byte the reference has there)
    }
    out[j] = c;
  }
}

}  // namespace tracyhip
#endif
