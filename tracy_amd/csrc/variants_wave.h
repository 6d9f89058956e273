// variants_wave.h -- the variant calling of `tracy decompose -v` for ONE trace on ONE wave, equal to tracy_amd/host/indigo_out.hpp:
//   var_scan    callVariants of one two-row alignment     variants.h:56-126
//   var_merge   insertVariant across the two alleles      variants.h:34-53
//   var_sort    std::sort(var) with the ties defined      indigo.h:442, Variant::operator<
//   call_index  variantCallIndex                          variants.h:205
// variants_wave runs the four over the two allele alignments of a trace and writes its sorted tracyhip_variant list and their text.
//
// The scan walks the columns in rounds of 64, one column per lane; every read of a row is one coalesced 64-byte access.  With
// a(j) = row0[j] != '-' and b(j) = row1[j] != '-' inside [viStart, viEnd], everything the reference carries from column to column is
// a prefix count or a "last column before j" of the ballots A and B of a round plus what the rounds before left:
//   vi, ri      counts of a / b columns up to j (the reference's values after its two ++)
//   la, lb      the last a / b column before j: the highest bit of A / B below the lane, else the carried one (a max-scan)
//   a deletion  closes at an a column with b columns in (la, j): they are its characters, ri at la its position, the last b column
//               at or before la its anchor
//   an insertion closes at a b column with a columns in (lb, j): they are its characters, lb its anchor, ri before j its position
// A run still open behind viEnd is never emitted (the reference does not flush).  Events whose ref holds N / n or whose pos <= 0
// are dropped where they would be pushed.  Events leave in column order, a closing run before the SNV of its column.
//
// W: the wave abstraction of decompose_wave.h (lane, ballot, bcast, excl_sum, sync); tests/emu/emu_variants.cpp runs the same text on
// the 64-fiber host wave.  The per-allele event lists live in memory the caller hands in (2 x max_variants VarEvent), written by
// one lane and read by another across w.sync().
#ifndef TRACY_AMD_VARIANTS_WAVE_H
#define TRACY_AMD_VARIANTS_WAVE_H

#include <cstdint>

#include "../../include/tracy_hip.h"
#include "dp_lane.h"  // TR_HD

namespace tracyhip {

// one event of one allele between the scan and the text
struct VarEvent {
  int32_t pos, basenum;
  uint32_t ref_len, alt_len;  // (1, 1) SNV; (1 + n, 1) deletion; (1, 1 + n) insertion
  int32_t anchor;             // run: the anchor's column in row1
  uint32_t src, end;          // SNV: its column in src; run: its characters are the non-gap bytes of the columns in (src, end) of row1 (deletion) / row0 (insertion)
  uint32_t gt;                // 1; 2 once the other allele has brought the same (pos, ref, alt).  Allele 2: 0 = merged into allele 1's event
};
static_assert(sizeof(VarEvent) == 32, "VarEvent is laid out for two 16-byte accesses");

// the two allele alignments of a trace and what call_index reads
struct VarTrace {
  const uint8_t* row0[2];  // the allele
  const uint8_t* row1[2];  // the reference slice
  uint32_t len[2];
  int32_t pos0[2];         // rs.pos
  uint32_t forward, bc_len;
};

TR_HD uint32_t var_popc(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
TR_HD uint32_t var_high(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }  // x != 0
TR_HD uint64_t var_upto(uint32_t bit) { return bit >= 63u ? ~0ull : (2ull << bit) - 1ull; }  // bits 0 .. bit
TR_HD bool var_is_n(uint8_t c) { return c == 'N' || c == 'n'; }

// callVariants of one alignment: the kept events in push order into ev[0 .. cap); returns how many there are (more than cap: the
// rest was not written).  Every lane returns the count.
template <class W>
TR_HD uint32_t var_scan_wave(W& w, const uint8_t* row0, const uint8_t* row1, uint32_t L, int32_t pos0, VarEvent* ev, uint32_t cap) {
  const uint32_t lane = w.lane();
  const uint64_t below = (1ull << lane) - 1ull, upto = var_upto(lane);
  // viStart, viEnd and ri at viStart (variants.h:60-68)
  int32_t vs = -1, ve = -1, ri0 = pos0;
  for (uint32_t b = 0; b < L; b += 64) {
    const uint32_t j = b + lane;
    const uint64_t A = w.ballot(j < L && row0[j] != '-');
    if (vs < 0) {
      const uint64_t B = w.ballot(j < L && row1[j] != '-');
      if (A) {
        const uint32_t f = (uint32_t)__builtin_ctzll(A);
        vs = (int32_t)(b + f);
        ri0 += (int32_t)var_popc(B & ((1ull << f) - 1ull));
      } else {
        ri0 += (int32_t)var_popc(B);
      }
    }
    if (A) ve = (int32_t)(b + var_high(A));
  }
  if (vs < 0) return 0;
  // carried from round to round (wave-uniform)
  int32_t vi_c = 0, ri_c = ri0, nn_c = 0;            // counts of a columns, b columns (from pos0 on) and b columns that hold N / n
  int32_t la_c = -1, ri_la_c = ri0, nn_la_c = 0;     // the last a column, and ri / the N count there
  int32_t lb_la_c = -1;                              // the last b column at or before la_c
  int32_t lb_c = -1, vi_lb_c = 0;                    // the last b column, and vi there
  uint32_t n = 0;
  for (uint32_t b = (uint32_t)vs & ~63u; b <= (uint32_t)ve; b += 64) {
    const uint32_t j = b + lane;
    const bool in = j >= (uint32_t)vs && j <= (uint32_t)ve;
    const uint8_t c0 = in ? row0[j] : (uint8_t)'-', c1 = in ? row1[j] : (uint8_t)'-';
    const bool a = c0 != '-', bb = c1 != '-', isn = bb && var_is_n(c1);
    const uint64_t A = w.ballot(a), B = w.ballot(bb), NN = w.ballot(isn);
    const int32_t vi = vi_c + (int32_t)var_popc(A & upto), ri = ri_c + (int32_t)var_popc(B & upto), nn = nn_c + (int32_t)var_popc(NN & upto);
    const int32_t vi_before = vi - (a ? 1 : 0), ri_before = ri - (bb ? 1 : 0), nn_before = nn - (isn ? 1 : 0);
    int32_t la = la_c, ri_la = ri_la_c, nn_la = nn_la_c, lb_la = lb_la_c;
    if (A & below) {
      const uint32_t h = var_high(A & below);
      const uint64_t m = var_upto(h);
      la = (int32_t)(b + h);
      ri_la = ri_c + (int32_t)var_popc(B & m);
      nn_la = nn_c + (int32_t)var_popc(NN & m);
      lb_la = (B & m) ? (int32_t)(b + var_high(B & m)) : lb_c;
    }
    int32_t lb = lb_c, vi_lb = vi_lb_c;
    if (B & below) {
      const uint32_t h = var_high(B & below);
      lb = (int32_t)(b + h);
      vi_lb = vi_c + (int32_t)var_popc(A & var_upto(h));
    }
    // the run that closes here (at most one: a deletion needs b columns behind the last a column, an insertion the reverse)
    VarEvent run{}, snv{};
    bool has_run = false, has_snv = false;
    if (a && ri_before - ri_la > 0) {  // deletion, variants.h:80-87
      const uint8_t anc = lb_la >= 0 ? row1[lb_la] : (uint8_t)'N';
      run = VarEvent{ri_la, vi_before, 1u + (uint32_t)(ri_before - ri_la), 1u, lb_la, (uint32_t)la, j, 1u};
      has_run = run.pos > 0 && !var_is_n(anc) && nn_before == nn_la;
    } else if (bb && vi_before - vi_lb > 0) {  // insertion, variants.h:88-97
      const uint8_t anc = lb >= 0 ? row1[lb] : (uint8_t)'N';
      run = VarEvent{ri_before, vi_before, 1u, 1u + (uint32_t)(vi_before - vi_lb), lb, (uint32_t)lb, j, 1u};
      has_run = run.pos > 0 && !var_is_n(anc);
    }
    if (a && bb && c0 != c1) {  // SNV, variants.h:102-104
      snv = VarEvent{ri, vi, 1u, 1u, (int32_t)j, j, j, 1u};
      has_snv = snv.pos > 0 && !isn;
    }
    const uint64_t R = w.ballot(has_run), S = w.ballot(has_snv);
    uint32_t slot = n + var_popc(R & below) + var_popc(S & below);
    if (has_run) {
      if (slot < cap) ev[slot] = run;
      ++slot;
    }
    if (has_snv && slot < cap) ev[slot] = snv;
    n += var_popc(R) + var_popc(S);
    if (A) {
      const uint32_t h = var_high(A);
      const uint64_t m = var_upto(h);
      la_c = (int32_t)(b + h);
      ri_la_c = ri_c + (int32_t)var_popc(B & m);
      nn_la_c = nn_c + (int32_t)var_popc(NN & m);
      lb_la_c = (B & m) ? (int32_t)(b + var_high(B & m)) : lb_c;
    }
    if (B) {
      const uint32_t h = var_high(B);
      lb_c = (int32_t)(b + h);
      vi_lb_c = vi_c + (int32_t)var_popc(A & var_upto(h));
    }
    vi_c += (int32_t)var_popc(A);
    ri_c += (int32_t)var_popc(B);
    nn_c += (int32_t)var_popc(NN);
  }
  return n;
}

// k-th non-gap byte behind column `at` of a row (a run's characters; alignments built from op strings have no gap-gap columns and
// the walk is one step per character)
TR_HD uint8_t var_next_char(const uint8_t* row, uint32_t& at) {
  do ++at; while (row[at] == '-');
  return row[at];
}

// insertVariant's test: the same pos, ref and alt (events of two alignments; lengths equal means the same kind)
TR_HD bool var_same(const VarEvent& x, const uint8_t* x0, const uint8_t* x1, const VarEvent& y, const uint8_t* y0, const uint8_t* y1) {
  if (x.pos != y.pos || x.ref_len != y.ref_len || x.alt_len != y.alt_len) return false;
  if (x.ref_len == 1 && x.alt_len == 1) return x1[x.src] == y1[y.src] && x0[x.src] == y0[y.src];
  if (x1[x.anchor] != y1[y.anchor]) return false;
  const bool del = x.ref_len > 1;
  const uint8_t *xr = del ? x1 : x0, *yr = del ? y1 : y0;
  uint32_t xa = x.src, ya = y.src;
  for (uint32_t k = (del ? x.ref_len : x.alt_len) - 1u; k > 0; --k)
    if (var_next_char(xr, xa) != var_next_char(yr, ya)) return false;
  return true;
}

TR_HD bool var_key_less(const VarEvent& x, const VarEvent& y) { return x.pos < y.pos || (x.pos == y.pos && x.basenum < y.basenum); }
TR_HD bool var_key_equal(const VarEvent& x, const VarEvent& y) { return x.pos == y.pos && x.basenum == y.basenum; }

// The variants of one trace.  ev: 2 x max_variants events of scratch; var: max_variants records; text: max_text bytes.  Record r's
// ref is text[ref_off .. + ref_len), its alt text[alt_off .. + alt_len), packed in record order, ref first.  A trace whose events do
// not fit (either allele's list, the merged list, the text) leaves *var_n = 0 and *var_flags = 1 and writes no record and no text.
template <class W>
TR_HD void variants_wave(W& w, const VarTrace& t, uint32_t trim_left, uint32_t trim_right, uint32_t max_variants, uint32_t max_text, VarEvent* ev,
                         tracyhip_variant* var, uint8_t* text, uint32_t* var_n, uint32_t* var_flags) {
  const uint32_t lane = w.lane();
  const uint64_t below = (1ull << lane) - 1ull;
  VarEvent *e1 = ev, *e2 = ev + max_variants;
  const uint32_t n1 = var_scan_wave(w, t.row0[0], t.row1[0], t.len[0], t.pos0[0], e1, max_variants);
  const uint32_t n2 = var_scan_wave(w, t.row0[1], t.row1[1], t.len[1], t.pos0[1], e2, max_variants);
  bool overflow = n1 > max_variants || n2 > max_variants;
  w.sync();
  // var_merge: allele 2's event with an equal in allele 1 adds to that one's gt and leaves (within an allele no two events are equal:
  // at most one partner, and nobody else writes it)
  uint32_t kept2 = 0;
  if (!overflow) {
    for (uint32_t b = 0; b < n2; b += 64) {
      const uint32_t i = b + lane;
      bool keep = i < n2;
      if (keep) {
        const VarEvent y = e2[i];
        for (uint32_t k = 0; k < n1; ++k)
          if (e1[k].pos == y.pos && var_same(e1[k], t.row0[0], t.row1[0], y, t.row0[1], t.row1[1])) {
            e1[k].gt = 2;
            e2[i].gt = 0;
            keep = false;
            break;
          }
      }
      kept2 += var_popc(w.ballot(keep));
    }
    overflow = n1 + kept2 > max_variants;
  }
  w.sync();
  const uint32_t m = n1 + kept2;
  // the text all records need, before anything is written
  if (!overflow) {
    uint32_t bytes = 0;
    for (uint32_t i = lane; i < n1 + n2; i += 64) {
      const VarEvent& x = i < n1 ? e1[i] : e2[i - n1];
      if (x.gt) bytes += x.ref_len + x.alt_len;
    }
    const uint32_t before = w.excl_sum(bytes);
    overflow = w.bcast(before + bytes, 63) > max_text;  // (a trace's events hold fewer than 2^31 characters: two rows of uint32 columns)
  }
  if (overflow) {
    if (lane == 0) { *var_n = 0; *var_flags = 1; }
    w.sync();
    return;
  }
  // var_sort: the rank of an event is the number of events before it by (pos, basenum), ties in merge order (allele 1 first, each
  // allele in push order).  The record goes to its rank with the event's index in ref_off until the text is laid out.
  for (uint32_t i = lane; i < n1 + n2; i += 64) {
    const bool second = i >= n1;
    const uint32_t own = second ? i - n1 : i;
    const VarEvent x = second ? e2[own] : e1[own];
    if (!x.gt) continue;
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n1; ++k) rank += (var_key_less(e1[k], x) || (var_key_equal(e1[k], x) && (second || k < own))) ? 1u : 0u;
    for (uint32_t k = 0; k < n2; ++k) rank += (e2[k].gt && (var_key_less(e2[k], x) || (var_key_equal(e2[k], x) && second && k < own))) ? 1u : 0u;
    const uint32_t call = t.forward ? trim_left + (uint32_t)x.basenum - 1u : t.bc_len - (trim_right + (uint32_t)x.basenum);
    var[rank] = tracyhip_variant{x.pos, x.basenum, (int32_t)x.gt, call, i, x.ref_len, 0u, x.alt_len};
  }
  w.sync();
  // offsets in record order, then the characters: an SNV by its lane, a run by the whole wave (its columns in rounds of 64)
  uint32_t text_at = 0;
  for (uint32_t b = 0; b < m; b += 64) {
    const uint32_t r = b + lane;
    tracyhip_variant v{};
    VarEvent x{};
    bool second = false;
    if (r < m) {
      v = var[r];
      second = v.ref_off >= n1;
      x = second ? e2[v.ref_off - n1] : e1[v.ref_off];
    }
    const uint32_t bytes = v.ref_len + v.alt_len;
    const uint32_t off = text_at + w.excl_sum(bytes);
    text_at = w.bcast(off + bytes, 63);
    const bool is_run = r < m && bytes > 2;
    if (r < m) {
      v.ref_off = off;
      v.alt_off = off + v.ref_len;
      var[r] = v;
      const uint8_t *r0 = t.row0[second ? 1 : 0], *r1 = t.row1[second ? 1 : 0];
      if (is_run) {
        text[v.ref_off] = r1[x.anchor];
        text[v.alt_off] = r1[x.anchor];
      } else {
        text[v.ref_off] = r1[x.src];
        text[v.alt_off] = r0[x.src];
      }
    }
    for (uint64_t runs = w.ballot(is_run); runs; runs &= runs - 1) {
      const uint32_t src_lane = (uint32_t)__builtin_ctzll(runs);
      const uint32_t lo = w.bcast(x.src, src_lane), hi = w.bcast(x.end, src_lane);
      const uint32_t del = w.bcast(v.ref_len > 1 ? 1u : 0u, src_lane), sec = w.bcast(second ? 1u : 0u, src_lane);
      uint32_t dst = w.bcast((v.ref_len > 1 ? v.ref_off : v.alt_off) + 1u, src_lane);
      const uint8_t* row = del ? t.row1[sec] : t.row0[sec];
      for (uint32_t c = lo + 1; c < hi; c += 64) {
        const uint32_t col = c + lane;
        const bool take = col < hi && row[col] != '-';
        const uint64_t T = w.ballot(take);
        if (take) text[dst + var_popc(T & below)] = row[col];
        dst += var_popc(T);
      }
    }
  }
  if (lane == 0) { *var_n = m; *var_flags = 0; }
  w.sync();
}

}  // namespace tracyhip
#endif
