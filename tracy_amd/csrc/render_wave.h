// render_wave.h -- the text of ONE tile of one trace on ONE wave: traceTxtOut (abif.h:513-533), _traceJsonOut (json.h:33-105) and
// assemblyTrace (json.h:120-194), byte for byte what tracy_amd/host prints (trace_io.hpp, indigo_out.hpp traceJsonBody, sage_out.hpp
// assemblyTrace) for every trace it answers.
//
// A trace's text is a sequence of SECTIONS, a section a sequence of ITEMS, and an item the bytes one `out << ...` run of the reference
// produces for one sample or one call; the opening of a section belongs to its first item, the closing to its last:
//     TSV     header line | one line per sample
//     JSON    "pos" | "peakA" .. "peakT" | "basecallPos" | "basecallQual" | "basecalls" | "primarySeq" | "secondarySeq"
//     GAPPED  "peakA" .. "peakT" | "basecallPos" | "basecallQual" | "basecalls" (gapless counter, raw secondary)
// In front of them every form has a section of no bytes over the calls that CHECKS the positions.  A TILE is kRenderTile consecutive
// items of one section; tiles are numbered through the sections of a trace (render_locate) and through the traces of a launch
// (RenderTrace::tile_first).  Because the positions of an answered trace are strictly increasing inside [0, nsamples), the reference's
// cursor loop visits every call, in order: a call section is a list over the calls with ", " in front of all but the first.
//
// Three bodies, one wave each:
//     render_count_body   per tile: the bytes of its items (the same render_item text as the emit pass, into a counting sink), summed;
//                         a check tile: "some position is bad".  A GAPPED "basecalls" tile also leaves the number of non-'-' primaries
//                         in front of it, which its digits depend on.
//     render_scan_body    per trace: the exclusive sum over its tiles in place (tile offsets), text_len and the status
//     render_emit_body    per tile: 64 items at a time, a lane measures its item, excl_sum places it in the wave's LDS, the lane writes
//                         it there; the LDS image is kept congruent to the destination modulo 16, so whole 16-byte words leave as one
//                         store each and only the head and the tail of a tile leave byte-wise.  Every byte of the text is written
//                         exactly once, by the tile that owns it; no atomics.
// A sample line of the TSV finds its call through a table in LDS: one binary search of bcpos per tile for the first call at or behind
// the tile's first sample, then the (at most kRenderTile) calls of the tile enter their slot.
//
// Answered: bc_len in 1 .. kRenderMaxCalls, nsamples in 1 .. kRenderMaxSamples, positions strictly increasing inside [0, nsamples).
// The text of such a trace stays below 2^31 bytes (render_plan.h render_bound).  Anything else is DEFERRED: status and text_len 0.
// No read depends on a position: positions are printed, compared and searched, never used as an index without a range test.
//
// W: the wave of dev_wave.h (lane, ballot, bcast, sum, excl_sum, sync, lds).
#ifndef TRACY_AMD_RENDER_WAVE_H
#define TRACY_AMD_RENDER_WAVE_H

#include <cstdint>

#include "dp_lane.h"  // TR_HD

namespace tracyhip {

constexpr int32_t kRenderStatusOk = 0, kRenderStatusDeferred = 1, kRenderStatusTooSmall = 2;  // TRACYHIP_RENDER_*
constexpr uint32_t kRenderTsv = 0, kRenderJson = 1, kRenderGapped = 2;                        // TRACYHIP_RENDER_TSV / JSON / GAPPED
constexpr uint32_t kRenderMaxCalls = 131071;  // as pad and basecalling
constexpr uint32_t kRenderMaxSamples = 1u << 23;
constexpr uint32_t kRenderTile = 256;     // items per tile
constexpr uint32_t kRenderMaxItem = 80;   // bytes of the longest item: a TSV line of a called sample is 75 (render_plan.cpp tries the extremes)
constexpr uint32_t kRenderImage = 64 * kRenderMaxItem + 16;            // the LDS image: a step's items behind up to 15 bytes left over
constexpr uint32_t kRenderLdsBytes = kRenderImage + 2 * kRenderTile;  // + the call table of a TSV sample tile (uint16 each)

enum RenderSection : uint32_t {
  RS_CHECK, RS_HEADER, RS_SAMPLES, RS_POS, RS_PEAK_A, RS_PEAK_C, RS_PEAK_G, RS_PEAK_T, RS_BCPOS, RS_BCQUAL, RS_CALLS, RS_CALLS_GAPPED,
  RS_PRISEQ, RS_SECSEQ, RS_NONE
};

struct RenderTrace {  // per trace, built by the host (render_plan.h)
  uint64_t sig_off;   // elements
  uint64_t bc_off;    // elements: the five basecall arrays
  uint64_t text_off;  // bytes
  uint64_t text_cap;
  uint32_t nsamples, bc_len;
  uint32_t trim_l, trim_r;
  uint32_t tile_first;  // of the launch's tiles; the trace owns render_tiles() of them (none where the host can tell it is not answered)
  uint32_t answerable;
};
struct RenderOut {
  int32_t status;
  uint32_t text_len;
};
struct RenderArgs {
  const void* signal;
  const int32_t* bcpos;
  const uint8_t *primary, *secondary, *consensus, *estqual;
  const RenderTrace* tr;
  RenderOut* out;
  uint32_t* tile_bytes;  // per tile: its bytes (count), then its offset in the trace's text (scan)
  uint32_t* tile_aux;    // per tile: check tiles "a position is bad"; GAPPED call tiles the gapless count in front
  uint8_t* text;         // null: sizes only
  uint32_t ntraces, ntiles, form;
};

TR_HD bool render_answerable(uint32_t ns, uint32_t n) { return n >= 1 && n <= kRenderMaxCalls && ns >= 1 && ns <= kRenderMaxSamples; }
TR_HD uint32_t render_tiles_of(uint32_t items) { return (items + kRenderTile - 1) / kRenderTile; }

// the sections of a form in the order of the text, and the items of each
TR_HD uint32_t render_nsections(uint32_t form) { return form == kRenderTsv ? 3u : form == kRenderJson ? 11u : 8u; }
TR_HD RenderSection render_section(uint32_t form, uint32_t k) {
  if (k == 0) return RS_CHECK;
  if (form == kRenderTsv) return k == 1 ? RS_HEADER : RS_SAMPLES;
  if (form == kRenderJson) {
    const RenderSection s[11] = {RS_CHECK, RS_POS, RS_PEAK_A, RS_PEAK_C, RS_PEAK_G, RS_PEAK_T, RS_BCPOS, RS_BCQUAL, RS_CALLS, RS_PRISEQ, RS_SECSEQ};
    return s[k];
  }
  const RenderSection s[8] = {RS_CHECK, RS_PEAK_A, RS_PEAK_C, RS_PEAK_G, RS_PEAK_T, RS_BCPOS, RS_BCQUAL, RS_CALLS_GAPPED};
  return s[k];
}
TR_HD uint32_t render_items(RenderSection s, uint32_t ns, uint32_t n) {
  if (s == RS_HEADER) return 1;
  return (s == RS_SAMPLES || (s >= RS_POS && s <= RS_PEAK_T)) ? ns : n;
}
TR_HD uint32_t render_tiles(uint32_t form, uint32_t ns, uint32_t n) {
  uint32_t t = 0;
  for (uint32_t k = 0; k < render_nsections(form); ++k) t += render_tiles_of(render_items(render_section(form, k), ns, n));
  return t;
}
struct RenderTileAt {
  RenderSection sec;
  uint32_t i0, i1;  // items
};
TR_HD RenderTileAt render_locate(uint32_t form, uint32_t ns, uint32_t n, uint32_t tile) {
  for (uint32_t k = 0; k < render_nsections(form); ++k) {
    const RenderSection s = render_section(form, k);
    const uint32_t items = render_items(s, ns, n), tiles = render_tiles_of(items);
    if (tile < tiles) {
      const uint32_t i0 = tile * kRenderTile;
      return RenderTileAt{s, i0, items - i0 < kRenderTile ? items : i0 + kRenderTile};
    }
    tile -= tiles;
  }
  return RenderTileAt{RS_NONE, 0, 0};
}

TR_HD uint32_t render_digits(uint32_t v) {  // decimal digits of v, from comparisons
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
         (v >= 1000000000u);
}

// the two sinks of render_item: the byte count, and the bytes
struct RenderCount {
  uint32_t n = 0;
  TR_HD void ch(uint8_t) { n += 1; }
  TR_HD void lit(const char*, uint32_t len) { n += len; }
  TR_HD void num(int32_t x) {
    const uint32_t v = x < 0 ? 0u - (uint32_t)x : (uint32_t)x;  // (INT32_MIN: negated in unsigned arithmetic)
    n += render_digits(v) + (x < 0 ? 1u : 0u);
  }
};
struct RenderWrite {
  uint8_t* p;
  TR_HD void ch(uint8_t c) { *p++ = c; }
  TR_HD void lit(const char* s, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) p[i] = (uint8_t)s[i];
    p += len;
  }
  TR_HD void num(int32_t x) {
    uint32_t v = x < 0 ? 0u - (uint32_t)x : (uint32_t)x;
    if (x < 0) *p++ = '-';
    const uint32_t nd = render_digits(v);
    for (uint32_t d = nd; d-- > 0;) {
      const uint32_t q = v / 10u;  // (a multiply-high by a constant)
      p[d] = (uint8_t)('0' + (v - 10u * q));
      v = q;
    }
    p += nd;
  }
};

template <bool S16>
TR_HD int32_t render_load(const void* sig, uint64_t idx) {
  return S16 ? (int32_t) static_cast<const int16_t*>(sig)[idx] : static_cast<const int32_t*>(sig)[idx];
}

struct RenderView {  // one trace's arrays
  const void* signal;
  uint64_t sig_off;
  const int32_t* pos;
  const uint8_t *pri, *sec, *con, *q;
  uint32_t ns, n, trim_l, keep_until;
};

#define TRACYHIP_RENDER_LIT(s, text) (s).lit(text, (uint32_t)sizeof(text) - 1u)

// item i of section `sec` into sink s.  aux: RS_SAMPLES 1 + the call at this sample (0: none); RS_CALLS_GAPPED the gapless number
template <bool S16, class Sink>
TR_HD void render_item(const RenderView& v, RenderSection sec, uint32_t i, uint32_t aux, Sink& s) {
  switch (sec) {
    case RS_HEADER:
      TRACYHIP_RENDER_LIT(s, "pos\tpeakA\tpeakC\tpeakG\tpeakT\tbasenum\tprimary\tsecondary\tconsensus\tqual\ttrim\n");
      return;
    case RS_SAMPLES: {
      s.num((int32_t)(i + 1));
      s.ch('\t');
      for (uint32_t k = 0; k < 4; ++k) {
        s.num(render_load<S16>(v.signal, v.sig_off + (uint64_t)k * v.ns + i));
        s.ch('\t');
      }
      if (aux == 0) {
        TRACYHIP_RENDER_LIT(s, "NA\tNA\tNA\tNA\tNA\tNA\n");
        return;
      }
      const uint32_t c = aux - 1;
      s.num((int32_t)(c + 1));
      s.ch('\t'); s.ch(v.pri[c]);
      s.ch('\t'); s.ch(v.sec[c]);
      s.ch('\t'); s.ch(v.con[c]);
      s.ch('\t');
      s.num((int32_t)v.q[c]);
      s.ch('\t'); s.ch((c < v.trim_l || c >= v.keep_until) ? 'Y' : 'N');
      s.ch('\n');
      return;
    }
    case RS_POS:
    case RS_PEAK_A: case RS_PEAK_C: case RS_PEAK_G: case RS_PEAK_T: {
      if (i == 0) {
        if (sec == RS_POS) TRACYHIP_RENDER_LIT(s, "\"pos\": [");
        else {
          TRACYHIP_RENDER_LIT(s, "\"peak");
          s.ch((uint8_t)("ACGT"[sec - RS_PEAK_A]));
          TRACYHIP_RENDER_LIT(s, "\": [");
        }
      } else TRACYHIP_RENDER_LIT(s, ", ");
      if (sec == RS_POS) s.num((int32_t)(i + 1));
      else s.num(render_load<S16>(v.signal, v.sig_off + (uint64_t)(sec - RS_PEAK_A) * v.ns + i));
      if (i == v.ns - 1) TRACYHIP_RENDER_LIT(s, "],\n");
      return;
    }
    case RS_BCPOS:
    case RS_BCQUAL: {
      if (i == 0) {
        if (sec == RS_BCPOS) TRACYHIP_RENDER_LIT(s, "\"basecallPos\": [");
        else TRACYHIP_RENDER_LIT(s, "\"basecallQual\": [");
      } else TRACYHIP_RENDER_LIT(s, ", ");
      if (sec == RS_BCPOS) s.num((int32_t)((uint32_t)v.pos[i] + 1u));
      else s.num((int32_t)v.q[i]);
      if (i == v.n - 1) TRACYHIP_RENDER_LIT(s, "],\n");
      return;
    }
    case RS_CALLS:
    case RS_CALLS_GAPPED: {
      if (i == 0) TRACYHIP_RENDER_LIT(s, "\"basecalls\": {");
      else TRACYHIP_RENDER_LIT(s, ", ");
      const uint8_t p = v.pri[i], c2 = v.sec[i];
      s.ch('"');
      s.num((int32_t)((uint32_t)v.pos[i] + 1u));
      if (sec == RS_CALLS_GAPPED && p == '-') TRACYHIP_RENDER_LIT(s, "\":\"-\"");
      else {
        TRACYHIP_RENDER_LIT(s, "\":\"");
        s.num((int32_t)(sec == RS_CALLS ? i + 1 : aux));
        s.ch(':'); s.ch(p);
        if (p != c2) {
          s.ch('|');
          if (sec == RS_CALLS_GAPPED) s.ch(c2);
          else switch (c2) {  // expandIUPAC, abif.h:99-113
            case 'A': case 'C': case 'G': case 'T': case 'N': s.ch(c2); break;
            case 'R': TRACYHIP_RENDER_LIT(s, "A|G"); break;
            case 'Y': TRACYHIP_RENDER_LIT(s, "C|T"); break;
            case 'S': TRACYHIP_RENDER_LIT(s, "C|G"); break;
            case 'W': TRACYHIP_RENDER_LIT(s, "A|T"); break;
            case 'K': TRACYHIP_RENDER_LIT(s, "G|T"); break;
            case 'M': TRACYHIP_RENDER_LIT(s, "A|C"); break;
            default: s.ch('N');
          }
        }
        s.ch('"');
      }
      if (i == v.n - 1) {
        if (sec == RS_CALLS) TRACYHIP_RENDER_LIT(s, "},\n");
        else TRACYHIP_RENDER_LIT(s, "}\n");
      }
      return;
    }
    case RS_PRISEQ:
    case RS_SECSEQ: {
      if (i == 0) {
        if (sec == RS_PRISEQ) TRACYHIP_RENDER_LIT(s, "\"primarySeq\": \"");
        else TRACYHIP_RENDER_LIT(s, "\"secondarySeq\": \"");
      }
      s.ch(sec == RS_PRISEQ ? v.pri[i] : v.sec[i]);
      if (i == v.n - 1) {
        if (sec == RS_PRISEQ) TRACYHIP_RENDER_LIT(s, "\",\n");
        else TRACYHIP_RENDER_LIT(s, "\"\n");
      }
      return;
    }
    default: return;
  }
}

// the trace that owns tile `tile`: the last one whose tile_first is <= tile among those that own a tile (tile_first does not fall)
TR_HD uint32_t render_trace_of(const RenderTrace* tr, uint32_t ntraces, uint32_t tile) {
  uint32_t lo = 0, hi = ntraces;  // first trace whose tile_first is > tile
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tr[mid].tile_first <= tile) lo = mid + 1; else hi = mid;
  }
  return lo - 1;  // (traces without a tile share the tile_first of the next one and sit below it: lo - 1 is the owner)
}

TR_HD RenderView render_view(const RenderArgs& a, const RenderTrace& tr) {
  RenderView v;
  v.signal = a.signal; v.sig_off = tr.sig_off;
  v.pos = a.bcpos + tr.bc_off;
  v.pri = a.primary + tr.bc_off; v.sec = a.secondary + tr.bc_off;
  v.con = a.consensus ? a.consensus + tr.bc_off : v.pri;  // (read by the TSV alone, which validate refuses without it)
  v.q = a.estqual + tr.bc_off;
  v.ns = tr.nsamples; v.n = tr.bc_len; v.trim_l = tr.trim_l;
  v.keep_until = tr.trim_r < tr.bc_len ? tr.bc_len - tr.trim_r : 0;
  return v;
}

// What the items of a tile need beyond their index, kept from step to step.  begin() is called by the whole wave once per tile,
// aux() by the whole wave once per step of 64 items.
struct RenderTileState {
  uint32_t c_lo = 0;     // RS_SAMPLES: the first call at or behind the tile's first sample
  uint32_t gapless = 0;  // RS_CALLS_GAPPED: non-'-' primaries in front of the step
  template <class W>
  TR_HD void begin(W& w, const RenderView& v, const RenderTileAt& at, bool have_gapless, uint32_t gapless_in) {
    const uint32_t lane = w.lane();
    if (at.sec == RS_SAMPLES) {
      uint32_t lo = 0, hi = v.n;  // first call whose position is >= at.i0 (the same in every lane)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v.pos[mid] < (int32_t)at.i0) lo = mid + 1; else hi = mid;
      }
      c_lo = lo;
      uint16_t* tab = reinterpret_cast<uint16_t*>(w.lds() + kRenderImage);
      for (uint32_t j = lane; j < kRenderTile; j += 64) tab[j] = 0;
      w.sync();
      // positions that rise by at least one: no more than kRenderTile calls fall into the tile
      for (uint32_t j = lane; j < kRenderTile && c_lo + j < v.n; j += 64) {
        const int32_t p = v.pos[c_lo + j];
        if (p >= (int32_t)at.i0 && p < (int32_t)at.i1) tab[(uint32_t)p - at.i0] = (uint16_t)(j + 1);
      }
      w.sync();
    } else if (at.sec == RS_CALLS_GAPPED) {
      if (have_gapless) gapless = gapless_in;
      else {
        uint32_t cnt = 0;
        for (uint32_t j = lane; j < at.i0; j += 64) cnt += v.pri[j] != '-' ? 1u : 0u;
        gapless = w.sum(cnt);
      }
    }
  }
  template <class W>
  TR_HD uint32_t aux(W& w, const RenderView& v, const RenderTileAt& at, uint32_t i, bool valid) {
    if (at.sec == RS_SAMPLES) {
      if (!valid) return 0;
      const uint32_t j = reinterpret_cast<const uint16_t*>(w.lds() + kRenderImage)[i - at.i0];
      return j ? c_lo + j : 0;  // 1 + the call
    }
    if (at.sec == RS_CALLS_GAPPED) {
      const uint32_t lane = w.lane();
      const uint64_t m = w.ballot(valid && v.pri[i] != '-');
      const uint64_t upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1);
      const uint32_t r = gapless + (uint32_t)__builtin_popcountll(m & upto);  // ++gapless of this call, where it has one
      gapless += (uint32_t)__builtin_popcountll(m);
      return r;
    }
    return 0;
  }
};

// ---- launch 1: one wave per tile ----
template <bool S16, class W>
TR_HD void render_count_body(W& w, const RenderArgs& a, uint32_t tile) {
  const uint32_t lane = w.lane();
  const uint32_t t = render_trace_of(a.tr, a.ntraces, tile);
  const RenderTrace tr = a.tr[t];
  const RenderView v = render_view(a, tr);
  const RenderTileAt at = render_locate(a.form, v.ns, v.n, tile - tr.tile_first);
  if (at.sec == RS_CHECK) {
    bool bad = false;
    for (uint32_t i = at.i0 + lane; i < at.i1; i += 64) {
      const int32_t cur = v.pos[i];
      if (cur < 0 || (uint32_t)cur >= v.ns || (i && cur <= v.pos[i - 1])) bad = true;
    }
    const uint64_t any = w.ballot(bad);
    if (lane == 0) { a.tile_bytes[tile] = 0; a.tile_aux[tile] = any ? 1u : 0u; }
    return;
  }
  RenderTileState st;
  st.begin(w, v, at, false, 0);
  const uint32_t gapless_front = st.gapless;
  uint32_t bytes = 0;
  for (uint32_t i0 = at.i0; i0 < at.i1; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool valid = i < at.i1;
    const uint32_t aux = st.aux(w, v, at, i, valid);
    RenderCount c;
    if (valid) render_item<S16>(v, at.sec, i, aux, c);
    bytes += c.n;
  }
  bytes = w.sum(bytes);
  if (lane == 0) { a.tile_bytes[tile] = bytes; a.tile_aux[tile] = gapless_front; }
}

// ---- launch 2: one wave per trace ----
template <class W>
TR_HD void render_scan_body(W& w, const RenderArgs& a, uint32_t t) {
  const uint32_t lane = w.lane();
  const RenderTrace tr = a.tr[t];
  if (!tr.answerable) {  // (the whole wave)
    if (lane == 0) a.out[t] = RenderOut{kRenderStatusDeferred, 0};
    return;
  }
  const uint32_t tiles = render_tiles(a.form, tr.nsamples, tr.bc_len), checks = render_tiles_of(tr.bc_len);
  uint32_t total = 0;  // (below 2^31: render_bound)
  bool bad = false;
  for (uint32_t k0 = 0; k0 < tiles; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool in = k < tiles;
    const uint32_t b = in ? a.tile_bytes[tr.tile_first + k] : 0u;
    if (in && k < checks && a.tile_aux[tr.tile_first + k]) bad = true;
    const uint32_t before = total + w.excl_sum(b);
    if (in) a.tile_bytes[tr.tile_first + k] = before;
    total += w.sum(b);
  }
  if (w.ballot(bad) != 0) {
    if (lane == 0) a.out[t] = RenderOut{kRenderStatusDeferred, 0};
    return;
  }
  const bool small = a.text != nullptr && (uint64_t)total > tr.text_cap;
  if (lane == 0) a.out[t] = RenderOut{small ? kRenderStatusTooSmall : kRenderStatusOk, total};
}

// ---- launch 3: one wave per tile ----
struct alignas(16) RenderVec { uint32_t v[4]; };

// The LDS image: byte j of it is destined for address `base + j`, base a multiple of 16; [lo, hi) is composed and not yet stored, lo < 16.
// Whole 16-byte words of [lo, hi) leave as one store each, the bytes in front of the first word boundary byte-wise once a boundary is
// reached; what is left behind the last boundary moves to the front.  last: everything leaves.  Called by the whole wave.
template <class W>
TR_HD void render_flush(W& w, uint8_t* img, uint8_t*& base, uint32_t& lo, uint32_t& hi, bool last) {
  const uint32_t lane = w.lane();
  const uint32_t full = hi & ~15u;
  if (full > lo) {
    uint32_t start = lo;
    if (lo & 15u) {  // (lo < 16)
      if (lane >= lo && lane < 16) base[lane] = img[lane];
      start = 16;
    }
    for (uint32_t j = start + 16 * lane; j < full; j += 16 * 64)
      *reinterpret_cast<RenderVec*>(base + j) = *reinterpret_cast<const RenderVec*>(img + j);
    const uint32_t rest = hi - full;
    uint8_t keep = 0;
    if (lane < rest) keep = img[full + lane];
    w.sync();
    if (lane < rest) img[lane] = keep;
    base += full; lo = 0; hi = rest;
    w.sync();
  }
  if (last && lane >= lo && lane < hi) base[lane] = img[lane];  // (hi < 16 here)
}

template <bool S16, class W>
TR_HD void render_emit_body(W& w, const RenderArgs& a, uint32_t tile) {
  const uint32_t lane = w.lane();
  const uint32_t t = render_trace_of(a.tr, a.ntraces, tile);
  if (a.out[t].status != kRenderStatusOk) return;  // (the whole wave)
  const RenderTrace tr = a.tr[t];
  const RenderView v = render_view(a, tr);
  const RenderTileAt at = render_locate(a.form, v.ns, v.n, tile - tr.tile_first);
  if (at.sec == RS_CHECK) return;
  uint8_t* img = reinterpret_cast<uint8_t*>(w.lds());
  uint8_t* dst = a.text + tr.text_off + a.tile_bytes[tile];
  uint32_t lo = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u), hi = lo;
  uint8_t* base = dst - lo;
  RenderTileState st;
  st.begin(w, v, at, true, a.tile_aux[tile]);
  for (uint32_t i0 = at.i0; i0 < at.i1; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool valid = i < at.i1;
    const uint32_t aux = st.aux(w, v, at, i, valid);
    RenderCount c;
    if (valid) render_item<S16>(v, at.sec, i, aux, c);
    const uint32_t off = w.excl_sum(c.n), step = w.sum(c.n);
    if (valid) {
      RenderWrite wr{img + hi + off};
      render_item<S16>(v, at.sec, i, aux, wr);
    }
    hi += step;
    w.sync();
    render_flush(w, img, base, lo, hi, i0 + 64 >= at.i1);
  }
}

}  // namespace tracyhip
#endif
