// dcptext_wave.h -- the text of ONE tile of one trace's decompose report on ONE wave: writeDecomposition (decompose.h:622-632), the tail of
// traceAlleleAlignJsonOut behind the trace body (json.h:327-381) and the record lines of the VCF (variants.h:198-252 as text), byte for
// byte what tracy_amd/host/indigo_out.hpp prints (writeDecomposition, traceAlleleAlignJsonTail, vcfRecordLines) for every trace it answers.
//
// As in render_wave.h and alntext_wave.h a text is a sequence of SECTIONS, a section a sequence of ITEMS, and a TILE is kDcpTile
// consecutive items of one section, in the order of the text: a tile owns one contiguous piece of the text.
//     DECOMP  the header line, then one item per table row
//     JSON    chartConfig .. "alt1align": " | six row sections | "x" list | "y" list | variant rows | x ranges
//             a row section: one item per column (its byte) and a last item, the fixed text up to the next row (the closing of a list
//             section likewise); the last item of the x ranges closes the report
//     VCF     one item per variant record
// A variant section has max_variants items (the host cannot know var_n, which lies with the payloads): items at or behind var_n print
// nothing.  In front of the JSON and the VCF a section of max_variants items and no bytes CHECKS what only the data can tell: var_n <=
// max_variants, every variant's call index inside the basecalls, its ref and alt inside the trace's text region.  The items guard
// themselves by the same test (dcp_variant_ok), so that no read depends on an unchecked number: a record that fails prints nothing and
// the trace is DEFERRED by the scan.
//
// Three bodies, one wave each:
//     dcptext_count_body  per tile: the bytes of its items (the same dcptext_item text as the emit pass, into a counting sink); a tile of
//                         a row section counts its columns without a look at them
//     dcptext_scan_body   per trace: the exclusive sum over its tiles in place (tile offsets), text_len and the status
//     dcptext_emit_body   per tile: a lane measures its item, excl_sum places it, the lane writes it at its exact offset; the columns of
//                         a row section -- the bulk of a report -- are copied by the whole wave, as aligned dwords put together from the
//                         two source dwords they straddle (dcp_copy).  Every byte is written exactly once, by the tile that owns it.
// Items are not bounded in length (a variant row holds the chromosome name, its ref and its alt), which is why they are written where
// they belong and not composed in LDS.
//
// W: the wave of dev_wave.h (lane, ballot, sum, excl_sum).
#ifndef TRACY_AMD_DCPTEXT_WAVE_H
#define TRACY_AMD_DCPTEXT_WAVE_H

#include <cstdint>

#include "../../include/tracy_hip.h"  // tracyhip_variant
#include "dp_lane.h"                  // TR_HD
#include "render_wave.h"              // render_digits, RenderCount / RenderWrite

namespace tracyhip {

constexpr int32_t kDcpStatusOk = 0, kDcpStatusDeferred = 1, kDcpStatusTooSmall = 2;  // TRACYHIP_DCPTEXT_*
constexpr uint32_t kDcpDecomp = 0, kDcpJson = 1, kDcpVcf = 2;                         // TRACYHIP_DCPTEXT_DECOMP / JSON / VCF
constexpr uint32_t kDcpMaxCols = 1u << 22;
constexpr uint32_t kDcpMaxName = 65535;
constexpr uint32_t kDcpMaxRows = 1u << 22;   // of a decomposition table
constexpr uint32_t kDcpMaxVariants = 1024, kDcpMaxText = 1u << 19;
constexpr uint32_t kDcpMaxCalls = 0x7fffffffu;
constexpr uint32_t kDcpTile = 256;  // items per tile
constexpr uint32_t kDcpAnswerable = 1u, kDcpForward = 2u, kDcpIndelShift = 4u;  // DcpDesc::flags
enum DcpName : uint32_t { DN_CHR1, DN_CHR2, DN_FRAC1, DN_FRAC2 };

enum DcpSection : uint32_t {
  DS_CHECK, DS_TABLE,                                                                          // DECOMP: the table alone
  DS_HEAD, DS_ROW0, DS_ROW1, DS_ROW2, DS_ROW3, DS_ROW4, DS_ROW5, DS_DCPX, DS_DCPY, DS_VROWS, DS_XRANGES,  // JSON
  DS_VCF,
  DS_NONE
};

struct DcpDesc {  // per trace, built by the host (dcptext_plan.h)
  uint64_t dcp_off;      // elements of dcp_indel / dcp_err
  uint64_t rows_off[3];  // bytes of rows0[k] / rows1[k]
  uint64_t bc_off;       // elements of bcpos / estqual
  uint64_t name_off[4];  // bytes of names: DcpName
  uint64_t text_off, text_cap;
  uint32_t dcp_rows, cols[3], bc_len, name_len[4];
  uint32_t ref_pos[2];
  int32_t score[3];
  uint32_t bp_index;     // trim_left + breakpoint: the basecall the viewport of the report is centred on
  uint32_t trim_l, trim_r;  // 16 bits each
  uint32_t var_slot;     // the trace's place in var (x max_variants), var_text (x max_text) and var_n
  uint32_t tile_first;   // of the launch's tiles; the trace owns dcp_tiles() of them (none where the host can tell it is not answered)
  uint32_t flags;        // kDcpAnswerable | kDcpForward | kDcpIndelShift
};
struct DcpOut {
  int32_t status;
  uint32_t text_len;
};
struct DcpArgs {
  const int32_t *dcp_indel, *dcp_err;
  const uint8_t *rows0[3], *rows1[3];
  const int32_t* bcpos;
  const uint8_t* estqual;
  const tracyhip_variant* var;
  const uint8_t* var_text;
  const uint32_t* var_n;
  const uint8_t* names;
  const DcpDesc* tr;
  DcpOut* out;
  uint32_t* tile_bytes;  // per tile: its bytes (count), then its offset in the trace's text (scan)
  uint32_t* tile_aux;    // per tile: a check tile "a variant is bad", else 0
  uint8_t* text;         // null: sizes only
  uint32_t n, ntiles, form, qual_cut, max_variants, max_text;
};

// what the host can tell (the variants are the data's)
TR_HD bool dcp_answerable(uint32_t form, const uint32_t cols[3], uint32_t bc_len, const uint32_t name_len[4], uint32_t bp_index) {
  if (form == kDcpDecomp) return true;
  if (bc_len == 0 || bc_len > kDcpMaxCalls || name_len[DN_CHR1] > kDcpMaxName) return false;
  if (form == kDcpVcf) return true;
  for (uint32_t k = 0; k < 3; ++k)
    if (cols[k] > kDcpMaxCols) return false;
  for (uint32_t k = 1; k < 4; ++k)
    if (name_len[k] > kDcpMaxName) return false;
  return bp_index < bc_len;
}

struct DcpShape {  // what the cut into sections, items and tiles depends on
  uint32_t form, dcp_rows, cols[3], max_variants;
};
TR_HD uint32_t dcp_tiles_of(uint32_t items) { return (items + kDcpTile - 1) / kDcpTile; }
TR_HD uint32_t dcp_nsections(uint32_t form) { return form == kDcpDecomp ? 1u : form == kDcpJson ? 12u : 2u; }
TR_HD DcpSection dcp_section(uint32_t form, uint32_t k) {
  if (form == kDcpDecomp) return DS_TABLE;
  if (k == 0) return DS_CHECK;
  if (form == kDcpVcf) return DS_VCF;
  return (DcpSection)(DS_HEAD + k - 1);
}
TR_HD bool dcp_is_row(DcpSection s) { return s >= DS_ROW0 && s <= DS_ROW5; }
TR_HD uint32_t dcp_items(DcpSection s, const DcpShape& h) {
  switch (s) {
    case DS_CHECK: case DS_VCF: return h.max_variants;
    case DS_TABLE: case DS_DCPX: case DS_DCPY: return h.dcp_rows + 1;
    case DS_HEAD: return 1;
    case DS_VROWS: case DS_XRANGES: return h.max_variants + 1;
    default: return dcp_is_row(s) ? h.cols[(s - DS_ROW0) >> 1] + 1 : 0;
  }
}
TR_HD uint32_t dcp_check_tiles(const DcpShape& h) { return h.form == kDcpDecomp ? 0u : dcp_tiles_of(h.max_variants); }
TR_HD uint32_t dcp_tiles(const DcpShape& h) {
  uint32_t t = 0;
  for (uint32_t k = 0; k < dcp_nsections(h.form); ++k) t += dcp_tiles_of(dcp_items(dcp_section(h.form, k), h));
  return t;
}
struct DcpTileAt {
  DcpSection sec;
  uint32_t i0, i1;  // items
};
TR_HD DcpTileAt dcp_locate(const DcpShape& h, uint32_t tile) {
  for (uint32_t k = 0; k < dcp_nsections(h.form); ++k) {
    const DcpSection s = dcp_section(h.form, k);
    const uint32_t items = dcp_items(s, h), tiles = dcp_tiles_of(items);
    if (tile < tiles) {
      const uint32_t i0 = tile * kDcpTile;
      return DcpTileAt{s, i0, items - i0 < kDcpTile ? items : i0 + kDcpTile};
    }
    tile -= tiles;
  }
  return DcpTileAt{DS_NONE, 0, 0};
}

struct DcpView {  // one trace
  const int32_t *indel, *err, *pos;
  const uint8_t *r[6], *q, *vtext, *nm[4];
  const tracyhip_variant* var;
  uint32_t rows, cols[3], n, nlen[4], ref_pos[2], bp_index, trim_l, trim_r, nvar, var_n, max_variants, max_text, qual_cut;
  int32_t score[3];
  bool forward, indelshift;
};
TR_HD DcpShape dcp_shape(const DcpArgs& a, const DcpDesc& d) {
  return DcpShape{a.form, d.dcp_rows, {d.cols[0], d.cols[1], d.cols[2]}, a.max_variants};
}
TR_HD DcpView dcp_view(const DcpArgs& a, const DcpDesc& d) {
  DcpView v{};
  const bool table = a.form != kDcpVcf, calls = a.form != kDcpDecomp, json = a.form == kDcpJson;
  if (table) { v.indel = a.dcp_indel + d.dcp_off; v.err = a.dcp_err + d.dcp_off; }
  v.rows = d.dcp_rows;
  for (uint32_t k = 0; k < 3; ++k) {
    v.cols[k] = d.cols[k];
    if (json) { v.r[2 * k] = a.rows0[k] + d.rows_off[k]; v.r[2 * k + 1] = a.rows1[k] + d.rows_off[k]; }
    v.score[k] = d.score[k];
  }
  for (uint32_t k = 0; k < 4; ++k) {
    v.nlen[k] = d.name_len[k];
    if (calls) v.nm[k] = a.names + d.name_off[k];
  }
  v.n = d.bc_len;
  v.max_variants = a.max_variants; v.max_text = a.max_text; v.qual_cut = a.qual_cut & 0xffffu;
  if (calls) {
    v.pos = a.bcpos + d.bc_off; v.q = a.estqual + d.bc_off;
    v.var = a.var + (uint64_t)d.var_slot * a.max_variants;
    v.vtext = a.var_text + (uint64_t)d.var_slot * a.max_text;
    v.var_n = a.var_n[d.var_slot];
    v.nvar = v.var_n < a.max_variants ? v.var_n : a.max_variants;
  }
  v.ref_pos[0] = d.ref_pos[0]; v.ref_pos[1] = d.ref_pos[1];
  v.bp_index = d.bp_index; v.trim_l = d.trim_l; v.trim_r = d.trim_r;
  v.forward = (d.flags & kDcpForward) != 0;
  v.indelshift = (d.flags & kDcpIndelShift) != 0;
  return v;
}

#define TRACYHIP_DCP_LIT(s, text) (s).lit(text, (uint32_t)sizeof(text) - 1u)

template <class Sink>
TR_HD void dcp_unum(Sink& s, uint32_t x) {  // an unsigned number through the sinks' signed one
  if (x <= 0x7fffffffu) { s.num((int32_t)x); return; }
  s.num((int32_t)(x / 10u));
  s.ch((uint8_t)('0' + x % 10u));
}
template <class Sink>
TR_HD void dcp_bytes(Sink& s, const uint8_t* p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) s.ch(p[i]);
}

// variantCallIndex (variants.h:205) of a record, in the 32 bits the writers compute it in
TR_HD uint32_t dcp_call_index(const DcpView& v, const tracyhip_variant& r) {
  return v.forward ? v.trim_l + (uint32_t)r.basenum - 1u : v.n - (v.trim_r + (uint32_t)r.basenum);
}
// the record may be printed: its call lies inside the basecalls, its ref and alt inside the trace's text region
TR_HD bool dcp_variant_ok(const DcpView& v, const tracyhip_variant& r) {
  return dcp_call_index(v, r) < v.n && (uint64_t)r.ref_off + r.ref_len <= v.max_text && (uint64_t)r.alt_off + r.alt_len <= v.max_text;
}
// xWindowViewport (json.h:248-257) around basecall q < n
TR_HD void dcp_viewport(const DcpView& v, uint32_t q, int32_t& lo, int32_t& hi) {
  const int64_t centre = (int64_t)v.pos[q] + 1, lastpeak = v.pos[v.n - 1];
  lo = (int32_t)(centre <= 150 ? 1 : centre - 150);
  hi = (int32_t)(centre + 150 < lastpeak ? centre + 150 : lastpeak);
}
template <class Sink>
TR_HD void dcp_variant_type(Sink& s, const tracyhip_variant& r) {  // variantType, variants.h:129-138
  if (r.ref_len == 1 && r.alt_len == 1) TRACYHIP_DCP_LIT(s, "SNV");
  else if (r.ref_len > r.alt_len) TRACYHIP_DCP_LIT(s, "Deletion");
  else if (r.ref_len < r.alt_len) TRACYHIP_DCP_LIT(s, "Insertion");
  else TRACYHIP_DCP_LIT(s, "Complex");
}
template <class Sink>
TR_HD void dcp_allele_end(Sink& s, const DcpView& v, uint32_t k) {  // behind row 1 of allele k + 1
  TRACYHIP_DCP_LIT(s, "\",\n\"ref");
  s.ch((uint8_t)('1' + k));
  TRACYHIP_DCP_LIT(s, "forward\": ");
  s.ch(v.forward ? '1' : '0');
  TRACYHIP_DCP_LIT(s, ",\n\"align");
  s.ch((uint8_t)('1' + k));
  TRACYHIP_DCP_LIT(s, "score\": ");
  s.num(v.score[k]);
  TRACYHIP_DCP_LIT(s, ",\n");
}
template <class Sink>
TR_HD void dcp_allele_begin(Sink& s, const DcpView& v, uint32_t k) {  // in front of row 0 of allele k + 1
  TRACYHIP_DCP_LIT(s, "\"ref");
  s.ch((uint8_t)('1' + k));
  TRACYHIP_DCP_LIT(s, "chr\": \"");
  dcp_bytes(s, v.nm[DN_CHR1 + k], v.nlen[DN_CHR1 + k]);
  TRACYHIP_DCP_LIT(s, "\",\n\"ref");
  s.ch((uint8_t)('1' + k));
  TRACYHIP_DCP_LIT(s, "pos\": ");
  dcp_unum(s, v.ref_pos[k] + 1u);
  TRACYHIP_DCP_LIT(s, ",\n\"alt");
  s.ch((uint8_t)('1' + k));
  TRACYHIP_DCP_LIT(s, "align\": \"");
}

// item i of section `sec` into sink s
template <class Sink>
TR_HD void dcptext_item(const DcpView& v, DcpSection sec, uint32_t i, Sink& s) {
  switch (sec) {
    case DS_TABLE:
      if (i == 0) { TRACYHIP_DCP_LIT(s, "indel\tdecomp\n"); return; }
      s.num(v.indel[i - 1]); s.ch('\t'); s.num(v.err[i - 1]); s.ch('\n');
      return;
    case DS_HEAD: {
      int32_t lo, hi;
      dcp_viewport(v, v.bp_index, lo, hi);
      TRACYHIP_DCP_LIT(s, ",\n\"chartConfig\": { \"x\": { \"axis\": { \"range\": [");
      s.num(lo); TRACYHIP_DCP_LIT(s, ", "); s.num(hi);
      TRACYHIP_DCP_LIT(s, "] }}},\n");
      dcp_allele_begin(s, v, 0);
      return;
    }
    case DS_ROW0: case DS_ROW1: case DS_ROW2: case DS_ROW3: case DS_ROW4: case DS_ROW5: {
      const uint32_t k = sec - DS_ROW0;
      if (i < v.cols[k >> 1]) { s.ch(v.r[k][i]); return; }
      switch (k) {
        case 0: TRACYHIP_DCP_LIT(s, "\",\n\"ref1align\": \""); return;
        case 1: dcp_allele_end(s, v, 0); dcp_allele_begin(s, v, 1); return;
        case 2: TRACYHIP_DCP_LIT(s, "\",\n\"ref2align\": \""); return;
        case 3:
          dcp_allele_end(s, v, 1);
          TRACYHIP_DCP_LIT(s, "\"allele1fraction\": ");
          dcp_bytes(s, v.nm[DN_FRAC1], v.nlen[DN_FRAC1]);
          TRACYHIP_DCP_LIT(s, ",\n\"allele1align\": \"");
          return;
        case 4:
          TRACYHIP_DCP_LIT(s, "\",\n\"allele2fraction\": ");
          dcp_bytes(s, v.nm[DN_FRAC2], v.nlen[DN_FRAC2]);
          TRACYHIP_DCP_LIT(s, ",\n\"allele2align\": \"");
          return;
        default:
          TRACYHIP_DCP_LIT(s, "\",\n\"align3score\": ");
          s.num(v.score[2]);
          TRACYHIP_DCP_LIT(s, ",\n\"hetindel\": ");
          s.ch(v.indelshift ? '1' : '0');
          TRACYHIP_DCP_LIT(s, ",\n\"decomposition\": {\n\"x\": [");
          return;
      }
    }
    case DS_DCPX:
    case DS_DCPY:
      if (i < v.rows) {
        if (i) TRACYHIP_DCP_LIT(s, ", ");
        s.num(sec == DS_DCPX ? v.indel[i] : v.err[i]);
      } else if (sec == DS_DCPX) TRACYHIP_DCP_LIT(s, "],\n\"y\": [");
      else
        TRACYHIP_DCP_LIT(s, "]\n},\n\"variants\": {\n\"columns\": [\"chr\", \"pos\", \"id\", \"ref\", \"alt\", \"qual\", \"filter\", \"type\", \"genotype\", "
                            "\"basepos\", \"signalpos\"],\n\"rows\": [\n");
      return;
    case DS_VROWS:
    case DS_XRANGES:
    case DS_VCF: {
      if (i >= v.max_variants) {
        if (sec == DS_VROWS) TRACYHIP_DCP_LIT(s, "],\n\"xranges\": [\n");
        else if (sec == DS_XRANGES) TRACYHIP_DCP_LIT(s, "]\n}\n}\n");
        return;
      }
      if (i >= v.nvar) return;
      const tracyhip_variant r = v.var[i];
      if (!dcp_variant_ok(v, r)) return;  // (the check tile has seen it: the trace is deferred)
      const uint32_t q = dcp_call_index(v, r);
      const int32_t estq = (int32_t)v.q[q];
      const uint8_t *ref = v.vtext + r.ref_off, *alt = v.vtext + r.alt_off;
      if (sec == DS_XRANGES) {
        int32_t lo, hi;
        dcp_viewport(v, q, lo, hi);
        if (i) TRACYHIP_DCP_LIT(s, ",\n");
        s.ch('['); s.num(lo); TRACYHIP_DCP_LIT(s, ", "); s.num(hi); s.ch(']');
        return;
      }
      if (sec == DS_VROWS) {
        if (i) TRACYHIP_DCP_LIT(s, ",\n");
        TRACYHIP_DCP_LIT(s, "[\"");
        dcp_bytes(s, v.nm[DN_CHR1], v.nlen[DN_CHR1]);
        TRACYHIP_DCP_LIT(s, "\", ");
        s.num(r.pos);
        TRACYHIP_DCP_LIT(s, ", \".\", \"");
        dcp_bytes(s, ref, r.ref_len);
        TRACYHIP_DCP_LIT(s, "\", \"");
        dcp_bytes(s, alt, r.alt_len);
        TRACYHIP_DCP_LIT(s, "\", ");
        s.num(estq);
        if ((uint32_t)estq < v.qual_cut) TRACYHIP_DCP_LIT(s, ", \"LowQual\", \"");
        else TRACYHIP_DCP_LIT(s, ", \"PASS\", \"");
        dcp_variant_type(s, r);
        TRACYHIP_DCP_LIT(s, "\", \"");
        if (r.gt == 0) TRACYHIP_DCP_LIT(s, "hom. REF");
        else if (r.gt == 1) TRACYHIP_DCP_LIT(s, "het.");
        else if (r.gt == 2) TRACYHIP_DCP_LIT(s, "hom. ALT");
        else TRACYHIP_DCP_LIT(s, "missing");
        TRACYHIP_DCP_LIT(s, "\", ");
        s.num((int32_t)(q + 1u));  // basepos: trimLeft + basenum forward, size - (trimRight + basenum) + 1 reverse -- both q + 1
        TRACYHIP_DCP_LIT(s, ", ");
        s.num((int32_t)((uint32_t)v.pos[q] + 1u));
        s.ch(']');
        return;
      }
      bool has_n = false;  // strInclN(v.alt)
      for (uint32_t j = 0; j < r.alt_len; ++j) has_n = has_n || alt[j] == 'n' || alt[j] == 'N';
      const int32_t qual = has_n ? 0 : estq;
      dcp_bytes(s, v.nm[DN_CHR1], v.nlen[DN_CHR1]);
      s.ch('\t'); s.num(r.pos);
      TRACYHIP_DCP_LIT(s, "\t.\t");
      dcp_bytes(s, ref, r.ref_len);
      s.ch('\t');
      dcp_bytes(s, alt, r.alt_len);
      s.ch('\t'); s.num(qual);
      if ((uint32_t)qual < v.qual_cut) TRACYHIP_DCP_LIT(s, "\tLowQual\tTYPE=");
      else TRACYHIP_DCP_LIT(s, "\tPASS\tTYPE=");
      dcp_variant_type(s, r);
      TRACYHIP_DCP_LIT(s, ";METHOD=EMBL.TRACYv0.9.1;BASEPOS=");
      s.num((int32_t)(q + 1u));
      TRACYHIP_DCP_LIT(s, ";SIGNALPOS=");
      s.num((int32_t)((uint32_t)v.pos[q] + 1u));
      TRACYHIP_DCP_LIT(s, "\tGT:GQ\t");
      if (r.gt == 0) TRACYHIP_DCP_LIT(s, "0/0");
      else if (r.gt == 1) TRACYHIP_DCP_LIT(s, "0/1");
      else if (r.gt == 2) TRACYHIP_DCP_LIT(s, "1/1");
      else TRACYHIP_DCP_LIT(s, "./.");
      s.ch(':'); s.num(estq); s.ch('\n');
      return;
    }
    default: return;
  }
}

// the trace that owns tile `tile`: the last one whose tile_first is <= tile among those that own a tile (tile_first does not fall)
TR_HD uint32_t dcp_owner_of(const DcpDesc* tr, uint32_t n, uint32_t tile) {
  uint32_t lo = 0, hi = n;  // first trace whose tile_first is > tile
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tr[mid].tile_first <= tile) lo = mid + 1; else hi = mid;
  }
  return lo - 1;  // (traces without a tile share the tile_first of the next one and sit below it: lo - 1 is the owner)
}

// n bytes from src to dst by the whole wave.  Behind a byte-wise head dst is dword aligned: each dword stored is put together from
// the one or two ALIGNED source dwords it straddles -- the second of which always holds a byte of the run, so no dword is read that the
// run does not reach into.  What is left behind the last whole dword leaves byte-wise.
template <class W>
TR_HD void dcp_copy(W& w, uint8_t* dst, const uint8_t* src, uint32_t n) {
  const uint32_t lane = w.lane();
  uint32_t head = (uint32_t)((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
  if (head > n) head = n;
  if (lane < head) dst[lane] = src[lane];
  const uint32_t words = (n - head) / 4u;
  const uint8_t* s = src + head;
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u);
  const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s - sh);
  uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + head);
  if (sh == 0) {
    for (uint32_t k = lane; k < words; k += 64) d4[k] = s4[k];
  } else {
    for (uint32_t k = lane; k < words; k += 64) d4[k] = (s4[k] >> (8u * sh)) | (s4[k + 1] << (32u - 8u * sh));  // (little endian)
  }
  const uint32_t done = head + 4u * words;
  if (lane < n - done) dst[done + lane] = src[done + lane];
}

// ---- launch 1: one wave per tile ----
template <class W>
TR_HD void dcptext_count_body(W& w, const DcpArgs& a, uint32_t tile) {
  const uint32_t lane = w.lane();
  const DcpDesc d = a.tr[dcp_owner_of(a.tr, a.n, tile)];
  const DcpView v = dcp_view(a, d);
  const DcpTileAt at = dcp_locate(dcp_shape(a, d), tile - d.tile_first);
  if (at.sec == DS_CHECK) {
    bool bad = at.i0 == 0 && v.var_n > v.max_variants;
    for (uint32_t i = at.i0 + lane; i < at.i1; i += 64)
      if (i < v.nvar && !dcp_variant_ok(v, v.var[i])) bad = true;
    const uint64_t any = w.ballot(bad);
    if (lane == 0) { a.tile_bytes[tile] = 0; a.tile_aux[tile] = any ? 1u : 0u; }
    return;
  }
  uint32_t bytes = 0;
  if (dcp_is_row(at.sec)) {  // the columns are a byte each, whatever they hold
    const uint32_t cols = v.cols[(at.sec - DS_ROW0) >> 1];
    RenderCount c;
    if (at.i1 == cols + 1u) dcptext_item(v, at.sec, cols, c);
    bytes = ((at.i1 < cols ? at.i1 : cols) - at.i0) + c.n;
  } else {
    for (uint32_t i0 = at.i0; i0 < at.i1; i0 += 64) {
      const uint32_t i = i0 + lane;
      RenderCount c;
      if (i < at.i1) dcptext_item(v, at.sec, i, c);
      bytes += c.n;
    }
    bytes = w.sum(bytes);
  }
  if (lane == 0) { a.tile_bytes[tile] = bytes; a.tile_aux[tile] = 0; }
}

// ---- launch 2: one wave per trace ----
template <class W>
TR_HD void dcptext_scan_body(W& w, const DcpArgs& a, uint32_t t) {
  const uint32_t lane = w.lane();
  const DcpDesc d = a.tr[t];
  if (!(d.flags & kDcpAnswerable)) {  // (the whole wave)
    if (lane == 0) a.out[t] = DcpOut{kDcpStatusDeferred, 0};
    return;
  }
  const DcpShape h = dcp_shape(a, d);
  const uint32_t tiles = dcp_tiles(h), checks = dcp_check_tiles(h);
  uint32_t total = 0;  // (below 2^31: dcptext_bound)
  bool bad = false;
  for (uint32_t k0 = 0; k0 < tiles; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool in = k < tiles;
    const uint32_t b = in ? a.tile_bytes[d.tile_first + k] : 0u;
    if (in && k < checks && a.tile_aux[d.tile_first + k]) bad = true;
    const uint32_t before = total + w.excl_sum(b);
    if (in) a.tile_bytes[d.tile_first + k] = before;
    total += w.sum(b);
  }
  if (w.ballot(bad) != 0) {
    if (lane == 0) a.out[t] = DcpOut{kDcpStatusDeferred, 0};
    return;
  }
  const bool small = a.text != nullptr && (uint64_t)total > d.text_cap;
  if (lane == 0) a.out[t] = DcpOut{small ? kDcpStatusTooSmall : kDcpStatusOk, total};
}

// ---- launch 3: one wave per tile ----
template <class W>
TR_HD void dcptext_emit_body(W& w, const DcpArgs& a, uint32_t tile) {
  const uint32_t lane = w.lane();
  const uint32_t t = dcp_owner_of(a.tr, a.n, tile);
  if (a.out[t].status != kDcpStatusOk) return;  // (the whole wave)
  const DcpDesc d = a.tr[t];
  const DcpView v = dcp_view(a, d);
  const DcpTileAt at = dcp_locate(dcp_shape(a, d), tile - d.tile_first);
  if (at.sec == DS_CHECK) return;
  uint8_t* dst = a.text + d.text_off + a.tile_bytes[tile];
  if (dcp_is_row(at.sec)) {
    const uint32_t k = at.sec - DS_ROW0, cols = v.cols[k >> 1];
    const uint32_t ncol = (at.i1 < cols ? at.i1 : cols) - at.i0;
    dcp_copy(w, dst, v.r[k] + at.i0, ncol);
    if (at.i1 == cols + 1u && lane == 0) {
      RenderWrite wr{dst + ncol};
      dcptext_item(v, at.sec, cols, wr);
    }
    return;
  }
  uint32_t done = 0;
  for (uint32_t i0 = at.i0; i0 < at.i1; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool valid = i < at.i1;
    RenderCount c;
    if (valid) dcptext_item(v, at.sec, i, c);
    const uint32_t off = w.excl_sum(c.n), step = w.sum(c.n);
    if (valid && c.n) {
      RenderWrite wr{dst + done + off};
      dcptext_item(v, at.sec, i, wr);
    }
    done += step;
  }
}

}  // namespace tracyhip
#endif
