// dcptext_plan.cpp -- a stand-alone run of tracy_amd/csrc/dcptext_plan.h and the HIP-free parts of dcptext_wave.h (no HIP, its own main;
// tests/test_emu_dcptext.py builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o dcptext_plan tests/cpp/dcptext_plan.cpp
// It checks: the tile cut of a trace (dcp_locate walks every section once, in order, tiles of at most kDcpTile items, as many as
// dcp_tiles says) at counts 0, 1 and one tile +- 1; the owner of a tile among traces of which some own none; every item of the deferral
// list, the host's at its edges (dcptext_answerable) and the data's (dcp_variant_ok); the two sinks of dcptext_item against each other
// and dcptext_bound against the text of extreme traces composed item by item; the chunk cut (consecutive, covering, within the limit,
// descriptors inside the spans, tile numbers that follow each other, the same tiles whatever the limit); an offset that leaves 64
// bits; the verdicts of dcptext_validate.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../tracy_amd/csrc/dcptext_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static void check_tiles() {
  const uint32_t counts[] = {0u, 1u, kDcpTile - 2, kDcpTile - 1, kDcpTile, kDcpTile + 1, 2 * kDcpTile + 1};
  for (uint32_t form = 0; form < 3; ++form)
    for (uint32_t rows : counts)
      for (uint32_t cols : counts)
        for (uint32_t maxv : {1u, kDcpTile - 1, kDcpTile, kDcpTile + 1, kDcpMaxVariants}) {
          const DcpShape h{form, rows, {cols, cols / 2, 0u}, maxv};
          const uint32_t tiles = dcp_tiles(h);
          uint32_t k = 0;
          for (uint32_t s = 0; s < dcp_nsections(form); ++s) {
            const DcpSection sec = dcp_section(form, s);
            const uint32_t items = dcp_items(sec, h);
            CHECK(items >= 1);
            for (uint32_t i0 = 0; i0 < items; i0 += kDcpTile, ++k) {
              const DcpTileAt at = dcp_locate(h, k);
              CHECK(at.sec == sec && at.i0 == i0 && at.i1 == std::min(items, i0 + kDcpTile));
            }
          }
          CHECK(k == tiles);
          CHECK(dcp_locate(h, tiles).sec == DS_NONE);
          CHECK((form == kDcpDecomp) == (dcp_section(form, 0) != DS_CHECK));
          CHECK(dcp_check_tiles(h) == (form == kDcpDecomp ? 0u : dcp_tiles_of(maxv)));
        }
  const DcpShape h{kDcpJson, 7, {10, 20, 30}, 4};
  CHECK(dcp_items(DS_ROW0, h) == 11 && dcp_items(DS_ROW1, h) == 11 && dcp_items(DS_ROW2, h) == 21 && dcp_items(DS_ROW5, h) == 31);
  CHECK(dcp_items(DS_DCPX, h) == 8 && dcp_items(DS_VROWS, h) == 5 && dcp_items(DS_VCF, h) == 4 && dcp_items(DS_TABLE, h) == 8);
  // owners: traces 1, 2 and 5 own no tile
  const uint32_t first[6] = {0, 5, 5, 5, 9, 12};
  std::vector<DcpDesc> tr(6);
  for (int t = 0; t < 6; ++t) tr[t].tile_first = first[t];
  const uint32_t owner[12] = {0, 0, 0, 0, 0, 3, 3, 3, 3, 4, 4, 4};
  for (uint32_t k = 0; k < 12; ++k) CHECK(dcp_owner_of(tr.data(), 6, k) == owner[k]);
}

// a batch of traces over arrays of its own
struct Batch {
  uint32_t n;
  std::vector<int32_t> indel, err, bcpos;
  std::vector<uint8_t> rows[3][2], estqual, vtext, names, forward, indelshift;
  std::vector<uint64_t> dcp_off, rows_off[3], bc_off, name_off[4], text_off, text_cap;
  std::vector<uint32_t> dcp_rows, cols[3], bc_len, name_len[4], var_n, ref_pos[2], breakpoint, trim_l, trim_r;
  std::vector<int32_t> score[3], status;
  std::vector<uint32_t> text_len;
  std::vector<tracyhip_variant> var;
  std::vector<uint8_t> text;
  tracyhip_dcptext_job job{};
  tracyhip_dcptext_result res{};

  Batch(uint32_t n_, uint32_t form, uint32_t rows_each, uint32_t cols_each, uint32_t bc_each, uint32_t name_each, uint32_t maxv, uint32_t maxt) : n(n_) {
    auto off = [&](std::vector<uint64_t>& o, uint64_t each) { o.resize(n); for (uint32_t t = 0; t < n; ++t) o[t] = t * each; };
    indel.assign((size_t)n * rows_each + 1, -7); err.assign((size_t)n * rows_each + 1, 9);
    off(dcp_off, rows_each); dcp_rows.assign(n, rows_each);
    for (int k = 0; k < 3; ++k) {
      for (int r = 0; r < 2; ++r) rows[k][r].assign((size_t)n * cols_each + 4, (uint8_t)('A' + k + r));
      off(rows_off[k], cols_each); cols[k].assign(n, cols_each); score[k].assign(n, -3 + k);
    }
    bcpos.resize((size_t)n * bc_each + 1);
    for (size_t i = 0; i < bcpos.size(); ++i) bcpos[i] = (int32_t)(5 + 11 * (i % (bc_each ? bc_each : 1)));
    estqual.assign((size_t)n * bc_each + 1, 40);
    off(bc_off, bc_each); bc_len.assign(n, bc_each);
    var.assign((size_t)n * maxv, tracyhip_variant{}); vtext.assign((size_t)n * maxt, 'C'); var_n.assign(n, 0);
    names.assign((size_t)4 * n * name_each + 4, 'x');
    for (int k = 0; k < 4; ++k) { name_off[k].resize(n); name_len[k].assign(n, name_each); for (uint32_t t = 0; t < n; ++t) name_off[k][t] = ((uint64_t)4 * t + k) * name_each; }
    for (int k = 0; k < 2; ++k) ref_pos[k].assign(n, 100 + k);
    forward.assign(n, 1); indelshift.assign(n, 1); breakpoint.assign(n, 0); trim_l.assign(n, 0); trim_r.assign(n, 0);
    status.assign(n, -1); text_len.assign(n, 0);
    job.n = n; job.form = form; job.qual_cut = 45;
    job.dcp_indel = indel.data(); job.dcp_err = err.data(); job.dcp_offset = dcp_off.data(); job.dcp_rows = dcp_rows.data();
    for (int k = 0; k < 3; ++k) {
      job.rows0[k] = rows[k][0].data(); job.rows1[k] = rows[k][1].data(); job.rows_offset[k] = rows_off[k].data(); job.cols[k] = cols[k].data();
      job.score[k] = score[k].data();
    }
    job.bcpos = bcpos.data(); job.estqual = estqual.data(); job.bc_offset = bc_off.data(); job.bc_len = bc_len.data();
    job.var = var.data(); job.var_text = vtext.data(); job.var_n = var_n.data(); job.max_variants = maxv; job.max_text = maxt;
    for (int k = 0; k < 2; ++k) {
      job.ref_pos[k] = ref_pos[k].data();
      job.chr_offset[k] = name_off[k].data(); job.chr_len[k] = name_len[k].data();
      job.frac_offset[k] = name_off[2 + k].data(); job.frac_len[k] = name_len[2 + k].data();
    }
    job.forward = forward.data(); job.indelshift = indelshift.data(); job.breakpoint = breakpoint.data();
    job.trim_left = trim_l.data(); job.trim_right = trim_r.data(); job.names = names.data();
    res.status = status.data(); res.text_len = text_len.data();
  }
  void with_text(uint64_t cap_each) {
    text.assign((size_t)n * cap_each + 1, 0);
    text_off.resize(n); text_cap.assign(n, cap_each);
    for (uint32_t t = 0; t < n; ++t) text_off[t] = t * cap_each;
    res.text = text.data(); res.text_offset = text_off.data(); res.text_cap = text_cap.data();
  }
  DcpArgs args(const DcpDesc* d) const {
    DcpArgs a{};
    a.dcp_indel = job.dcp_indel; a.dcp_err = job.dcp_err;
    for (int k = 0; k < 3; ++k) { a.rows0[k] = job.rows0[k]; a.rows1[k] = job.rows1[k]; }
    a.bcpos = job.bcpos; a.estqual = job.estqual; a.var = job.var; a.var_text = job.var_text; a.var_n = job.var_n; a.names = job.names;
    a.tr = d; a.n = n; a.form = job.form; a.qual_cut = job.qual_cut; a.max_variants = job.max_variants; a.max_text = job.max_text;
    return a;
  }
};

// the whole text of trace t, item after item; every item through both sinks
static std::string compose(const Batch& b, uint32_t t) {
  std::vector<DcpChunk> chunks;
  uint32_t bad = 0;
  CHECK(dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad) && chunks.size() == 1);
  const DcpDesc d = dcptext_desc(&b.job, &b.res, chunks[0], false, t, 0);
  const DcpArgs a = b.args(&d);
  const DcpView v = dcp_view(a, d);
  const DcpShape h = dcp_shape(a, d);
  std::string text;
  for (uint32_t s = 0; s < dcp_nsections(b.job.form); ++s) {
    const DcpSection sec = dcp_section(b.job.form, s);
    if (sec == DS_CHECK) continue;
    for (uint32_t i = 0; i < dcp_items(sec, h); ++i) {
      RenderCount c;
      dcptext_item(v, sec, i, c);
      std::string piece(c.n + 8, '\x7e');
      RenderWrite w{reinterpret_cast<uint8_t*>(&piece[0])};
      dcptext_item(v, sec, i, w);
      CHECK(w.p == reinterpret_cast<uint8_t*>(&piece[0]) + c.n && piece.compare(c.n, 8, std::string(8, '\x7e')) == 0);
      text.append(piece, 0, c.n);
    }
  }
  return text;
}

static tracyhip_dcptext_shape shape_of(const Batch& b, uint32_t t) {
  tracyhip_dcptext_shape s{};
  s.dcp_rows = b.dcp_rows[t];
  for (int k = 0; k < 3; ++k) s.cols[k] = b.cols[k][t];
  for (int k = 0; k < 2; ++k) { s.chr_len[k] = b.name_len[k][t]; s.frac_len[k] = b.name_len[2 + k][t]; }
  s.max_variants = b.job.max_variants; s.max_text = b.job.max_text;
  return s;
}

static void check_bound_and_sinks() {
  for (uint32_t form = 0; form < 3; ++form)
    for (uint32_t rows : {0u, 1u, 255u, 256u, 257u})
      for (uint32_t cols : {0u, 1u, 255u, 256u, 257u})
        for (uint32_t nv : {0u, 1u, 3u}) {
          const uint32_t maxv = 3, maxt = 16, nb = 40;
          Batch b(1, form, rows, cols, nb, 5, maxv, maxt);
          // the longest numbers there are: INT32_MIN everywhere, positions at the far end, a quality of three digits
          for (auto& x : b.indel) x = INT32_MIN;
          for (auto& x : b.err) x = INT32_MIN;
          for (int k = 0; k < 3; ++k) b.score[k][0] = INT32_MIN;
          for (size_t i = 0; i < b.bcpos.size(); ++i) b.bcpos[i] = 2000000000 + (int32_t)i * 1000;
          for (auto& q : b.estqual) q = 255;
          b.ref_pos[0][0] = 0xfffffffeu; b.ref_pos[1][0] = 0x7fffffffu;
          b.var_n[0] = nv;
          for (uint32_t i = 0; i < nv; ++i) b.var[i] = tracyhip_variant{INT32_MIN, (int32_t)(nb - i), -1, 0, 0, maxt, 0, maxt};  // (Complex: the longest word but "Insertion")
          if (nv > 1) b.var[1] = tracyhip_variant{INT32_MIN, 2, 0, 0, 0, 1, 0, maxt};  // Insertion, "hom. REF"
          const std::string text = compose(b, 0);
          const tracyhip_dcptext_shape s = shape_of(b, 0);
          CHECK(dcptext_bound(form, s) >= text.size());
          if (form == kDcpDecomp) CHECK(text.size() == 13 + (size_t)rows * 24);
          if (form == kDcpVcf) CHECK((text.empty()) == (nv == 0));
          if (form == kDcpJson) CHECK(text.compare(0, 18, ",\n\"chartConfig\": {") == 0 && text.compare(text.size() - 6, 6, "]\n}\n}\n") == 0);
        }
  tracyhip_dcptext_shape big{};
  big.dcp_rows = kDcpMaxRows;
  for (int k = 0; k < 3; ++k) big.cols[k] = kDcpMaxCols;
  for (int k = 0; k < 2; ++k) big.chr_len[k] = big.frac_len[k] = kDcpMaxName;
  big.max_variants = kDcpMaxVariants; big.max_text = kDcpMaxText;
  for (uint32_t form = 0; form < 3; ++form) CHECK(dcptext_bound(form, big) > 0 && dcptext_bound(form, big) < (1ull << 31));  // text_len and the tile offsets are 32-bit
  CHECK(dcptext_bound(3, big) == 0);
}

static void check_deferral() {
  for (uint32_t form : {kDcpJson, kDcpVcf}) {
    const bool json = form == kDcpJson;
    Batch b(1, form, 4, 10, 50, 6, 2, 16);
    CHECK(dcptext_answerable(&b.job, 0) && dcptext_tiles(&b.job, 0) > 0);
    // a name longer than 65535 bytes
    for (int k = 0; k < 4; ++k) {
      b.name_len[k][0] = kDcpMaxName;
      CHECK(dcptext_answerable(&b.job, 0));
      b.name_len[k][0] = kDcpMaxName + 1;
      CHECK(dcptext_answerable(&b.job, 0) == (!json && k != 0));  // (the VCF reads chr1 alone)
      CHECK((dcptext_tiles(&b.job, 0) == 0) == !dcptext_answerable(&b.job, 0));
      b.name_len[k][0] = 6;
    }
    // bc_len = 0
    b.bc_len[0] = 0;
    CHECK(!dcptext_answerable(&b.job, 0));
    b.bc_len[0] = 1;
    CHECK(dcptext_answerable(&b.job, 0));
    b.bc_len[0] = 50;
    // trim_left + breakpoint at or beyond bc_len: the JSON's alone, the trim taken in 16 bits
    b.breakpoint[0] = 49; CHECK(dcptext_answerable(&b.job, 0));
    b.breakpoint[0] = 50; CHECK(dcptext_answerable(&b.job, 0) == !json);
    b.breakpoint[0] = 30; b.trim_l[0] = 19; CHECK(dcptext_answerable(&b.job, 0));
    b.trim_l[0] = 20; CHECK(dcptext_answerable(&b.job, 0) == !json);
    b.trim_l[0] = 65536 + 19; CHECK(dcptext_answerable(&b.job, 0));
    b.breakpoint[0] = 0xffffffffu; b.trim_l[0] = 1; CHECK(dcptext_answerable(&b.job, 0));  // (wraps to 0 as the writer's sum does)
    b.breakpoint[0] = 0; b.trim_l[0] = 0;
    // cols > 2^22
    for (int k = 0; k < 3; ++k) {
      b.cols[k][0] = kDcpMaxCols; CHECK(dcptext_answerable(&b.job, 0));
      b.cols[k][0] = kDcpMaxCols + 1; CHECK(dcptext_answerable(&b.job, 0) == !json);
      b.cols[k][0] = 10;
    }
    // the data's: var_n, the call index, the ranges
    std::vector<DcpChunk> chunks;
    uint32_t bad = 0;
    CHECK(dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad));
    const DcpDesc d = dcptext_desc(&b.job, &b.res, chunks[0], false, 0, 0);
    CHECK(d.flags & kDcpAnswerable);
    const DcpArgs a = b.args(&d);
    DcpView v = dcp_view(a, d);
    tracyhip_variant r{1, 1, 1, 0, 0, 8, 8, 8};
    CHECK(dcp_variant_ok(v, r));
    r.basenum = 50; CHECK(dcp_variant_ok(v, r));
    r.basenum = 51; CHECK(!dcp_variant_ok(v, r));   // forward: trim_left + basenum - 1 = bc_len
    r.basenum = 0; CHECK(!dcp_variant_ok(v, r));    // wraps
    v.forward = false;
    r.basenum = 0; CHECK(!dcp_variant_ok(v, r));    // reverse: bc_len - (trim_right + 0) = bc_len
    r.basenum = 1; CHECK(dcp_variant_ok(v, r));
    r.basenum = 50; CHECK(dcp_variant_ok(v, r));
    r.basenum = 51; CHECK(!dcp_variant_ok(v, r));
    r.basenum = 1;
    r.ref_len = 9; CHECK(dcp_variant_ok(v, r)); r.ref_off = 8; CHECK(!dcp_variant_ok(v, r)); r.ref_off = 0xffffffffu; r.ref_len = 2; CHECK(!dcp_variant_ok(v, r));
    r.ref_off = 0; r.ref_len = 16; CHECK(dcp_variant_ok(v, r));
    r.alt_off = 9; CHECK(!dcp_variant_ok(v, r)); r.alt_off = 0xfffffff8u; CHECK(!dcp_variant_ok(v, r));
    b.var_n[0] = 3;
    v = dcp_view(a, d);
    CHECK(v.var_n == 3 && v.nvar == 2);  // more than max_variants: no item reads beyond the region, the check tile says so
  }
  Batch b(1, kDcpDecomp, 4, 0, 0, 0, 1, 2);
  b.bc_len[0] = 0;
  CHECK(dcptext_answerable(&b.job, 0));  // the table reads nothing else
}

static void check_chunks() {
  for (uint32_t form = 0; form < 3; ++form) {
    Batch b(23, form, 300, 700, 90, 9, 8, 128);
    for (uint32_t t = 0; t < b.n; ++t) { b.cols[0][t] = 700 - 13 * t; b.dcp_rows[t] = 300 - 7 * t; }
    b.name_len[0][5] = kDcpMaxName + 1;  // (a trace the host can tell is deferred: it owns no tile)
    b.with_text(60000);
    std::vector<DcpChunk> one, chunks;
    uint32_t bad = 0;
    CHECK(dcptext_cut_chunks(&b.job, &b.res, true, ~0ull, one, &bad) && one.size() == 1);
    for (uint64_t limit : {1ull, 150000ull, 400000ull, 2000000ull}) {
      CHECK(dcptext_cut_chunks(&b.job, &b.res, true, limit, chunks, &bad));
      uint32_t next = 0;
      uint64_t tiles = 0;
      for (const DcpChunk& c : chunks) {
        CHECK(c.t0 == next && c.t1 > c.t0);
        next = c.t1;
        CHECK(c.t1 - c.t0 == 1 || dcptext_chunk_bytes(&b.job, c, true, true) <= limit);
        uint32_t tile_first = 0;
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          const DcpDesc d = dcptext_desc(&b.job, &b.res, c, true, t, tile_first);
          CHECK(d.tile_first == tile_first && d.text_off + d.text_cap <= c.text.size());
          if (form != kDcpVcf) CHECK(d.dcp_off + d.dcp_rows <= c.dcp.size());
          if (form == kDcpJson) CHECK(d.rows_off[0] + d.cols[0] <= c.rows[0].size() && d.rows_off[2] + d.cols[2] <= c.rows[2].size());
          if (form != kDcpDecomp) CHECK(d.bc_off + d.bc_len <= c.bc.size() && d.name_off[0] + d.name_len[0] <= c.names.size() && d.var_slot == t - c.t0 && c.var.size() == c.t1 - c.t0);
          CHECK(((d.flags & kDcpAnswerable) != 0) == (form == kDcpDecomp || t != 5));
          tile_first += dcptext_tiles(&b.job, t);
        }
        CHECK(tile_first == c.tiles);
        tiles += c.tiles;
      }
      CHECK(next == b.n && tiles == one[0].tiles);
      if (limit == 1) CHECK(chunks.size() == b.n);
      if (limit == 400000ull) CHECK(chunks.size() >= 3 && chunks.size() < b.n);
    }
    // device payloads: used in place
    CHECK(dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad) && chunks.size() == 1);
    const DcpDesc d = dcptext_desc(&b.job, &b.res, chunks[0], false, 7, 0);
    CHECK(d.text_off == b.text_off[7] && (form == kDcpVcf || d.dcp_off == b.dcp_off[7]) && (form == kDcpDecomp || (d.var_slot == 7 && d.bc_off == b.bc_off[7])));
  }
}

static void check_overflow() {
  for (uint32_t form = 0; form < 3; ++form) {
    Batch b(4, form, 4, 10, 50, 6, 2, 16);
    b.with_text(1000);
    std::vector<DcpChunk> chunks;
    uint32_t bad = 99;
    CHECK(dcptext_cut_chunks(&b.job, &b.res, true, ~0ull, chunks, &bad));
    b.text_off[2] = ~0ull - 1000;
    CHECK(dcptext_cut_chunks(&b.job, &b.res, true, ~0ull, chunks, &bad));
    b.text_off[2] = ~0ull - 999;
    CHECK(!dcptext_cut_chunks(&b.job, &b.res, true, ~0ull, chunks, &bad) && bad == 2);
    b.text_off[2] = 0;
    if (form != kDcpVcf) {
      b.dcp_off[1] = ~0ull - 3;  // (four rows)
      CHECK(!dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad) && bad == 1);
      b.dcp_off[1] = 0;
    }
    if (form != kDcpDecomp) {
      b.bc_off[3] = ~0ull - 49;
      CHECK(!dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad) && bad == 3);
      b.bc_off[3] = 0;
      b.name_off[0][0] = ~0ull - 5;
      CHECK(!dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad) && bad == 0);
      b.name_off[0][0] = 0;
    }
    if (form == kDcpJson) {
      b.rows_off[2][1] = ~0ull - 9;  // (ten columns)
      CHECK(!dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad) && bad == 1);
      b.rows_off[2][1] = 0;
      b.name_off[3][2] = ~0ull;
      CHECK(!dcptext_cut_chunks(&b.job, &b.res, false, ~0ull, chunks, &bad) && bad == 2);
    }
  }
}

static void check_validate() {
  bool range = false;
  uint32_t bad = 0;
  for (uint32_t form = 0; form < 3; ++form) {
    Batch b(3, form, 4, 10, 50, 6, 2, 16);
    auto why = [&]() { return dcptext_validate(&b.job, TRACYHIP_MEM_HOST, &b.res, &range, &bad); };
    CHECK(!why() && !range);
    CHECK(dcptext_validate(nullptr, 0, &b.res, &range, &bad) && dcptext_validate(&b.job, 0, nullptr, &range, &bad));
    CHECK(dcptext_validate(&b.job, 2, &b.res, &range, &bad) && !range);
    b.job.form = 3; CHECK(why() && !range); b.job.form = form;
    for (uint32_t mv : {0u, kDcpMaxVariants + 1}) { b.job.max_variants = mv; CHECK((why() != nullptr) == (form != kDcpDecomp) && range == (form != kDcpDecomp)); }
    b.job.max_variants = kDcpMaxVariants; CHECK(!why()); b.job.max_variants = 2;
    for (uint32_t mt : {1u, kDcpMaxText + 1}) { b.job.max_text = mt; CHECK((why() != nullptr) == (form != kDcpDecomp) && range == (form != kDcpDecomp)); }
    b.job.max_text = kDcpMaxText; CHECK(!why()); b.job.max_text = 16;
    b.dcp_rows[1] = kDcpMaxRows; CHECK(!why());
    b.dcp_rows[1] = kDcpMaxRows + 1; CHECK((why() != nullptr) == (form != kDcpVcf)); if (form != kDcpVcf) CHECK(range && bad == 1);
    b.dcp_rows[1] = 4;
    b.res.text = reinterpret_cast<uint8_t*>(&b); CHECK(why() && !range);  // a text without offsets and capacities
    b.res.text = nullptr;
    b.res.status = nullptr; CHECK(why()); b.res.status = b.status.data();
    const int32_t* keep = b.job.dcp_indel;
    b.job.dcp_indel = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(keep) + 1); CHECK((why() != nullptr) == (form != kDcpVcf));
    b.job.dcp_indel = nullptr; CHECK((why() != nullptr) == (form != kDcpVcf)); b.job.dcp_indel = keep;
    const uint8_t* r = b.job.rows1[2];
    b.job.rows1[2] = nullptr; CHECK((why() != nullptr) == (form == kDcpJson)); b.job.rows1[2] = r;
    const uint32_t* vn = b.job.var_n;
    b.job.var_n = nullptr; CHECK((why() != nullptr) == (form != kDcpDecomp)); b.job.var_n = vn;
    const uint32_t* cl = b.job.chr_len[1];
    b.job.chr_len[1] = nullptr; CHECK((why() != nullptr) == (form == kDcpJson)); b.job.chr_len[1] = cl;
    b.job.n = 0; b.job.dcp_indel = nullptr; b.job.var = nullptr; CHECK(!why());  // nothing to do
  }
}

int main() {
  check_tiles();
  check_bound_and_sinks();
  check_deferral();
  check_chunks();
  check_overflow();
  check_validate();
  if (failures) { std::printf("dcptext_plan: %d failure(s)\n", failures); return 1; }
  std::printf("dcptext_plan: ok\n");
  return 0;
}
