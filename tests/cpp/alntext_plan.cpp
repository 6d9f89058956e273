// alntext_plan.cpp -- a stand-alone run of tracy_amd/csrc/alntext_plan.h and the HIP-free parts of alntext_wave.h (no HIP, its own main;
// tests/test_emu_alntext.py builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o alntext_plan tests/cpp/alntext_plan.cpp
// It checks: the tile cut of an alignment (aln_locate walks every section once, in order, tiles of at most kAlnTile items, as many as
// aln_tiles says); the cut of the blocks into items at a linelimit that divides nothing; the owner of a tile and of a column tile among
// alignments of which some own none; the two sinks of alntext_item against each other on the extreme values, and that no item is longer
// than kAlnMaxItem; alntext_bound against the text of extreme alignments composed item by item; the deferral rule at its edges; the
// chunk cut (consecutive, covering, within the limit, descriptors inside the spans, tile numbers that follow each other); an offset
// that leaves 64 bits; the verdicts of alntext_validate and slices_validate.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../tracy_amd/csrc/alntext_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static void check_tiles() {
  for (uint32_t form = 0; form < 3; ++form)
    for (uint32_t L : {1u, 7u, 60u, 256u, 65535u})
      for (uint32_t cols : {0u, 1u, 59u, 60u, 61u, 255u, 256u, 257u, 1025u})
        for (uint32_t n0 : {0u, 300u}) {
          const AlnShape h{form, form == kAlnPlot ? L : 1u, cols, n0, 255u};
          const uint32_t tiles = aln_tiles(h);
          uint32_t k = 0;
          for (uint32_t s = 0; s < aln_nsections(form); ++s) {
            const AlnSection sec = aln_section(form, s);
            const uint32_t items = aln_items(sec, h);
            for (uint32_t i0 = 0; i0 < items; i0 += kAlnTile, ++k) {
              const AlnTileAt at = aln_locate(h, k);
              CHECK(at.sec == sec && at.i0 == i0 && at.i1 == std::min(items, i0 + kAlnTile));
            }
          }
          CHECK(k == tiles);
          CHECK(aln_locate(h, tiles).sec == AS_NONE);
          CHECK(aln_section(form, 0) == AS_CHECK && aln_items(AS_CHECK, h) == 1);
        }
  // the blocks, item by item: every (block, line, place) once, in the order of the text
  for (uint32_t L : {1u, 7u, 60u, 300u})
    for (uint32_t cols : {0u, 1u, 6u, 7u, 8u, 299u, 300u, 301u, 1025u}) {
      uint32_t k = 0;
      for (uint32_t s = 0, b = 0; s < cols; s += L, ++b) {
        const uint32_t wb = std::min(L, cols - s);
        for (uint32_t line = 0; line < 3; ++line)
          for (uint32_t p = 0; p < wb + 2; ++p, ++k) {
            const AlnBlockAt at = aln_block_at(k, cols, L);
            CHECK(at.b == b && at.s == s && at.wb == wb && at.line == line && at.p == p);
          }
      }
      CHECK(k == aln_block_items(cols, L));
      CHECK(aln_nblocks(cols, L) == (cols + L - 1) / L);
    }
  CHECK(aln_block_items(kAlnMaxCols, 1) == 9u * kAlnMaxCols);
  // owners: alignments 1, 2 and 5 own no tile
  const uint32_t first[6] = {0, 5, 5, 5, 9, 12};
  std::vector<AlnDesc> al(6);
  for (int t = 0; t < 6; ++t) al[t].tile_first = al[t].col_first = first[t];
  const uint32_t owner[12] = {0, 0, 0, 0, 0, 3, 3, 3, 3, 4, 4, 4};
  for (uint32_t k = 0; k < 12; ++k) CHECK(aln_owner_of(al.data(), 6, k) == owner[k] && aln_col_owner_of(al.data(), 6, k) == owner[k]);
}

// the whole text of one alignment, item after item, the letter counts kept by a plain loop; every item through both sinks
static std::string compose(const AlnView& v, uint32_t form) {
  const AlnShape h{form, v.L, v.cols, v.n0, v.n1};
  std::string text;
  for (uint32_t s = 0; s < aln_nsections(form); ++s) {
    const AlnSection sec = aln_section(form, s);
    uint32_t own = 0;
    for (uint32_t i = 0; i < aln_items(sec, h); ++i) {
      uint32_t aux0 = 0, aux1 = 0;
      if (sec == AS_UNG0 || sec == AS_UNG1) aux0 = own;
      if (sec == AS_BLOCKS) {
        const AlnBlockAt at = aln_block_at(i, v.cols, v.L);
        for (uint32_t j = 0; j < at.s; ++j) { aux0 += v.r0[j] != '-'; aux1 += v.r1[j] != '-'; }
      }
      RenderCount c;
      alntext_item(v, sec, i, aux0, aux1, c);
      std::vector<uint8_t> buf(c.n + 8, 0xee);
      RenderWrite w{buf.data()};
      alntext_item(v, sec, i, aux0, aux1, w);
      CHECK(w.p == buf.data() + c.n);  // the two sinks agree
      CHECK(c.n <= kAlnMaxItem);
      for (uint32_t k = c.n; k < c.n + 8; ++k) CHECK(buf[k] == 0xee);
      text.append(reinterpret_cast<const char*>(buf.data()), c.n);
      if ((sec == AS_UNG0 || sec == AS_UNG1) && i < v.cols) own += (sec == AS_UNG0 ? v.r0[i] : v.r1[i]) != '-';
    }
  }
  return text;
}

static void check_items_and_bound() {
  for (uint32_t key = 0; key < 4; ++key)
    for (uint32_t L : {1u, 7u, 60u, 65535u})
      for (uint32_t cols : {0u, 1u, 7u, 61u, 400u})
        for (int fw = 0; fw < 2; ++fw) {
          std::string r0(cols, 'A'), r1(cols, 'C'), nm0(300, 'n'), nm1(17, 'm');
          for (uint32_t j = 0; j < cols; j += 5) r0[j] = '-';
          AlnView v{};
          v.r0 = reinterpret_cast<const uint8_t*>(r0.data()); v.r1 = reinterpret_cast<const uint8_t*>(r1.data());
          v.nm0 = reinterpret_cast<const uint8_t*>(nm0.data()); v.nm1 = reinterpret_cast<const uint8_t*>(nm1.data());
          v.cols = cols; v.n0 = 300; v.n1 = 17; v.L = L; v.fald = L + 14; v.key = key;
          v.ref_pos = 2147483647 - 1 - (int32_t)cols - 1;  // the largest answered: ten digits in every counter
          v.ref_len = cols; v.score = -2147483647 - 1; v.forward = fw != 0;
          CHECK(aln_answerable(cols, 300, 17, v.ref_pos, v.ref_len));
          for (uint32_t form = 0; form < 3; ++form) {
            v.mirrored = form == kAlnPlot && !v.forward && key != 3;
            if (form != kAlnPlot && (key || L != 60)) continue;
            AlnView u = v;
            if (form != kAlnPlot) { u.L = 1; u.fald = 15; }
            if (form == kAlnJson) u.n0 = 0;
            const std::string text = compose(u, form);
            const uint64_t bound = alntext_bound(form, L, cols, u.n0, 17);
            CHECK(text.size() <= bound);
            CHECK(bound <= text.size() + 64 + 2 * (cols / 5 + cols / (L + 14) + 2) + 8 * (uint64_t)aln_nblocks(cols, L));  // (not far above: gaps, breaks, label places)
            if (form == kAlnPlot && key == 3 && cols) CHECK(text.find("Alt2214748") != std::string::npos);  // setw(9) overflowed
          }
        }
  CHECK(alntext_bound(3, 60, 10, 1, 1) == 0 && alntext_bound(kAlnPlot, 0, 10, 1, 1) == 0 && alntext_bound(kAlnPlot, 65536, 10, 1, 1) == 0);
  for (uint32_t form = 0; form < 3; ++form)
    for (uint32_t L : {1u, 60u, 65535u}) CHECK(alntext_bound(form, L, kAlnMaxCols, kAlnMaxName, kAlnMaxName) < (1ull << 31));  // text_len is 32 bits
}

static void check_deferral() {
  CHECK(aln_answerable(0, 0, 0, 0, 0));
  CHECK(aln_answerable(kAlnMaxCols, kAlnMaxName, kAlnMaxName, 0, 0) && !aln_answerable(kAlnMaxCols + 1, 0, 0, 0, 0));
  CHECK(!aln_answerable(1, kAlnMaxName + 1, 0, 0, 0) && !aln_answerable(1, 0, kAlnMaxName + 1, 0, 0));
  CHECK(!aln_answerable(1, 0, 0, -1, 0) && !aln_answerable(1, 0, 0, -2147483647 - 1, 0));
  // ref_pos + max(ref_len, cols) + 1 < 2^31
  CHECK(aln_answerable(100, 0, 0, 2147483647 - 101, 0) && !aln_answerable(100, 0, 0, 2147483647 - 100, 0));
  CHECK(aln_answerable(1, 0, 0, 2147483647 - 101, 100) && !aln_answerable(1, 0, 0, 2147483647 - 100, 100));
  CHECK(!aln_answerable(1, 0, 0, 0, 0xffffffffu) && !aln_answerable(1, 0, 0, 2147483647, 0) && aln_answerable(0, 0, 0, 2147483646, 0));
}

struct Job {
  std::vector<uint64_t> roff, n0off, n1off, toff, tcap;
  std::vector<uint32_t> cols, n0len, n1len, reflen, tlen;
  std::vector<int32_t> pos, score, status;
  std::vector<uint8_t> fwd;
  uint8_t dummy[4] = {0, 0, 0, 0};
  tracyhip_alntext_job job{};
  tracyhip_alntext_result out{};
  explicit Job(uint32_t n, uint32_t form, bool payload) {
    uint64_t r = 3, nm = 5, tx = 7;  // (nothing starts at 0 or aligned)
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t c = t % 7 == 3 ? 0 : 100 + 37 * t;
      cols.push_back(c); roff.push_back(r); r += c + (t % 3);
      n0len.push_back(t % 5); n0off.push_back(nm); nm += t % 5;
      n1len.push_back(10 + t % 4); n1off.push_back(nm); nm += 10 + t % 4 + (t % 2);
      pos.push_back(t % 11 == 5 ? -1 : (int32_t)(1000 * t)); reflen.push_back(c); fwd.push_back(t & 1); score.push_back(-(int32_t)t);
      const uint64_t cap = alntext_bound(form, 60, c, t % 5, 10 + t % 4);
      toff.push_back(tx); tcap.push_back(cap); tx += cap + (t % 4);
    }
    status.assign(n + 1, 0); tlen.assign(n + 1, 0);
    job.n = n; job.form = form; job.key = 0; job.linelimit = 60;
    job.rows0 = job.rows1 = job.names = dummy;
    job.rows_offset = roff.data(); job.cols = cols.data();
    job.name0_offset = n0off.data(); job.name0_len = n0len.data(); job.name1_offset = n1off.data(); job.name1_len = n1len.data();
    job.ref_pos = pos.data(); job.ref_len = reflen.data(); job.forward = fwd.data(); job.score = score.data();
    out.status = status.data(); out.text_len = tlen.data();
    if (payload) { out.text = dummy; out.text_offset = toff.data(); out.text_cap = tcap.data(); }
  }
};

static void check_chunks() {
  for (uint32_t form = 0; form < 3; ++form)
    for (int host = 0; host < 2; ++host)
      for (int payload = 0; payload < 2; ++payload)
        for (uint64_t limit : {uint64_t(1), uint64_t(20000), uint64_t(200000), ~uint64_t(0)}) {
          Job j(40, form, payload != 0);
          std::vector<AlnChunk> chunks;
          uint32_t bad = 99;
          CHECK(alntext_cut_chunks(&j.job, &j.out, host != 0, limit, chunks, &bad));
          CHECK(!chunks.empty() && chunks.front().t0 == 0 && chunks.back().t1 == 40);
          if (limit == ~uint64_t(0)) CHECK(chunks.size() == 1);
          if (limit == 1) CHECK(chunks.size() == 40);  // an alignment alone goes whatever it takes
          for (size_t k = 0; k < chunks.size(); ++k) {
            const AlnChunk& c = chunks[k];
            CHECK(c.t1 > c.t0);
            if (k) CHECK(c.t0 == chunks[k - 1].t1);
            if (c.t1 - c.t0 > 1) CHECK(alntext_chunk_bytes(c, host != 0, payload != 0) <= limit);
            uint32_t tile_first = 0, col_first = 0;
            for (uint32_t t = c.t0; t < c.t1; ++t) {
              const AlnDesc d = alntext_desc(&j.job, &j.out, c, host != 0, t, tile_first, col_first);
              CHECK(d.tile_first == tile_first && d.col_first == col_first);
              CHECK(((d.flags & kAlnAnswerable) != 0) == (j.pos[t] >= 0));
              CHECK(((d.flags & kAlnForward) != 0) == (j.fwd[t] != 0));
              if (!(d.flags & kAlnAnswerable)) CHECK(alntext_tiles(&j.job, t) == 0 && alntext_coltiles(&j.job, t) == 0);
              else CHECK(alntext_tiles(&j.job, t) >= aln_nsections(form) - (form == kAlnPlot && j.cols[t] == 0 ? 1u : 0u));
              if (form != kAlnPlot) CHECK(alntext_coltiles(&j.job, t) == 0);
              if (host) {
                CHECK(d.rows_off + d.cols <= c.rows.size() && d.name1_off + d.name1_len <= c.names.size() && d.name0_off + d.name0_len <= c.names.size());
                if (payload) CHECK(d.text_off + d.text_cap <= c.text.size());
              } else {
                CHECK(d.rows_off == j.roff[t] && d.name1_off == j.n1off[t]);
                if (payload) CHECK(d.text_off == j.toff[t]);
              }
              if (form == kAlnJson) CHECK(d.name0_len == 0);
              tile_first += alntext_tiles(&j.job, t);
              col_first += alntext_coltiles(&j.job, t);
            }
            CHECK(tile_first == c.tiles && col_first == c.coltiles);
          }
        }
  Job j(5, kAlnPlot, true);
  std::vector<AlnChunk> chunks;
  uint32_t bad = 99;
  j.roff[2] = ~uint64_t(0) - 5;
  CHECK(!alntext_cut_chunks(&j.job, &j.out, true, ~uint64_t(0), chunks, &bad) && bad == 2);
  j.roff[2] = 0; j.toff[1] = ~uint64_t(0);
  CHECK(!alntext_cut_chunks(&j.job, &j.out, true, ~uint64_t(0), chunks, &bad) && bad == 1);
  j.toff[1] = 0; j.n1off[4] = ~uint64_t(0) - 1;
  CHECK(!alntext_cut_chunks(&j.job, &j.out, true, ~uint64_t(0), chunks, &bad) && bad == 4);
}

static void check_validate() {
  {
    Job j(3, kAlnPlot, true);
    CHECK(alntext_validate(&j.job, TRACYHIP_MEM_HOST, &j.out) == nullptr && alntext_validate(&j.job, TRACYHIP_MEM_DEVICE, &j.out) == nullptr);
    CHECK(alntext_validate(nullptr, 0, &j.out) && alntext_validate(&j.job, 0, nullptr) && alntext_validate(&j.job, 2, &j.out));
    j.job.key = 4; CHECK(alntext_validate(&j.job, 0, &j.out)); j.job.key = 3; CHECK(!alntext_validate(&j.job, 0, &j.out));
    j.job.linelimit = 0; CHECK(alntext_validate(&j.job, 0, &j.out));
    j.job.linelimit = 65536; CHECK(alntext_validate(&j.job, 0, &j.out));
    j.job.linelimit = 65535; CHECK(!alntext_validate(&j.job, 0, &j.out));
    j.job.form = 3; CHECK(alntext_validate(&j.job, 0, &j.out));
    j.job.form = kAlnFasta; j.job.key = 9; j.job.linelimit = 0; CHECK(!alntext_validate(&j.job, 0, &j.out));  // (read by the plot alone)
    j.job.score = nullptr; CHECK(!alntext_validate(&j.job, 0, &j.out));
    j.job.form = kAlnPlot; j.job.key = 0; j.job.linelimit = 60; CHECK(alntext_validate(&j.job, 0, &j.out));
  }
  {
    Job j(3, kAlnJson, false);
    j.job.name0_offset = nullptr; j.job.name0_len = nullptr;
    CHECK(!alntext_validate(&j.job, 0, &j.out));
    j.job.form = kAlnFasta; CHECK(alntext_validate(&j.job, 0, &j.out));
    j.job.n = 0; j.job.rows0 = nullptr; CHECK(!alntext_validate(&j.job, 0, &j.out));
  }
  {
    Job j(3, kAlnPlot, true);
    j.out.text_cap = nullptr; CHECK(alntext_validate(&j.job, 0, &j.out));
    j.out.text = nullptr; CHECK(!alntext_validate(&j.job, 0, &j.out));
    j.out.status = nullptr; CHECK(alntext_validate(&j.job, 0, &j.out));
  }
  // slices
  const uint8_t refs[8] = {'A', 'C', 'G', 'T', 'a', 'x', 'N', 'n'};
  uint8_t out[16] = {0};
  const uint64_t roff[2] = {0, 4}, ooff[3] = {0, 4, 8};
  const uint32_t rlen[2] = {4, 4}, ridx[3] = {1, 0, 1}, begin[3] = {0, 1, 2}, len[3] = {4, 3, 2};
  const uint8_t fwd[3] = {1, 0, 0};
  tracyhip_slices_job s{};
  s.n = 3; s.refs = tracyhip_seqset{TRACYHIP_SEQ_CHAR, refs, roff, rlen, 2}; s.ref_index = ridx; s.forward = fwd; s.slice_begin = begin; s.slice_len = len;
  bool range = true;
  uint32_t bad = 9;
  CHECK(slices_validate(&s, 0, out, ooff, &range, &bad) == nullptr && !range);
  uint32_t len2[3] = {4, 4, 2};  // 1 + 4 > 4
  s.slice_len = len2;
  CHECK(slices_validate(&s, 0, out, ooff, &range, &bad) != nullptr && range && bad == 1);
  s.slice_len = len;
  const uint32_t ridx2[3] = {1, 2, 0};
  s.ref_index = ridx2;
  CHECK(slices_validate(&s, 0, out, ooff, &range, &bad) != nullptr && !range && bad == 1);
  s.ref_index = nullptr;  // identity: slice 2 has no reference
  CHECK(slices_validate(&s, 0, out, ooff, &range, &bad) != nullptr && !range && bad == 2);
  s.ref_index = ridx; s.refs.kind = TRACYHIP_SEQ_PROFILE;
  CHECK(slices_validate(&s, 0, out, ooff, &range, &bad) != nullptr && !range);
  s.refs.kind = TRACYHIP_SEQ_CHAR;
  CHECK(slices_validate(&s, 0, nullptr, ooff, &range, &bad) != nullptr && slices_validate(&s, 0, out, nullptr, &range, &bad) != nullptr);
  CHECK(slices_validate(&s, 3, out, ooff, &range, &bad) != nullptr && slices_validate(nullptr, 0, out, ooff, &range, &bad) != nullptr);
  const uint64_t ooff2[3] = {0, ~uint64_t(0) - 1, 8};
  CHECK(slices_validate(&s, 0, out, ooff2, &range, &bad) != nullptr && range && bad == 1);
  CHECK(slice_tiles(0) == 0 && slice_tiles(1) == 1 && slice_tiles(kSliceTile) == 1 && slice_tiles(kSliceTile + 1) == 2);
  CHECK(slice_complement('a') == 'T' && slice_complement('C') == 'G' && slice_complement('n') == 'N' && slice_complement('x') == 0 && slice_complement('-') == 0);
}

int main() {
  check_tiles();
  check_items_and_bound();
  check_deferral();
  check_chunks();
  check_validate();
  if (failures) { std::printf("alntext_plan: %d failures\n", failures); return 1; }
  std::printf("alntext_plan: ok\n");
  return 0;
}
