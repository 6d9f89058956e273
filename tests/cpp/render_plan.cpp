// render_plan.cpp -- a stand-alone run of tracy_amd/csrc/render_plan.h and the HIP-free parts of render_wave.h (no HIP, its own main;
// tests/test_emu_render.py builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o render_plan tests/cpp/render_plan.cpp
// It checks: the tile cut of a trace (render_locate walks every section once, in order, tiles of at most kRenderTile items, as many as
// render_tiles says); the owner of a tile among traces of which some own none; the two sinks of render_item against each other and
// against snprintf on the extreme values, and that no item is longer than kRenderMaxItem; render_bound against the longest text a
// trace of its sizes can have; the chunk cut (consecutive, covering, within the limit, descriptors inside the spans, tile numbers that
// follow each other); an offset that leaves 64 bits; render_validate's verdicts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../tracy_amd/csrc/render_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static void check_tiles() {
  for (uint32_t form = 0; form < 3; ++form)
    for (uint32_t ns : {1u, 63u, 255u, 256u, 257u, 513u, 10001u})
      for (uint32_t n : {1u, 2u, 256u, 257u, 700u}) {
        const uint32_t tiles = render_tiles(form, ns, n);
        uint32_t k = 0;
        for (uint32_t s = 0; s < render_nsections(form); ++s) {
          const RenderSection sec = render_section(form, s);
          const uint32_t items = render_items(sec, ns, n);
          CHECK(items >= 1);
          for (uint32_t i0 = 0; i0 < items; i0 += kRenderTile, ++k) {
            const RenderTileAt at = render_locate(form, ns, n, k);
            CHECK(at.sec == sec && at.i0 == i0 && at.i1 == std::min(items, i0 + kRenderTile));
          }
        }
        CHECK(k == tiles);
        CHECK(render_locate(form, ns, n, tiles).sec == RS_NONE);
        CHECK(render_section(form, 0) == RS_CHECK && render_tiles_of(n) == render_tiles_of(render_items(RS_CHECK, ns, n)));
      }
  // owners: traces 1, 2 and 5 own no tile
  const uint32_t first[6] = {0, 5, 5, 5, 9, 12};
  std::vector<RenderTrace> tr(6);
  for (int t = 0; t < 6; ++t) tr[t].tile_first = first[t];
  const uint32_t owner[12] = {0, 0, 0, 0, 0, 3, 3, 3, 3, 4, 4, 4};
  for (uint32_t k = 0; k < 12; ++k) CHECK(render_trace_of(tr.data(), 6, k) == owner[k]);
}

struct Arrays {
  std::vector<int32_t> sig, pos;
  std::vector<uint8_t> pri, sec, con, q;
  RenderView view(uint32_t ns, uint32_t n, uint32_t l, uint32_t r) {
    RenderView v;
    v.signal = sig.data(); v.sig_off = 0; v.pos = pos.data();
    v.pri = pri.data(); v.sec = sec.data(); v.con = con.data(); v.q = q.data();
    v.ns = ns; v.n = n; v.trim_l = l; v.keep_until = r < n ? n - r : 0;
    return v;
  }
};

static std::string item_text(const RenderView& v, RenderSection sec, uint32_t i, uint32_t aux) {
  RenderCount c;
  render_item<false>(v, sec, i, aux, c);
  std::vector<uint8_t> buf(c.n + 8, 0xee);
  RenderWrite w{buf.data()};
  render_item<false>(v, sec, i, aux, w);
  CHECK(w.p == buf.data() + c.n);          // the two sinks agree
  CHECK(buf[c.n] == 0xee);                 // and the writer stops there
  CHECK(c.n <= kRenderMaxItem);
  return std::string(reinterpret_cast<const char*>(buf.data()), c.n);
}

static void check_items() {
  // numbers against snprintf
  for (int64_t x : {0ll, 9ll, 10ll, 99ll, 100ll, 999ll, 1000ll, 9999ll, 10000ll, 32767ll, 99999ll, 100000ll, 999999999ll, 1000000000ll, 2147483647ll,
                    -1ll, -9ll, -10ll, -99ll, -32768ll, -2147483648ll}) {
    char want[16];
    const int len = std::snprintf(want, sizeof(want), "%lld", (long long)x);
    RenderCount c; c.num((int32_t)x);
    uint8_t got[16];
    RenderWrite w{got}; w.num((int32_t)x);
    CHECK((int)c.n == len && w.p == got + len && std::memcmp(got, want, (size_t)len) == 0);
  }
  // the longest items: the largest sample number, the most negative values, the largest call number, a three-digit quality
  Arrays a;
  a.sig.assign(4, INT32_MIN); a.pos.assign(1, 0); a.pri = {'A'}; a.sec = {'R'}; a.con = {'N'}; a.q = {255};
  {
    RenderView s = a.view(1, 1, 0, 0);
    const std::string line = item_text(s, RS_SAMPLES, 0, 1);
    CHECK(line == "1\t-2147483648\t-2147483648\t-2147483648\t-2147483648\t1\tA\tR\tN\t255\tN\n");
    // the same line with the largest sample and call numbers is longer by their digits: 7 and 6 instead of 1 and 1
    CHECK(line.size() + 6 + 5 <= kRenderMaxItem);
    CHECK(item_text(s, RS_SAMPLES, 0, 0) == "1\t-2147483648\t-2147483648\t-2147483648\t-2147483648\tNA\tNA\tNA\tNA\tNA\tNA\n");
    CHECK(item_text(s, RS_HEADER, 0, 0) == "pos\tpeakA\tpeakC\tpeakG\tpeakT\tbasenum\tprimary\tsecondary\tconsensus\tqual\ttrim\n");
    CHECK(item_text(s, RS_POS, 0, 0) == "\"pos\": [1],\n");
    CHECK(item_text(s, RS_PEAK_G, 0, 0) == "\"peakG\": [-2147483648],\n");
    CHECK(item_text(s, RS_BCPOS, 0, 0) == "\"basecallPos\": [1],\n" && item_text(s, RS_BCQUAL, 0, 0) == "\"basecallQual\": [255],\n");
    CHECK(item_text(s, RS_CALLS, 0, 0) == "\"basecalls\": {\"1\":\"1:A|A|G\"},\n");
    CHECK(item_text(s, RS_CALLS_GAPPED, 0, 1) == "\"basecalls\": {\"1\":\"1:A|R\"}\n");
    CHECK(item_text(s, RS_PRISEQ, 0, 0) == "\"primarySeq\": \"A\",\n" && item_text(s, RS_SECSEQ, 0, 0) == "\"secondarySeq\": \"R\"\n");
    // a position that is not one (the trace is deferred, its items are still measured): eleven characters, still within the image
    std::vector<int32_t> wild(1, INT32_MIN + 5);
    s.pos = wild.data();
    CHECK(item_text(s, RS_CALLS, 0, 0) == "\"basecalls\": {\"-2147483642\":\"1:A|A|G\"},\n");
    wild[0] = INT32_MAX;  // + 1 wraps in unsigned arithmetic
    CHECK(item_text(s, RS_BCPOS, 0, 0) == "\"basecallPos\": [-2147483648],\n");
  }
  // a small trace, every section against a text composed here
  {
    Arrays b;
    const uint32_t bns = 5, bn = 3;
    for (uint32_t k = 0; k < 4; ++k)
      for (uint32_t i = 0; i < bns; ++i) b.sig.push_back((int32_t)(k * 100 + i) - 150);
    b.pos = {0, 2, 4}; b.pri = {'A', '-', 'T'}; b.sec = {'A', '-', 'Q'}; b.con = {'A', 'C', 'G'}; b.q = {0, 9, 100};
    const RenderView bv = b.view(bns, bn, 1, 1);
    auto section = [&](RenderSection sec, const uint32_t* aux) {
      std::string s;
      for (uint32_t i = 0; i < render_items(sec, bns, bn); ++i) s += item_text(bv, sec, i, aux ? aux[i] : 0);
      return s;
    };
    const uint32_t at[5] = {1, 0, 2, 0, 3}, gapless[3] = {1, 0, 2};
    CHECK(section(RS_SAMPLES, at) ==
          "1\t-150\t-50\t50\t150\t1\tA\tA\tA\t0\tY\n2\t-149\t-49\t51\t151\tNA\tNA\tNA\tNA\tNA\tNA\n3\t-148\t-48\t52\t152\t2\t-\t-\tC\t9\tN\n"
          "4\t-147\t-47\t53\t153\tNA\tNA\tNA\tNA\tNA\tNA\n5\t-146\t-46\t54\t154\t3\tT\tQ\tG\t100\tY\n");
    CHECK(section(RS_POS, nullptr) == "\"pos\": [1, 2, 3, 4, 5],\n");
    CHECK(section(RS_PEAK_C, nullptr) == "\"peakC\": [-50, -49, -48, -47, -46],\n");
    CHECK(section(RS_BCPOS, nullptr) == "\"basecallPos\": [1, 3, 5],\n" && section(RS_BCQUAL, nullptr) == "\"basecallQual\": [0, 9, 100],\n");
    CHECK(section(RS_CALLS, nullptr) == "\"basecalls\": {\"1\":\"1:A\", \"3\":\"2:-\", \"5\":\"3:T|N\"},\n");
    CHECK(section(RS_CALLS_GAPPED, gapless) == "\"basecalls\": {\"1\":\"1:A\", \"3\":\"-\", \"5\":\"2:T|Q\"}\n");
    CHECK(section(RS_PRISEQ, nullptr) == "\"primarySeq\": \"A-T\",\n" && section(RS_SECSEQ, nullptr) == "\"secondarySeq\": \"A-Q\"\n");
  }
}

// the longest text of a trace of these sizes: every value the most negative, every sample number and call number as printed, every
// quality 255, secondaries that expand to three characters; calls on the last n samples
static uint64_t longest(uint32_t form, uint32_t ns, uint32_t n, uint32_t sb) {
  Arrays a;
  a.sig.assign(4ull * ns, sb == 2 ? -32768 : INT32_MIN);
  for (uint32_t c = 0; c < n; ++c) a.pos.push_back((int32_t)(ns - n + c));
  a.pri.assign(n, 'A'); a.sec.assign(n, 'R'); a.con.assign(n, 'A'); a.q.assign(n, 255);
  const RenderView v = a.view(ns, n, 0, 0);
  uint64_t total = 0;
  for (uint32_t s = 1; s < render_nsections(form); ++s) {
    const RenderSection sec = render_section(form, s);
    for (uint32_t i = 0; i < render_items(sec, ns, n); ++i) {
      uint32_t aux = 0;
      if (sec == RS_SAMPLES) aux = i >= ns - n ? i - (ns - n) + 1 : 0;
      if (sec == RS_CALLS_GAPPED) aux = i + 1;
      RenderCount c;
      render_item<false>(v, sec, i, aux, c);
      total += c.n;
    }
  }
  return total;
}

static void check_bound() {
  for (uint32_t form = 0; form < 3; ++form)
    for (uint32_t sb : {2u, 4u})
      for (uint32_t ns : {1u, 9u, 10u, 99u, 100u, 1000u, 10001u, 100002u}) {
        for (uint32_t n : {1u, 9u, 10u, 100u, 1000u}) {
          if (n > ns) continue;
          const uint64_t b = render_bound(form, ns, n, sb), worst = longest(form, ns, n, sb);
          CHECK(b >= worst);
          CHECK(b <= 2 * worst + 256);  // (and is no wild guess)
        }
      }
  CHECK(render_bound(3, 10, 10, 4) == 0);
  // inside the answered domain every text stays below 2^31 bytes: the sums of render_scan_body are 32-bit
  for (uint32_t form = 0; form < 3; ++form) CHECK(render_bound(form, kRenderMaxSamples, kRenderMaxCalls, 4) < (1ull << 31));
}

struct Batch {
  std::vector<uint64_t> sig_off, bc_off, text_off, text_cap;
  std::vector<uint32_t> ns, bc_len, tl, tr;
  tracyhip_render_job job{};
  tracyhip_render_result out{};
  std::vector<int32_t> status;
  std::vector<uint32_t> text_len;
  Batch(uint32_t n, uint32_t form, bool payload, bool trims) {
    uint64_t so = 3, bo = 1, to = 5;
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t calls = t % 11 == 5 ? 0 : 1 + (t * 37u) % 900u, samples = t % 13 == 7 ? 0 : 12u * calls + 5 + t % 3;
      ns.push_back(samples); bc_len.push_back(calls);
      tl.push_back(t % 4); tr.push_back(t % 3);
      sig_off.push_back(so); bc_off.push_back(bo); text_off.push_back(to);
      text_cap.push_back(render_bound(form, samples, calls, 4) + t % 3);
      so += 4ull * samples + t % 2; bo += calls + t % 5; to += text_cap.back() + t % 7;
    }
    static int32_t dummy32[4];
    static uint8_t dummy8[4];
    job.ntraces = n; job.form = form;
    job.signal = dummy32; job.signal_offset = sig_off.data(); job.nsamples = ns.data(); job.sample_bytes = 4;
    job.bcpos = dummy32; job.primary = job.secondary = job.consensus = job.estqual = dummy8;
    job.bc_offset = bc_off.data(); job.bc_len = bc_len.data();
    if (trims) { job.trim_left_each = tl.data(); job.trim_right_each = tr.data(); }
    status.assign(n, 0); text_len.assign(n, 0);
    out.status = status.data(); out.text_len = text_len.data();
    if (payload) { out.text = dummy8; out.text_offset = text_off.data(); out.text_cap = text_cap.data(); }
  }
};

static bool inside(const Span& s, uint64_t off, uint64_t len) { return len == 0 || (off >= s.lo && off + len <= s.hi); }

static void check_cut(uint32_t n, uint32_t form, bool payload, bool trims, bool host, uint64_t limit, size_t min_chunks) {
  Batch b(n, form, payload, trims);
  CHECK(render_validate(&b.job, host ? TRACYHIP_MEM_HOST : TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
  std::vector<RenderChunk> chunks;
  uint32_t bad = ~0u;
  CHECK(render_cut_chunks(&b.job, &b.out, host, limit, chunks, &bad));
  CHECK(chunks.size() >= min_chunks);
  uint32_t at = 0;
  for (const RenderChunk& c : chunks) {
    CHECK(c.t0 == at && c.t1 > c.t0 && c.t1 <= n);
    at = c.t1;
    if (c.t1 - c.t0 > 1) CHECK(render_chunk_bytes(c, 4, host, form == 0, payload) <= limit);
    uint32_t tile = 0;
    for (uint32_t t = c.t0; t < c.t1; ++t) {
      const RenderTrace d = render_trace_desc(&b.job, &b.out, c, host, t, tile);
      const bool ans = render_answerable(b.ns[t], b.bc_len[t]);
      CHECK(d.tile_first == tile && d.answerable == (ans ? 1u : 0u));
      CHECK(render_trace_tiles(&b.job, t) == (ans ? render_tiles(form, b.ns[t], b.bc_len[t]) : 0u));
      tile += render_trace_tiles(&b.job, t);
      CHECK(d.nsamples == b.ns[t] && d.bc_len == b.bc_len[t] && d.trim_l == (trims ? b.tl[t] : 0u) && d.trim_r == (trims ? b.tr[t] : 0u));
      CHECK(inside(c.sig, b.sig_off[t], 4ull * b.ns[t]) && inside(c.bc, b.bc_off[t], b.bc_len[t]));
      CHECK(d.sig_off + (host ? c.sig.lo : 0) == b.sig_off[t] && d.bc_off + (host ? c.bc.lo : 0) == b.bc_off[t]);
      if (payload) {
        CHECK(inside(c.text, b.text_off[t], b.text_cap[t]));
        CHECK(d.text_off + (host ? c.text.lo : 0) == b.text_off[t] && d.text_cap == b.text_cap[t]);
      } else {
        CHECK(d.text_off == 0 && d.text_cap == 0);
      }
    }
    CHECK(tile == c.tiles);
  }
  CHECK(at == n);
}

static void check_validate() {
  for (uint32_t form = 0; form < 3; ++form) {
    Batch b(5, form, true, true);
    CHECK(render_validate(&b.job, TRACYHIP_MEM_HOST, &b.out) == nullptr && render_validate(&b.job, TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
    CHECK(render_validate(nullptr, 0, &b.out) && render_validate(&b.job, 0, nullptr) && render_validate(&b.job, 2, &b.out));
    { Batch c(5, form, true, true); c.job.form = 3; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.job.sample_bytes = 3; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.job.trim_right_each = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.job.signal = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, false, true); c.job.signal = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }  // the sizes-only form reads the chromatogram too
    { Batch c(5, form, true, true); c.job.estqual = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.job.bc_len = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.out.text_len = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.out.text_cap = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.out.text_offset = nullptr; CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.job.consensus = nullptr; CHECK((render_validate(&c.job, 0, &c.out) != nullptr) == (form == 0)); }  // read by the TSV alone
    { Batch c(5, form, true, true); c.job.bcpos = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(c.job.bcpos) + 2); CHECK(render_validate(&c.job, 0, &c.out)); }
    { Batch c(5, form, true, true); c.job.ntraces = 0; c.job.signal = nullptr; CHECK(render_validate(&c.job, 0, &c.out) == nullptr); }  // an empty batch
  }
  // an offset + length that leaves 64 bits
  Batch w(9, 1, true, false);
  w.text_off[6] = ~0ull - 8;
  std::vector<RenderChunk> chunks;
  uint32_t bad = ~0u;
  CHECK(!render_cut_chunks(&w.job, &w.out, true, 1ull << 30, chunks, &bad) && bad == 6);
}

int main() {
  check_tiles();
  check_items();
  check_bound();
  for (uint32_t n : {1u, 3u, 4u, 5u, 64u, 257u})
    for (uint32_t form = 0; form < 3; ++form)
      for (int payload = 0; payload < 2; ++payload)
        for (int host = 0; host < 2; ++host) {
          check_cut(n, form, payload, payload, host, ~0ull, 1);
          check_cut(n, form, payload, !payload, host, 1ull << 20, 1);
          check_cut(n, form, payload, true, host, 1, host ? n : 1);  // host payloads: every trace alone (each stages its span of the calls)
        }
  check_cut(257, 0, true, true, true, 1ull << 20, 4);
  check_validate();
  if (failures) { std::printf("render_plan: %d failures\n", failures); return 1; }
  std::printf("render_plan: ok\n");
  return 0;
}
