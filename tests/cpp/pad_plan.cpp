// pad_plan.cpp -- a stand-alone run of tracy_amd/csrc/pad_plan.h (no HIP, its own main; tests/test_emu_pad.py builds it plain and with the
// sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o pad_plan tests/cpp/pad_plan.cpp
// It cuts batches of 1 .. 257 traces of mixed sizes under several limits, for host and device payloads and for the sizes-only form, and
// checks: the chunks are consecutive and cover every trace once, a chunk of more than one trace fits the limit, the spans hold every
// region of the chunk's traces, the descriptors point inside the spans (host) or at the caller's offsets (device), the scratch regions
// of a chunk follow each other without overlap and are empty for traces the sizes alone defer; an offset that leaves 64 bits is refused;
// and pad_validate's verdicts.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tracy_amd/csrc/pad_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

struct Batch {
  std::vector<uint64_t> sig_off, bc_off, row_off, osig_off, ocall_off;
  std::vector<uint32_t> ns, bc_len, row_len, tl, tr, scap, ccap;
  std::vector<uint8_t> rev;
  tracyhip_pad_job job{};
  tracyhip_pad_result out{};
  std::vector<int32_t> status;
  std::vector<uint32_t> meta[5];
  explicit Batch(uint32_t n, bool payload, bool trims) {
    uint64_t so = 3, bo = 1, ro = 7, oso = 4, oco = 2;
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t calls = t % 11 == 5 ? 0 : 1 + (t * 37u) % 900u, samples = 12u * calls + 5 + t % 3, cols = calls + (t * 13u) % 50u;
      ns.push_back(samples); bc_len.push_back(calls); row_len.push_back(cols);
      tl.push_back(t % 4 == 1 ? calls / 3 : 0); tr.push_back(t % 7 == 3 ? calls : t % 4 == 2 ? calls / 4 : 0);  // (t % 7 == 3: trims take all)
      rev.push_back(t % 3 == 0);
      sig_off.push_back(so); bc_off.push_back(bo); row_off.push_back(ro);
      so += 4ull * samples + t % 2; bo += calls + t % 5; ro += cols;
      scap.push_back(samples + 6 * cols); ccap.push_back(calls + cols);
      osig_off.push_back(oso); ocall_off.push_back(oco);
      oso += 4ull * scap.back(); oco += ccap.back();
    }
    static int32_t dummy32[4];
    static uint8_t dummy8[4];
    job.ntraces = n;
    job.signal = dummy32; job.signal_offset = sig_off.data(); job.nsamples = ns.data(); job.sample_bytes = 4;
    job.bcpos = dummy32; job.primary = job.secondary = job.consensus = job.estqual = dummy8;
    job.bc_offset = bc_off.data(); job.bc_len = bc_len.data();
    job.rows = dummy8; job.row_offset = row_off.data(); job.row_len = row_len.data();
    if (trims) { job.trim_left_each = tl.data(); job.trim_right_each = tr.data(); }
    job.reverse = rev.data();
    status.assign(n, 0);
    for (auto& m : meta) m.assign(n, 0);
    out.status = status.data(); out.nsamples_out = meta[0].data(); out.ncalls_out = meta[1].data(); out.leading_gaps = meta[2].data();
    out.trailing_gaps = meta[3].data(); out.step = meta[4].data();
    if (payload) {
      out.signal = dummy32; out.sample_offset = osig_off.data(); out.sample_cap = scap.data();
      out.bcpos = dummy32; out.primary = out.secondary = out.consensus = out.estqual = dummy8;
      out.call_offset = ocall_off.data(); out.call_cap = ccap.data();
    }
  }
};

static bool inside(const PadSpan& s, uint64_t off, uint64_t len) { return len == 0 || (off >= s.lo && off + len <= s.hi); }

static void check_cut(uint32_t n, bool payload, bool trims, bool host, uint64_t limit, size_t min_chunks) {
  Batch b(n, payload, trims);
  CHECK(pad_validate(&b.job, host ? TRACYHIP_MEM_HOST : TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
  std::vector<PadChunk> chunks;
  uint32_t bad = ~0u;
  CHECK(pad_cut_chunks(&b.job, &b.out, host, limit, chunks, &bad));
  CHECK(chunks.size() >= min_chunks);
  uint32_t at = 0;
  for (const PadChunk& c : chunks) {
    CHECK(c.t0 == at && c.t1 > c.t0 && c.t1 <= n);
    at = c.t1;
    if (c.t1 - c.t0 > 1) CHECK(pad_chunk_bytes(c, 4, host, payload, payload) <= limit);
    uint64_t scratch = 0;
    for (uint32_t t = c.t0; t < c.t1; ++t) {
      const PadTrace d = pad_trace_desc(&b.job, &b.out, c, host, t, scratch);
      const uint64_t w = payload ? pad_scratch_words(&b.job, t) : 0;
      const uint32_t l = trims ? b.tl[t] : 0, r = trims ? b.tr[t] : 0;
      if (!pad_sizes_answerable(b.ns[t], b.bc_len[t], l, r)) CHECK(w == 0);
      else if (payload) CHECK(w == (uint64_t)kPadInsWords * pad_max_inserts(b.bc_len[t] - l - r, b.row_len[t]));
      CHECK(d.scratch_off == scratch);
      scratch += w;
      CHECK(d.nsamples == b.ns[t] && d.bc_len == b.bc_len[t] && d.row_len == b.row_len[t] && d.trim_l == l && d.trim_r == r && d.reverse == b.rev[t]);
      CHECK(inside(c.bc, b.bc_off[t], b.bc_len[t]) && inside(c.row, b.row_off[t], b.row_len[t]));
      const uint64_t base_bc = host ? c.bc.lo : 0, base_row = host ? c.row.lo : 0;
      CHECK(d.bc_off + base_bc == b.bc_off[t] && d.row_off + base_row == b.row_off[t]);
      if (payload) {
        CHECK(inside(c.sig, b.sig_off[t], 4ull * b.ns[t]) && inside(c.osig, b.osig_off[t], 4ull * b.scap[t]) && inside(c.ocall, b.ocall_off[t], b.ccap[t]));
        CHECK(d.sig_off + (host ? c.sig.lo : 0) == b.sig_off[t] && d.out_sig_off + (host ? c.osig.lo : 0) == b.osig_off[t] &&
              d.out_call_off + (host ? c.ocall.lo : 0) == b.ocall_off[t]);
        CHECK(d.sample_cap == b.scap[t] && d.call_cap == b.ccap[t]);
      } else {
        CHECK(d.sig_off == 0 && d.out_sig_off == 0 && d.out_call_off == 0 && d.sample_cap == 0 && d.call_cap == 0);
      }
    }
    CHECK(scratch == c.scratch_words);
  }
  CHECK(at == n);
}

static void check_validate() {
  Batch b(5, true, true);
  CHECK(pad_validate(&b.job, TRACYHIP_MEM_HOST, &b.out) == nullptr && pad_validate(&b.job, TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
  CHECK(pad_validate(nullptr, 0, &b.out) && pad_validate(&b.job, 0, nullptr) && pad_validate(&b.job, 2, &b.out));
  { Batch c(5, true, true); c.job.sample_bytes = 3; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.job.trim_right_each = nullptr; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.job.row_len = nullptr; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.out.step = nullptr; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.out.sample_cap = nullptr; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.out.call_offset = nullptr; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.job.estqual = nullptr; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.job.signal = nullptr; CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true, true); c.job.bcpos = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(c.job.bcpos) + 2); CHECK(pad_validate(&c.job, 0, &c.out)); }
  { Batch c(5, false, false); c.job.signal = nullptr; c.job.signal_offset = nullptr; CHECK(pad_validate(&c.job, 0, &c.out) == nullptr); }  // sizes only
  { Batch c(5, true, true); c.job.ntraces = 0; c.job.rows = nullptr; CHECK(pad_validate(&c.job, 0, &c.out) == nullptr); }           // an empty batch
  // an offset + length that leaves 64 bits
  Batch w(9, true, false);
  w.osig_off[6] = ~0ull - 8;
  std::vector<PadChunk> chunks;
  uint32_t bad = ~0u;
  CHECK(!pad_cut_chunks(&w.job, &w.out, true, 1ull << 30, chunks, &bad) && bad == 6);
}

int main() {
  for (uint32_t n : {1u, 3u, 4u, 5u, 64u, 257u})
    for (int payload = 0; payload < 2; ++payload)
      for (int trims = 0; trims < 2; ++trims)
        for (int host = 0; host < 2; ++host) {
          check_cut(n, payload, trims, host, ~0ull, 1);
          check_cut(n, payload, trims, host, 1ull << 20, 1);
          check_cut(n, payload, trims, host, 1, host ? n : 1);  // host payloads: every trace alone (each stages its calls and its row)
        }
  check_cut(257, true, true, true, 1ull << 20, 4);
  check_validate();
  if (failures) { std::printf("pad_plan: %d failures\n", failures); return 1; }
  std::printf("pad_plan: ok\n");
  return 0;
}
