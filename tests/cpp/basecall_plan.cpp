// basecall_plan.cpp -- a stand-alone run of tracy_amd/csrc/basecall_plan.h and ragged_plan.h (no HIP, its own main;
// tests/test_emu_basecall.py builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o basecall_plan tests/cpp/basecall_plan.cpp
// 1. It cuts batches of 1 .. 257 traces of mixed sizes (some without positions, some with fewer than 3 samples, some beyond kBcMaxPos)
//    under several limits, for host and device payloads, and checks: the chunks are consecutive and cover every trace once, a chunk of
//    more than one trace fits the limit, with limit 1 and host payloads every trace is alone, the spans hold every region, the
//    descriptors point inside the spans (host) or at the caller's offsets (device), the scratch regions of a chunk follow each other
//    without overlap and are empty for traces the sizes alone defer.
// 2. An offset that leaves 64 bits is refused with the trace's index; basecall_validate's verdicts, one check per message.
// 3. RunMerger with a functor that records its triples: over 300 traces with random region lengths, gaps on either side, both or
//    neither, and traces that report fewer entries than their region holds or none, the union of the triples of each array is exactly
//    the reported entries of every trace -- each byte once, nothing outside -- and two traces contiguous on both sides and fully
//    reported give one triple.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../tracy_amd/csrc/basecall_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

struct Batch {
  std::vector<uint64_t> sig_off, pos_off;
  std::vector<uint32_t> ns, np;
  tracyhip_basecall_job job{};
  tracyhip_basecall_result out{};
  std::vector<int32_t> status;
  std::vector<uint32_t> meta[4];
  explicit Batch(uint32_t n) {
    uint64_t so = 3, po = 1;
    for (uint32_t t = 0; t < n; ++t) {
      uint32_t calls = t % 11 == 5 ? 0 : 1 + (t * 37u) % 900u;  // (t % 11 == 5: no positions)
      if (t % 29 == 8) calls = kBcMaxPos + 1 + t;               // more than the device answers
      const uint32_t samples = t % 13 == 4 ? t % 3 : 12u * (calls % 4096u) + 5 + t % 3;  // (t % 13 == 4: fewer than 3 samples)
      ns.push_back(samples); np.push_back(calls);
      sig_off.push_back(so); pos_off.push_back(po);
      so += 4ull * samples + t % 2; po += calls + t % 5;
    }
    static int32_t dummy32[4];
    job.ntraces = n;
    job.signal = dummy32; job.signal_offset = sig_off.data(); job.nsamples = ns.data(); job.sample_bytes = 4;
    job.basecallpos = dummy32; job.pos_offset = pos_off.data(); job.npos = np.data();
    job.sigratio = 0.33f; job.trim_stringency = 0;
    status.assign(n, 0);
    for (auto& m : meta) m.assign(n, 0);
    out.status = status.data(); out.bc_len = meta[0].data(); out.trim_left = meta[1].data(); out.trim_right = meta[2].data();
    out.best_section = meta[3].data();
  }
};

static bool inside(const Span& s, uint64_t off, uint64_t len) { return len == 0 || (off >= s.lo && off + len <= s.hi); }

static void check_cut(uint32_t n, uint32_t sb, bool host, uint64_t limit, size_t min_chunks) {
  Batch b(n);
  b.job.sample_bytes = sb;
  CHECK(basecall_validate(&b.job, host ? TRACYHIP_MEM_HOST : TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
  std::vector<BasecallChunk> chunks;
  uint32_t bad = ~0u;
  CHECK(basecall_cut_chunks(&b.job, host, limit, chunks, &bad));
  CHECK(chunks.size() >= min_chunks);
  if (!host) CHECK(chunks.size() == 1);
  uint32_t at = 0;
  for (const BasecallChunk& c : chunks) {
    CHECK(c.t0 == at && c.t1 > c.t0 && c.t1 <= n);
    at = c.t1;
    if (host && c.t1 - c.t0 > 1) CHECK(c.sig.size() * sb <= limit);
    if (host && c.t1 < n) CHECK(c.sig.with(b.sig_off[c.t1], 4ull * b.ns[c.t1]).size() * sb > limit);  // (it closed for a reason)
    uint64_t scratch = 0;
    for (uint32_t t = c.t0; t < c.t1; ++t) {
      const BasecallTrace d = basecall_trace_desc(&b.job, c, host, t, scratch);
      const uint64_t w = basecall_scratch_words(&b.job, t);
      const bool answerable = b.np[t] >= 1 && b.np[t] <= kBcMaxPos && b.ns[t] >= 3 && b.ns[t] <= kBcMaxSamples;
      CHECK(w == (answerable ? 3ull * b.np[t] + 1 : 0));
      CHECK(d.scratch_off == scratch);
      scratch += w;
      CHECK(d.nsamples == b.ns[t] && d.npos == b.np[t]);
      CHECK(inside(c.sig, b.sig_off[t], 4ull * b.ns[t]) && inside(c.pos, b.pos_off[t], b.np[t]));
      CHECK(d.sig_off + (host ? c.sig.lo : 0) == b.sig_off[t] && d.pos_off + (host ? c.pos.lo : 0) == b.pos_off[t]);
    }
  }
  CHECK(at == n);
}

static void check_validate() {
  const char* why;
  auto is = [&](const char* msg) { return why && std::strcmp(why, msg) == 0; };
  Batch b(5);
  CHECK(basecall_validate(&b.job, TRACYHIP_MEM_HOST, &b.out) == nullptr && basecall_validate(&b.job, TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
  why = basecall_validate(nullptr, 0, &b.out); CHECK(is("null job / result"));
  why = basecall_validate(&b.job, 0, nullptr); CHECK(is("null job / result"));
  why = basecall_validate(&b.job, 2, &b.out); CHECK(is("bad mem"));
  { Batch c(5); c.job.sample_bytes = 3; why = basecall_validate(&c.job, 0, &c.out); CHECK(is("sample_bytes must be 2 or 4")); }
  { Batch c(5); c.job.sigratio = std::nanf(""); why = basecall_validate(&c.job, 0, &c.out); CHECK(is("sigratio is not a number")); }
  { Batch c(5); c.job.trim_stringency = std::nanf(""); why = basecall_validate(&c.job, 0, &c.out); CHECK(is("trim_stringency must be 0 or positive")); }
  { Batch c(5); c.job.trim_stringency = -1; why = basecall_validate(&c.job, 0, &c.out); CHECK(is("trim_stringency must be 0 or positive")); }
  { Batch c(5); c.job.npos = nullptr; why = basecall_validate(&c.job, 0, &c.out); CHECK(is("null signal / basecallpos or one of their offset and length arrays")); }
  { Batch c(5); c.job.signal = nullptr; why = basecall_validate(&c.job, 0, &c.out); CHECK(is("null signal / basecallpos or one of their offset and length arrays")); }
  { Batch c(5); c.job.sample_bytes = 2; c.job.signal = reinterpret_cast<const char*>(c.job.signal) + 1; why = basecall_validate(&c.job, 0, &c.out);
    CHECK(is("signal / basecallpos not aligned to their element size")); }
  { Batch c(5); c.job.basecallpos = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(c.job.basecallpos) + 2); why = basecall_validate(&c.job, 0, &c.out);
    CHECK(is("signal / basecallpos not aligned to their element size")); }
  { Batch c(5); c.out.best_section = nullptr; why = basecall_validate(&c.job, 0, &c.out);
    CHECK(is("null per-trace result array (status, bc_len, trim_left, trim_right, best_section)")); }
  { Batch c(5); c.job.ntraces = 0; c.job.signal = nullptr; c.out.status = nullptr; CHECK(basecall_validate(&c.job, 0, &c.out) == nullptr); }  // an empty batch
  // an offset + length that leaves 64 bits: the chromatogram's, the positions', host and device payloads
  for (int host = 0; host < 2; ++host) {
    std::vector<BasecallChunk> chunks;
    uint32_t bad = ~0u;
    Batch s(9);
    s.sig_off[6] = ~0ull - 8;
    CHECK(!basecall_cut_chunks(&s.job, host, 1ull << 30, chunks, &bad) && bad == 6);
    Batch p(9);
    p.pos_off[3] = ~0ull - 8;
    bad = ~0u;
    CHECK(!basecall_cut_chunks(&p.job, host, 1ull << 30, chunks, &bad) && bad == 3);
    Batch ok(9);  // the last element may end at 2^64 - 1
    ok.pos_off[8] = ~0ull - ok.np[8];
    CHECK(basecall_cut_chunks(&ok.job, host, ~0ull, chunks, &bad));
  }
  CHECK(offset_fits(~0ull, 0) && !offset_fits(~0ull, 1) && offset_fits(0, ~0ull) && !offset_fits(1, ~0ull));
}

// ---- the run-merger ----
struct Triple { int k; uint64_t src, dst, bytes; };
struct Record {
  std::vector<Triple>* log;
  int operator()(int k, uint64_t s, uint64_t d, uint64_t bytes) const { log->push_back(Triple{k, s, d, bytes}); return 0; }
};
struct FailSecond {  // the second triple is an error
  int* calls;
  int operator()(int, uint64_t, uint64_t, uint64_t) const { return ++*calls == 2 ? 7 : 0; }
};

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// gaps: bit 0 -- between regions on the staged side, bit 1 -- on the caller's
template <int N>
static void check_merger(const uint32_t (&widths)[N], int gaps) {
  const uint32_t n = 300;
  std::vector<uint64_t> rel(n), dst(n);
  std::vector<uint32_t> cap(n), got(n);
  uint64_t r = 0, d = 5;
  for (uint32_t t = 0; t < n; ++t) {
    cap[t] = 1 + rnd() % 40;
    got[t] = t % 11 == 3 ? 0 : t % 7 == 2 ? rnd() % cap[t] : cap[t];
    rel[t] = r; dst[t] = d;
    r += cap[t] + ((gaps & 1) && rnd() % 3 == 0 ? 1 + rnd() % 5 : 0);
    d += cap[t] + ((gaps & 2) && rnd() % 3 == 0 ? 1 + rnd() % 5 : 0);
  }
  std::vector<Triple> log;
  RunMerger<N, Record> m{{}, Record{&log}};
  for (int k = 0; k < N; ++k) m.width[k] = widths[k];
  size_t expect_runs = 0;
  bool open = false;
  uint64_t end_r = 0, end_d = 0;
  for (uint32_t t = 0; t < n; ++t) {
    CHECK(m.add(rel[t], dst[t], got[t]) == 0);
    if (!got[t]) continue;
    if (!open || rel[t] != end_r || dst[t] != end_d) ++expect_runs;
    open = true;
    end_r = rel[t] + got[t]; end_d = dst[t] + got[t];
  }
  CHECK(m.flush() == 0);
  CHECK(m.flush() == 0);  // nothing is left
  int live = 0;
  for (int k = 0; k < N; ++k) live += widths[k] != 0;
  CHECK(log.size() == expect_runs * live);
  if (!gaps) CHECK(expect_runs > 1 && expect_runs < n);  // the short and the silent traces alone end a run
  for (int k = 0; k < N; ++k) {
    // what arrived at each byte of the caller's array: the staged byte it came from + 1, 0 where nothing did
    std::vector<uint64_t> from((d + 8) * (widths[k] ? widths[k] : 1), 0);
    for (const Triple& x : log) {
      if (x.k != k) continue;
      CHECK(widths[k] != 0 && x.bytes > 0 && x.bytes % widths[k] == 0);
      for (uint64_t i = 0; i < x.bytes; ++i) {
        CHECK(x.dst + i < from.size());
        if (x.dst + i >= from.size()) break;
        CHECK(from[x.dst + i] == 0);  // each byte once
        from[x.dst + i] = x.src + i + 1;
      }
    }
    if (!widths[k]) continue;
    std::vector<uint64_t> want(from.size(), 0);
    for (uint32_t t = 0; t < n; ++t)
      for (uint64_t i = 0; i < (uint64_t)got[t] * widths[k]; ++i) want[dst[t] * widths[k] + i] = rel[t] * widths[k] + i + 1;
    CHECK(from == want);  // exactly the reported entries, nothing outside
  }
}

static void check_merger_small() {
  std::vector<Triple> log;
  RunMerger<3, Record> m{{1, 0, 24}, Record{&log}};
  // two traces contiguous on both sides and fully reported: one triple per live array
  CHECK(m.add(10, 110, 7) == 0 && m.add(17, 117, 5) == 0 && m.flush() == 0);
  CHECK(log.size() == 2);
  if (log.size() == 2) {
    CHECK(log[0].k == 0 && log[0].src == 10 && log[0].dst == 110 && log[0].bytes == 12);
    CHECK(log[1].k == 2 && log[1].src == 240 && log[1].dst == 2640 && log[1].bytes == 288);
  }
  // contiguous on one side only: two runs
  log.clear();
  CHECK(m.add(0, 0, 4) == 0 && m.add(4, 5, 4) == 0 && m.add(9, 9, 4) == 0 && m.flush() == 0);
  CHECK(log.size() == 6);
  // an error of the functor comes back from add() / flush()
  int calls = 0;
  RunMerger<2, FailSecond> f{{4, 4}, FailSecond{&calls}};
  CHECK(f.add(0, 0, 3) == 0 && f.add(8, 3, 1) == 7 && calls == 2);
}

int main() {
  for (uint32_t n : {1u, 3u, 4u, 5u, 64u, 257u})
    for (uint32_t sb : {4u, 2u})
      for (int host = 0; host < 2; ++host) {
        check_cut(n, sb, host, ~0ull, 1);
        check_cut(n, sb, host, 1ull << 20, 1);
        check_cut(n, sb, host, 1, host ? n : 1);  // host payloads: every trace alone
      }
  check_cut(257, 4, true, 1ull << 20, 4);
  check_validate();
  for (int gaps = 0; gaps < 4; ++gaps) {
    check_merger<1>({2}, gaps);
    check_merger<5>({4, 1, 0, 1, 0}, gaps);
    check_merger<5>({0, 1, 1, 1, 1}, gaps);
    check_merger<7>({1, 1, 1, 1, 4, 16, 24}, gaps);
    check_merger<7>({1, 0, 0, 1, 0, 16, 24}, gaps);
    check_merger<7>({0, 0, 0, 0, 0, 0, 0}, gaps);
  }
  check_merger_small();
  if (failures) { std::printf("basecall_plan: %d failures\n", failures); return 1; }
  std::printf("basecall_plan: ok\n");
  return 0;
}
