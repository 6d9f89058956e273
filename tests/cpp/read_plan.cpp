// read_plan.cpp -- a stand-alone run of tracy_amd/csrc/read_plan.h (no HIP, its own main; tests/test_emu_read.py builds it plain and with the
// sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o read_plan tests/cpp/read_plan.cpp
// It cuts batches of 1 .. 257 file images of mixed lengths under several limits -- one smaller than any file, one of exactly one file --
// for host and device payloads and for the sizes-only form, and checks: the chunks are consecutive and cover every file once, a chunk
// of more than one file fits the limit, the spans hold every region of the chunk's files, the descriptors point inside the spans (host)
// or at the caller's offsets (device), the tiles of a chunk follow each other and suffice for any file of that length; an offset that
// leaves 64 bits is refused; read_validate's verdicts; the bound.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tracy_amd/csrc/read_plan.h"

using namespace tracyhip;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

constexpr uint32_t kFileLen = 5000;  // of every file of a uniform batch

struct Batch {
  std::vector<uint64_t> file_off, osig_off, ocall_off;
  std::vector<uint32_t> file_len, scap, ccap;
  tracyhip_read_job job{};
  tracyhip_read_result out{};
  std::vector<int32_t> status, format;
  std::vector<uint32_t> ns, nc;
  explicit Batch(uint32_t n, bool payload, bool uniform = false) {
    uint64_t fo = 3, oso = 4, oco = 2;
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t len = uniform ? kFileLen : t % 11 == 5 ? 0 : 40 + (t * 7919u) % 100000u;
      file_off.push_back(fo); file_len.push_back(len);
      fo += len + t % 3;  // (any alignment, gaps between the images)
      scap.push_back(read_bound_samples(len)); ccap.push_back(read_bound_calls(len));
      osig_off.push_back(oso); ocall_off.push_back(oco);
      oso += 4ull * scap.back() + t % 2; oco += ccap.back();
    }
    static uint8_t dummy8[4];
    static int32_t dummy32[4];
    job.ntraces = n; job.bytes = dummy8; job.file_offset = file_off.data(); job.file_len = file_len.data(); job.sample_bytes = 2;
    status.assign(n, 0); format.assign(n, 0); ns.assign(n, 0); nc.assign(n, 0);
    out.status = status.data(); out.format = format.data(); out.nsamples = ns.data(); out.ncalls = nc.data();
    if (payload) {
      out.signal = dummy32; out.sample_offset = osig_off.data(); out.sample_cap = scap.data();
      out.basecallpos = dummy32; out.basecalls1 = out.basecalls2 = out.qual = dummy8;
      out.call_offset = ocall_off.data(); out.call_cap = ccap.data();
    }
  }
};

static bool inside(const Span& s, uint64_t off, uint64_t len) { return len == 0 || (off >= s.lo && off + len <= s.hi); }

static size_t check_cut(Batch& b, bool payload, bool host, uint64_t limit, size_t min_chunks) {
  const uint32_t n = b.job.ntraces;
  CHECK(read_validate(&b.job, host ? TRACYHIP_MEM_HOST : TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
  std::vector<ReadChunk> chunks;
  uint32_t bad = ~0u;
  CHECK(read_cut_chunks(&b.job, &b.out, host, limit, chunks, &bad));
  CHECK(chunks.size() >= min_chunks);
  uint32_t at = 0;
  for (const ReadChunk& c : chunks) {
    CHECK(c.t0 == at && c.t1 > c.t0 && c.t1 <= n);
    at = c.t1;
    if (c.t1 - c.t0 > 1) CHECK(read_chunk_bytes(c, b.job.sample_bytes, host, payload) <= limit);
    uint32_t tile = 0;
    for (uint32_t t = c.t0; t < c.t1; ++t) {
      const ReadFile d = read_file_desc(&b.job, &b.out, c, host, t, tile);
      CHECK(d.tile_first == tile && d.file_len == b.file_len[t]);
      tile += read_file_tiles(b.file_len[t]);
      // the groups of a channel are counted from the 8-element boundary below its first output element: one more than the samples fill
      CHECK((uint64_t)d.tiles_per_channel * 64 >= read_bound_samples(b.file_len[t]) / kReadGroup + 2);
      CHECK(inside(c.in, b.file_off[t], b.file_len[t]));
      CHECK(d.file_off + (host ? c.in.lo : 0) == b.file_off[t]);
      if (payload) {
        CHECK(inside(c.osig, b.osig_off[t], 4ull * b.scap[t]) && inside(c.ocall, b.ocall_off[t], b.ccap[t]));
        CHECK(d.out_sig_off + (host ? c.osig.lo : 0) == b.osig_off[t] && d.out_call_off + (host ? c.ocall.lo : 0) == b.ocall_off[t]);
        CHECK(d.sample_cap == b.scap[t] && d.call_cap == b.ccap[t]);
      } else {
        CHECK(d.out_sig_off == 0 && d.out_call_off == 0 && d.sample_cap == 0 && d.call_cap == 0);
      }
    }
    CHECK(tile == c.tiles);
  }
  CHECK(at == n);
  return chunks.size();
}

static void check_validate() {
  Batch b(5, true);
  CHECK(read_validate(&b.job, TRACYHIP_MEM_HOST, &b.out) == nullptr && read_validate(&b.job, TRACYHIP_MEM_DEVICE, &b.out) == nullptr);
  CHECK(read_validate(nullptr, 0, &b.out) && read_validate(&b.job, 0, nullptr) && read_validate(&b.job, 2, &b.out));
  { Batch c(5, true); c.job.sample_bytes = 3; CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.job.bytes = nullptr; CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.job.file_len = nullptr; CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.out.format = nullptr; CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.out.sample_cap = nullptr; CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.out.call_offset = nullptr; CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.out.basecallpos = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(c.out.basecallpos) + 2); CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.out.signal = static_cast<char*>(c.out.signal) + 1; CHECK(read_validate(&c.job, 0, &c.out)); }
  { Batch c(5, true); c.job.bytes += 1; CHECK(read_validate(&c.job, 0, &c.out) == nullptr); }  // the images lie at any address
  { Batch c(5, false); CHECK(read_validate(&c.job, 0, &c.out) == nullptr); }                    // sizes only
  { Batch c(5, true); c.job.ntraces = 0; c.job.bytes = nullptr; CHECK(read_validate(&c.job, 0, &c.out) == nullptr); }  // an empty batch
  // an offset + length that leaves 64 bits: refused with the file's index, whatever the payloads
  for (int which = 0; which < 3; ++which) {
    Batch w(9, true);
    (which == 0 ? w.file_off : which == 1 ? w.osig_off : w.ocall_off)[6] = ~0ull - 8;
    std::vector<ReadChunk> chunks;
    uint32_t bad = ~0u;
    CHECK(!read_cut_chunks(&w.job, &w.out, which != 0, 1ull << 30, chunks, &bad) && bad == 6);
  }
  CHECK(read_bound_samples(0) == 0 && read_bound_calls(7) == 3 && read_bound_samples(100001) == 12500 && read_bound_calls(100001) == 50000);
  CHECK(read_bound_samples(~0u) == kReadMaxSamples && read_bound_calls(~0u) == kReadMaxCalls);
}

int main() {
  for (uint32_t n : {1u, 3u, 4u, 5u, 64u, 257u})
    for (int payload = 0; payload < 2; ++payload)
      for (int host = 0; host < 2; ++host) {
        Batch b(n, payload);
        check_cut(b, payload, host, ~0ull, 1);
        check_cut(b, payload, host, 1ull << 20, 1);
        check_cut(b, payload, host, 1, host ? n : 1);  // a limit smaller than one file: host payloads go every file alone
      }
  {
    // files of one length without gaps, sizes only: what a chunk stages is its images alone, so a limit of exactly one file cuts every
    // file alone, one byte more too, and exactly two files pairs them
    Batch u(9, false, true);
    for (uint32_t t = 0; t < 9; ++t) u.file_off[t] = 16 + (uint64_t)t * kFileLen;
    CHECK(check_cut(u, false, true, kFileLen, 9) == 9);
    CHECK(check_cut(u, false, true, kFileLen + 1, 9) == 9);
    CHECK(check_cut(u, false, true, 2 * kFileLen, 5) == 5);
    CHECK(check_cut(u, false, true, 2 * kFileLen - 1, 9) == 9);
  }
  {
    Batch b(257, true);
    CHECK(check_cut(b, true, true, 1ull << 20, 4) >= 4);
  }
  check_validate();
  if (failures) { std::printf("read_plan: %d failures\n", failures); return 1; }
  std::printf("read_plan: ok\n");
  return 0;
}
