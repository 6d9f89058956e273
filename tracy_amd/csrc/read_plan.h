// read_plan.h -- the HIP-free part of tracyhip_read_traces' host side (read.hip): what is refused before a device is touched, the bound,
// the cut of a batch into chunks of consecutive files whose staged bytes fit a limit, and the per-file descriptors of a chunk.
// tests/cpp/read_plan.cpp runs it under the sanitizers.
#ifndef TRACY_AMD_READ_PLAN_H
#define TRACY_AMD_READ_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tracy_hip.h"
#include "ragged_plan.h"
#include "read_wave.h"

namespace tracyhip {

inline bool read_wants_calls(const tracyhip_read_result* o) { return o->basecallpos || o->basecalls1 || o->basecalls2 || o->qual; }
inline bool read_wants_samples(const tracyhip_read_result* o) { return o->signal != nullptr; }

// null: the job may run; else why not (tracyhip_read_validate)
inline const char* read_validate(const tracyhip_read_job* job, int mem, const tracyhip_read_result* out) {
  if (!job || !out) return "null job / result";
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return "bad mem";
  if (job->sample_bytes != 2 && job->sample_bytes != 4) return "sample_bytes must be 2 or 4";
  if (job->ntraces == 0) return nullptr;
  if (!job->bytes || !job->file_offset || !job->file_len) return "null bytes / file_offset / file_len";
  if (!out->status || !out->format || !out->nsamples || !out->ncalls) return "null per-trace result array (status, format, nsamples, ncalls)";
  if (reinterpret_cast<uintptr_t>(out->basecallpos) % 4) return "basecallpos not aligned to 4 bytes";
  if (read_wants_samples(out)) {
    if (!out->sample_offset || !out->sample_cap) return "result signal without sample_offset / sample_cap";
    if (reinterpret_cast<uintptr_t>(out->signal) % job->sample_bytes) return "signal not aligned to its element size";
  }
  if (read_wants_calls(out) && (!out->call_offset || !out->call_cap)) return "result basecall arrays without call_offset / call_cap";
  return nullptr;
}

struct ReadChunk {
  uint32_t t0 = 0, t1 = 0;
  Span in, osig, ocall;  // of the file images and of the result arrays
  uint64_t tiles = 0;    // of the emit launch
};

inline uint32_t read_file_tiles(uint32_t file_len) { return 1 + 4 * read_channel_tiles(file_len); }
// what a chunk with these spans stages (host payloads), in bytes
inline uint64_t read_chunk_bytes(const ReadChunk& c, uint32_t sb, bool host, bool calls) {
  if (!host) return 0;
  return c.in.size() + c.osig.size() * sb + (calls ? c.ocall.size() * 7 : 0);
}
// false: an offset + length of file *bad_t leaves 64 bits, or the chunk's tiles leave 32 (a lone file never does)
inline bool read_cut_chunks(const tracyhip_read_job* job, const tracyhip_read_result* out, bool host, uint64_t limit, std::vector<ReadChunk>& chunks,
                            uint32_t* bad_t) {
  const bool samples = read_wants_samples(out), calls = read_wants_calls(out);
  return cut_spans(
      job->ntraces, limit, chunks, bad_t,
      [=](uint32_t t) {
        return offset_fits(job->file_offset[t], job->file_len[t]) && (!samples || offset_fits(out->sample_offset[t], 4ull * out->sample_cap[t])) &&
               (!calls || offset_fits(out->call_offset[t], out->call_cap[t]));
      },
      [=](ReadChunk& c, uint32_t t) {
        c.in.add(job->file_offset[t], job->file_len[t]);
        if (samples) c.osig.add(out->sample_offset[t], 4ull * out->sample_cap[t]);
        if (calls) c.ocall.add(out->call_offset[t], out->call_cap[t]);
        c.tiles += read_file_tiles(job->file_len[t]);
      },
      [=](const ReadChunk& c, uint64_t lim) { return read_chunk_bytes(c, job->sample_bytes, host, calls) > lim || c.tiles > 0x7fffffffull; });
}

// the descriptor of file t of chunk c: host payloads are staged from each span's first element, device payloads used in place
inline ReadFile read_file_desc(const tracyhip_read_job* job, const tracyhip_read_result* out, const ReadChunk& c, bool host, uint32_t t, uint32_t tile_first) {
  const bool samples = read_wants_samples(out), calls = read_wants_calls(out);
  ReadFile d{};
  d.file_off = job->file_offset[t] - (host ? c.in.lo : 0);
  d.out_sig_off = samples ? out->sample_offset[t] - (host ? c.osig.lo : 0) : 0;
  d.out_call_off = calls ? out->call_offset[t] - (host ? c.ocall.lo : 0) : 0;
  d.file_len = job->file_len[t];
  d.sample_cap = samples ? out->sample_cap[t] : 0;
  d.call_cap = calls ? out->call_cap[t] : 0;
  d.tile_first = tile_first;
  d.tiles_per_channel = read_channel_tiles(job->file_len[t]);
  return d;
}

}  // namespace tracyhip
#endif
