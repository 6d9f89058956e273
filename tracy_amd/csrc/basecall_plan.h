// basecall_plan.h -- the HIP-free part of tracyhip_basecall_traces' host side (basecall.hip): what is refused before a device is touched,
// the cut of a batch into chunks of consecutive traces whose staged chromatogram fits a limit, and the per-trace descriptors of a chunk.
// tests/cpp/basecall_plan.cpp runs it under the sanitizers.
#ifndef TRACY_AMD_BASECALL_PLAN_H
#define TRACY_AMD_BASECALL_PLAN_H

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/tracy_hip.h"
#include "basecall_wave.h"
#include "ragged_plan.h"

namespace tracyhip {

// null: the job may run; else why not (tracyhip_basecall_validate)
inline const char* basecall_validate(const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) {
  if (!job || !out) return "null job / result";
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return "bad mem";
  if (job->sample_bytes != 2 && job->sample_bytes != 4) return "sample_bytes must be 2 or 4";
  if (std::isnan(job->sigratio)) return "sigratio is not a number";
  if (std::isnan(job->trim_stringency) || job->trim_stringency < 0) return "trim_stringency must be 0 or positive";
  if (job->ntraces == 0) return nullptr;
  if (!job->signal || !job->signal_offset || !job->nsamples || !job->basecallpos || !job->pos_offset || !job->npos)
    return "null signal / basecallpos or one of their offset and length arrays";
  if (reinterpret_cast<uintptr_t>(job->signal) % job->sample_bytes || reinterpret_cast<uintptr_t>(job->basecallpos) % 4)
    return "signal / basecallpos not aligned to their element size";
  if (!out->status || !out->bc_len || !out->trim_left || !out->trim_right || !out->best_section)
    return "null per-trace result array (status, bc_len, trim_left, trim_right, best_section)";
  return nullptr;
}

struct BasecallChunk {
  uint32_t t0 = 0, t1 = 0;
  Span sig, pos;  // chromatogram elements; positions in and every per-basecall result out
};

// the words of the trace's scratch region: none for a trace whose sizes alone defer it
inline uint64_t basecall_scratch_words(const tracyhip_basecall_job* job, uint32_t t) {
  const uint32_t np = job->npos[t], ns = job->nsamples[t];
  return np >= 1 && np <= kBcMaxPos && ns >= 3 && ns <= kBcMaxSamples ? 3ull * np + 1 : 0;
}

// Host payloads: a chunk closes when the chromatogram span it stages would exceed `limit` bytes (a trace alone goes whatever it takes).
// Device payloads: one chunk.  false: an offset + length of trace *bad_t leaves 64 bits
inline bool basecall_cut_chunks(const tracyhip_basecall_job* job, bool host, uint64_t limit, std::vector<BasecallChunk>& chunks, uint32_t* bad_t) {
  return cut_spans(
      job->ntraces, limit, chunks, bad_t,
      [=](uint32_t t) { return offset_fits(job->signal_offset[t], 4ull * job->nsamples[t]) && offset_fits(job->pos_offset[t], job->npos[t]); },
      [=](BasecallChunk& c, uint32_t t) {
        c.sig.add(job->signal_offset[t], 4ull * job->nsamples[t]);
        c.pos.add(job->pos_offset[t], job->npos[t]);
      },
      [=](const BasecallChunk& c, uint64_t lim) { return host && c.sig.size() * job->sample_bytes > lim; });
}

// the descriptor of trace t of chunk c: host payloads are staged from each span's first element, device payloads used in place
inline BasecallTrace basecall_trace_desc(const tracyhip_basecall_job* job, const BasecallChunk& c, bool host, uint32_t t, uint64_t scratch_off) {
  return BasecallTrace{job->signal_offset[t] - (host ? c.sig.lo : 0), job->pos_offset[t] - (host ? c.pos.lo : 0), scratch_off, job->nsamples[t],
                       job->npos[t]};
}

}  // namespace tracyhip
#endif
