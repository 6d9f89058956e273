// pad_plan.h -- the HIP-free part of tracyhip_pad_traces' host side (pad.hip): what is refused before a device is touched, the cut of a
// batch into chunks of consecutive traces whose staged bytes and scratch fit a limit, and the per-trace descriptors of a chunk.
// tests/cpp/pad_plan.cpp runs it under the sanitizers.
#ifndef TRACY_AMD_PAD_PLAN_H
#define TRACY_AMD_PAD_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tracy_hip.h"
#include "pad_wave.h"
#include "ragged_plan.h"

namespace tracyhip {

inline bool pad_wants_calls(const tracyhip_pad_result* o) { return o->bcpos || o->primary || o->secondary || o->consensus || o->estqual; }
inline bool pad_wants_samples(const tracyhip_pad_result* o) { return o->signal != nullptr; }

// null: the job may run; else why not (tracyhip_pad_validate)
inline const char* pad_validate(const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out) {
  if (!job || !out) return "null job / result";
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return "bad mem";
  if (job->sample_bytes != 2 && job->sample_bytes != 4) return "sample_bytes must be 2 or 4";
  if ((job->trim_left_each == nullptr) != (job->trim_right_each == nullptr)) return "trim_left_each and trim_right_each go together: both or neither";
  if (job->ntraces == 0) return nullptr;
  if (!job->nsamples || !job->bcpos || !job->bc_offset || !job->bc_len) return "null nsamples / bcpos / bc_offset / bc_len";
  if (!job->rows || !job->row_offset || !job->row_len) return "null rows / row_offset / row_len";
  if (!out->status || !out->nsamples_out || !out->ncalls_out || !out->leading_gaps || !out->trailing_gaps || !out->step)
    return "null per-trace result array (status, nsamples_out, ncalls_out, leading_gaps, trailing_gaps, step)";
  if (reinterpret_cast<uintptr_t>(job->bcpos) % 4 || reinterpret_cast<uintptr_t>(out->bcpos) % 4) return "bcpos not aligned to 4 bytes";
  if (pad_wants_samples(out)) {
    if (!job->signal || !job->signal_offset) return "the padded signal is wanted: null signal / signal_offset";
    if (!out->sample_offset || !out->sample_cap) return "result signal without sample_offset / sample_cap";
    if (reinterpret_cast<uintptr_t>(job->signal) % job->sample_bytes || reinterpret_cast<uintptr_t>(out->signal) % job->sample_bytes)
      return "signal not aligned to its element size";
  }
  if (pad_wants_calls(out)) {
    if (!out->call_offset || !out->call_cap) return "result basecall arrays without call_offset / call_cap";
    if ((out->primary && !job->primary) || (out->secondary && !job->secondary) || (out->consensus && !job->consensus) ||
        (out->estqual && !job->estqual))
      return "a result basecall array is wanted whose input array is null";
  }
  return nullptr;
}

using PadSpan = Span;  // (the name tests/cpp/pad_plan.cpp knows it by)
struct PadChunk {
  uint32_t t0 = 0, t1 = 0;
  Span sig, bc, row, osig, ocall;  // of the input and the result arrays
  uint64_t scratch_words = 0;
};

inline uint32_t pad_trim(const uint32_t* each, uint32_t t) { return each ? each[t] : 0u; }
inline uint64_t pad_scratch_words(const tracyhip_pad_job* job, uint32_t t) {
  const uint32_t n = job->bc_len[t], l = pad_trim(job->trim_left_each, t), r = pad_trim(job->trim_right_each, t);
  if (!pad_sizes_answerable(job->nsamples[t], n, l, r)) return 0;
  return (uint64_t)kPadInsWords * pad_max_inserts(n - l - r, job->row_len[t]);
}
// what a chunk with these spans stages (host payloads) and holds as scratch, in bytes
inline uint64_t pad_chunk_bytes(const PadChunk& c, uint32_t sb, bool host, bool samples, bool calls) {
  uint64_t b = c.scratch_words * 4;
  if (!host) return b;
  b += c.bc.size() * 4 + c.row.size();
  if (calls) b += c.bc.size() * 4 + c.ocall.size() * 8;
  if (samples) b += (c.sig.size() + c.osig.size()) * sb;
  return b;
}
// false: an offset + length of trace *bad_t leaves 64 bits
inline bool pad_cut_chunks(const tracyhip_pad_job* job, const tracyhip_pad_result* out, bool host, uint64_t limit, std::vector<PadChunk>& chunks,
                           uint32_t* bad_t) {
  const bool samples = pad_wants_samples(out), calls = pad_wants_calls(out), payload = samples || calls;
  return cut_spans(
      job->ntraces, limit, chunks, bad_t,
      [=](uint32_t t) {
        return offset_fits(job->bc_offset[t], job->bc_len[t]) && offset_fits(job->row_offset[t], job->row_len[t]) &&
               (!samples || (offset_fits(job->signal_offset[t], 4ull * job->nsamples[t]) && offset_fits(out->sample_offset[t], 4ull * out->sample_cap[t]))) &&
               (!calls || offset_fits(out->call_offset[t], out->call_cap[t]));
      },
      [=](PadChunk& c, uint32_t t) {
        c.bc.add(job->bc_offset[t], job->bc_len[t]);
        c.row.add(job->row_offset[t], job->row_len[t]);
        if (samples) { c.sig.add(job->signal_offset[t], 4ull * job->nsamples[t]); c.osig.add(out->sample_offset[t], 4ull * out->sample_cap[t]); }
        if (calls) c.ocall.add(out->call_offset[t], out->call_cap[t]);
        if (payload) c.scratch_words += pad_scratch_words(job, t);
      },
      [=](const PadChunk& c, uint64_t lim) { return pad_chunk_bytes(c, job->sample_bytes, host, samples, calls) > lim; });
}

// the descriptor of trace t of chunk c: host payloads are staged from each span's first element, device payloads used in place
inline PadTrace pad_trace_desc(const tracyhip_pad_job* job, const tracyhip_pad_result* out, const PadChunk& c, bool host, uint32_t t, uint64_t scratch_off) {
  const bool samples = pad_wants_samples(out), calls = pad_wants_calls(out);
  PadTrace d{};
  d.sig_off = samples ? job->signal_offset[t] - (host ? c.sig.lo : 0) : 0;
  d.bc_off = job->bc_offset[t] - (host ? c.bc.lo : 0);
  d.row_off = job->row_offset[t] - (host ? c.row.lo : 0);
  d.scratch_off = scratch_off;
  d.out_sig_off = samples ? out->sample_offset[t] - (host ? c.osig.lo : 0) : 0;
  d.out_call_off = calls ? out->call_offset[t] - (host ? c.ocall.lo : 0) : 0;
  d.nsamples = job->nsamples[t]; d.bc_len = job->bc_len[t]; d.row_len = job->row_len[t];
  d.trim_l = pad_trim(job->trim_left_each, t); d.trim_r = pad_trim(job->trim_right_each, t);
  d.reverse = job->reverse ? job->reverse[t] != 0 : 0;
  d.sample_cap = samples ? out->sample_cap[t] : 0;
  d.call_cap = calls ? out->call_cap[t] : 0;
  return d;
}

}  // namespace tracyhip
#endif
