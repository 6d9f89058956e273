// render_plan.h -- the HIP-free part of tracyhip_render_traces' host side (render.hip): what is refused before a device is touched, the
// upper bound of a trace's text, the cut of a batch into chunks of consecutive traces whose staged bytes and tile scratch fit a limit,
// and the per-trace descriptors of a chunk.  tests/cpp/render_plan.cpp runs it under the sanitizers.
#ifndef TRACY_AMD_RENDER_PLAN_H
#define TRACY_AMD_RENDER_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tracy_hip.h"
#include "ragged_plan.h"
#include "render_wave.h"

namespace tracyhip {

// null: the job may run; else why not (tracyhip_render_validate)
inline const char* render_validate(const tracyhip_render_job* job, int mem, const tracyhip_render_result* out) {
  if (!job || !out) return "null job / result";
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return "bad mem";
  if (job->form != TRACYHIP_RENDER_TSV && job->form != TRACYHIP_RENDER_JSON && job->form != TRACYHIP_RENDER_GAPPED) return "bad form";
  if (job->sample_bytes != 2 && job->sample_bytes != 4) return "sample_bytes must be 2 or 4";
  if ((job->trim_left_each == nullptr) != (job->trim_right_each == nullptr)) return "trim_left_each and trim_right_each go together: both or neither";
  if (job->ntraces == 0) return nullptr;
  if (!job->signal || !job->signal_offset || !job->nsamples) return "null signal / signal_offset / nsamples";
  if (!job->bcpos || !job->primary || !job->secondary || !job->estqual || !job->bc_offset || !job->bc_len)
    return "null bcpos / primary / secondary / estqual / bc_offset / bc_len";
  if (job->form == TRACYHIP_RENDER_TSV && !job->consensus) return "the TSV prints the consensus: null consensus";
  if (!out->status || !out->text_len) return "null per-trace result array (status, text_len)";
  if (reinterpret_cast<uintptr_t>(job->bcpos) % 4) return "bcpos not aligned to 4 bytes";
  if (reinterpret_cast<uintptr_t>(job->signal) % job->sample_bytes) return "signal not aligned to its element size";
  if (out->text && (!out->text_offset || !out->text_cap)) return "result text without text_offset / text_cap";
  return nullptr;
}

// an upper bound of text_len of a trace of these sizes, whatever its values (tracyhip_render_bound); 0 for a form that does not exist.
// Beyond the answered domain it is still a number, and means nothing.
inline uint64_t render_bound(uint32_t form, uint32_t nsamples, uint32_t bc_len, uint32_t sample_bytes) {
  const uint64_t ns = nsamples, n = bc_len;
  const uint64_t val = sample_bytes == 2 ? 6 : 11;  // "-32768" / "-2147483648"
  const uint64_t dpos = render_digits(nsamples), dcall = render_digits(bc_len);
  const uint64_t peaks = 4 * (16 + ns * (val + 2));                // "\"peakA\": [" + "],\n" are 13
  const uint64_t callpos = 32 + n * (dpos + 2), callq = 32 + n * 5;  // "\"basecallQual\": [" + "],\n" are 20; a quality has three digits
  switch (form) {
    case kRenderTsv:  // the header; per sample its number, four values, six tabs and "NA" columns; per call what its columns add to them
      return 65 + ns * (dpos + 4 * val + 5 + 18) + n * (dcall + 4);
    case kRenderJson:  // a basecalls item: , "pos":"call:P|A|G"
      return 16 + ns * (dpos + 2) + peaks + callpos + callq + 32 + n * (dpos + dcall + 14) + 2 * (32 + n);
    case kRenderGapped:  // , "pos":"gapless:P|S"
      return peaks + callpos + callq + 32 + n * (dpos + dcall + 12);
    default: return 0;
  }
}

struct RenderChunk {
  uint32_t t0 = 0, t1 = 0;
  Span sig, bc, text;  // of the input arrays (elements) and of the result text (bytes)
  uint64_t tiles = 0;
};
constexpr uint64_t kRenderMaxChunkTiles = 1ull << 30;  // tile numbers are 32-bit on the device

inline uint32_t render_trim(const uint32_t* each, uint32_t t) { return each ? each[t] : 0u; }
inline uint32_t render_trace_tiles(const tracyhip_render_job* job, uint32_t t) {
  return render_answerable(job->nsamples[t], job->bc_len[t]) ? render_tiles(job->form, job->nsamples[t], job->bc_len[t]) : 0u;
}
// what a chunk stages (host payloads) and holds as scratch, in bytes
inline uint64_t render_chunk_bytes(const RenderChunk& c, uint32_t sb, bool host, bool consensus, bool payload) {
  uint64_t b = c.tiles * 8;
  if (!host) return b;
  b += c.sig.size() * sb + c.bc.size() * (4 + 3 + (consensus ? 1 : 0));
  if (payload) b += c.text.size();
  return b;
}
// false: an offset + length of trace *bad_t leaves 64 bits
inline bool render_cut_chunks(const tracyhip_render_job* job, const tracyhip_render_result* out, bool host, uint64_t limit,
                              std::vector<RenderChunk>& chunks, uint32_t* bad_t) {
  const bool payload = out->text != nullptr, consensus = job->form == TRACYHIP_RENDER_TSV;
  return cut_spans(
      job->ntraces, limit, chunks, bad_t,
      [=](uint32_t t) {
        return offset_fits(job->signal_offset[t], 4ull * job->nsamples[t]) && offset_fits(job->bc_offset[t], job->bc_len[t]) &&
               (!payload || offset_fits(out->text_offset[t], out->text_cap[t]));
      },
      [=](RenderChunk& c, uint32_t t) {
        c.sig.add(job->signal_offset[t], 4ull * job->nsamples[t]);
        c.bc.add(job->bc_offset[t], job->bc_len[t]);
        if (payload) c.text.add(out->text_offset[t], out->text_cap[t]);
        c.tiles += render_trace_tiles(job, t);
      },
      [=](const RenderChunk& c, uint64_t lim) {
        return render_chunk_bytes(c, job->sample_bytes, host, consensus, payload) > lim || c.tiles > kRenderMaxChunkTiles;
      });
}

// the descriptor of trace t of chunk c: host payloads are staged from each span's first element, device payloads used in place
inline RenderTrace render_trace_desc(const tracyhip_render_job* job, const tracyhip_render_result* out, const RenderChunk& c, bool host, uint32_t t,
                                     uint32_t tile_first) {
  RenderTrace d{};
  d.sig_off = job->signal_offset[t] - (host ? c.sig.lo : 0);
  d.bc_off = job->bc_offset[t] - (host ? c.bc.lo : 0);
  d.text_off = out->text ? out->text_offset[t] - (host ? c.text.lo : 0) : 0;
  d.text_cap = out->text ? out->text_cap[t] : 0;
  d.nsamples = job->nsamples[t]; d.bc_len = job->bc_len[t];
  d.trim_l = render_trim(job->trim_left_each, t); d.trim_r = render_trim(job->trim_right_each, t);
  d.tile_first = tile_first;
  d.answerable = render_answerable(d.nsamples, d.bc_len) ? 1u : 0u;
  return d;
}

}  // namespace tracyhip
#endif
