// two_pass.h -- the host frame of the batch calls that run twice over ragged items, once for the sizes and once for the payloads
// (tracyhip_read_traces, tracyhip_pad_traces, tracyhip_render_traces, tracyhip_render_alignments): what every one of them does around
// its own launches.  The call's file keeps its kernels, its scratch, the layout of what it stages, the launches, what it reports per
// item and what it copies back; the cut is its *_plan.h's over ragged_plan.h's cut_spans.
//
// A call goes: begin() -- nothing to do for no item, else the context, the counters, the cut into chunks under the workspace limit
// (tracyhip_set_workspace_limit; 256 MB without one) and one buffer for the whole batch, descriptors up in front and results back behind
// them; the call sizes its scratch for the largest chunk; run() -- per chunk the descriptors of its items go up, the call stages and
// launches over the chunk's slice of that buffer, and
//   host payloads: the chunk's results come back and the stream is waited for, every item is reported, what the call copies back is
//                  queued and waited for: two waits per chunk, one in the sizes-only form;
//   device payloads: nothing waits between the launches; the results of all chunks come back behind the last one, in one copy and the
//                  one wait of the call -- the sizes are what the caller allocates or builds its next job by.
// tracyhip_basecall_traces is not one of them: its descriptor buffer is per chunk, it waits per chunk with device payloads too, and it
// has neither a sizes-only form nor counters; folding it in would change its stream order.
#ifndef TRACY_AMD_TWO_PASS_H
#define TRACY_AMD_TWO_PASS_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"

namespace tracyhip {

// Desc: what a launch reads per item; Out: what it writes per item; Chunk: the call's chunk of ragged_plan.h's cut_spans
template <class Desc, class Out, class Chunk>
struct TwoPass {
  tracyhip_ctx* ctx;
  uint32_t n;  // items of the batch
  bool host;   // host payloads
  std::vector<Chunk> chunks;  // empty behind begin(): there is nothing to do
  std::vector<Desc> meta;     // filled by the call's launch, chunk by chunk
  std::vector<Out> res;       // what report and copy-back read
  uint8_t* d0 = nullptr;      // [Desc x n | Out x n], the second part aligned to 16
  size_t b_out = 0;

  // who: the call's name, noun: what it calls an item ("trace", "alignment"), for the error text; slot: the DevBuf of the batch's
  // buffer; stats: the call's own counters in the context, nchunks: the one of them that takes the number of chunks;
  // cut(limit, chunks, &bad_t): the call's *_cut_chunks
  template <class Stats, class Cut>
  int begin(const char* who, const char* noun, int slot, Stats tracyhip_ctx::*stats, uint32_t Stats::*nchunks, Cut cut) {
    if (n == 0) return TRACYHIP_OK;
    const int rc = ctx_begin(ctx);
    if (rc != TRACYHIP_OK) return rc;
    ctx->stats = tracyhip_call_stats{};
    ctx->stats.traces = n;
    ctx->*stats = Stats{};
    uint32_t bad_t = 0;
    if (!cut(ctx->ws_limit ? ctx->ws_limit : 256ull << 20, chunks, &bad_t)) {
      chunks.clear();
      return set_error(TRACYHIP_ERR_RANGE, "%s: an offset + length of %s %u leaves 64 bits", who, noun, bad_t);
    }
    (ctx->*stats).*nchunks = (uint32_t)chunks.size();
    b_out = (sizeof(Desc) * n + 15) & ~size_t(15);
    HIP_TRY(ensure_into(ctx->dev[slot], b_out + sizeof(Out) * n, d0));
    meta.resize(n);
    res.resize(n);
    return TRACYHIP_OK;
  }

  // the chunk's slices of the batch's buffer
  const Desc* desc_ptr(const Chunk& c) const { return reinterpret_cast<const Desc*>(d0) + c.t0; }
  Out* out_ptr(const Chunk& c) const { return reinterpret_cast<Out*>(d0 + b_out) + c.t0; }
  hipError_t upload(const Chunk& c) {
    return hipMemcpyAsync(d0 + sizeof(Desc) * c.t0, meta.data() + c.t0, sizeof(Desc) * (c.t1 - c.t0), hipMemcpyHostToDevice, ctx->stream);
  }
  hipError_t fetch_chunk(const Chunk& c) {
    return hipMemcpyAsync(res.data() + c.t0, out_ptr(c), sizeof(Out) * (c.t1 - c.t0), hipMemcpyDeviceToHost, ctx->stream);
  }
  hipError_t fetch_all() { return hipMemcpyAsync(res.data(), d0 + b_out, sizeof(Out) * n, hipMemcpyDeviceToHost, ctx->stream); }

  // launch(c): fills meta[c.t0 .. c.t1) and sends them with upload(c), stages the payloads of a host chunk, builds the kernel
  // arguments over desc_ptr(c) / out_ptr(c), timing_begin, the launches, timing_end; report(t): res[t] into the caller's per-item
  // arrays and the counters; back(c): for a host chunk of a call with payloads, queues the copies of what the items with status OK
  // reported (RunMerger add + flush).  launch and back return a status.  payloads: the call writes payload arrays, not the sizes alone;
  // a host chunk of such a call gets its second wait whether or not an item had something to copy, so that host_syncs stays twice the
  // chunks -- which is why `back` does not say what it queued
  template <class Launch, class Report, class Back>
  int run(bool payloads, Launch launch, Report report, Back back) {
    int rc;
    for (const Chunk& c : chunks) {
      if ((rc = launch(c)) != TRACYHIP_OK) return rc;
      if (!host) continue;  // device payloads: the results of all chunks come back behind the last launch
      HIP_TRY(fetch_chunk(c));
      HIP_TRY(ctx_sync(ctx));
      timing_collect(ctx);
      for (uint32_t t = c.t0; t < c.t1; ++t) report(t);
      if (!payloads) continue;
      // exactly what was reported goes back, straight into the caller's arrays; regions that follow each other on both sides travel as one copy
      if ((rc = back(c)) != TRACYHIP_OK) return rc;
      HIP_TRY(ctx_sync(ctx));
    }
    if (!host) {
      HIP_TRY(fetch_all());
      HIP_TRY(ctx_sync(ctx));  // the one synchronisation of a device call
      timing_collect(ctx);
      for (uint32_t t = 0; t < n; ++t) report(t);
    }
    return TRACYHIP_OK;
  }
};

}  // namespace tracyhip
#endif
