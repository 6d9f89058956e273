// pad.hip -- tracyhip_pad_traces: chromatograms and basecalls re-spaced along their alignment rows on the device (hard trim trim.h:77-99,
// reverseComplementTrace trim.h:125-150, alignmentTracePadding json.h:383-472), equal in every field to the host chain of tracy_amd/host
// for every trace it answers; the rest is DEFERRED to the host.
//
// One wave per trace, four traces per workgroup; the per-trace body and its closed forms are pad_wave.h's (compiled for the host wave by
// tests/emu/emu_pad.cpp), the wave dev_wave.h's SoloWave.  Each wave owns 3 KB of the workgroup's LDS, the moving tile of its insert
// list.  What is refused before a device is touched, the cut into chunks and the descriptors are pad_plan.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "dev_wave.h"
#include "pad_plan.h"
#include "pad_wave.h"

using namespace tracyhip;

static_assert(TRACYHIP_PAD_OK == kPadStatusOk && TRACYHIP_PAD_DEFERRED == kPadStatusDeferred && TRACYHIP_PAD_TOO_SMALL == kPadStatusTooSmall, "status codes");

namespace {

constexpr uint32_t kPadWaves = 4;  // traces per workgroup

template <bool S16>
__global__ __launch_bounds__(64 * kPadWaves) void pad_kernel(PadArgs a) {
  const uint32_t t = blockIdx.x * kPadWaves + (threadIdx.x >> 6);
  if (t >= a.ntraces) return;  // (the whole wave)
  SoloWave<kPadWaves, kPadLdsBytes> w;
  pad_wave_body<S16>(w, a, t);
}

int validate(const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out) {
  const char* why = pad_validate(job, mem, out);
  return why ? set_error(TRACYHIP_ERR_ARG, "tracyhip_pad_traces: %s", why) : TRACYHIP_OK;
}

}  // namespace

extern "C" {

int tracyhip_pad_validate(const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out) { return validate(job, mem, out); }

int tracyhip_last_pad_stats(tracyhip_ctx* ctx, tracyhip_pad_stats* out) {
  if (!ctx || !out) return set_error(TRACYHIP_ERR_ARG, "null context / out");
  *out = ctx->pad_stats;
  return TRACYHIP_OK;
}

int tracyhip_pad_traces(tracyhip_ctx* ctx, const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out) {
  int rc = validate(job, mem, out);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const uint32_t n = job->ntraces;
  if (n == 0) return TRACYHIP_OK;
  rc = ctx_begin(ctx);
  if (rc != TRACYHIP_OK) return rc;
  ctx->stats = tracyhip_call_stats{};
  ctx->stats.traces = n;
  ctx->pad_stats = tracyhip_pad_stats{};
  const bool host = mem == TRACYHIP_MEM_HOST;
  const uint32_t sb = job->sample_bytes;
  const bool samples = pad_wants_samples(out), calls = pad_wants_calls(out);
  std::vector<PadChunk> chunks;
  uint32_t bad_t = 0;
  if (!pad_cut_chunks(job, out, host, ctx->ws_limit ? ctx->ws_limit : 256ull << 20, chunks, &bad_t))
    return set_error(TRACYHIP_ERR_RANGE, "tracyhip_pad_traces: an offset + length of trace %u leaves 64 bits", bad_t);
  ctx->pad_stats.pad_chunks = (uint32_t)chunks.size();

  // descriptors up and results back for the whole batch in one buffer; a chunk launches over its slice
  const size_t b_out = (sizeof(PadTrace) * n + 15) & ~size_t(15);
  uint8_t* d0; HIP_TRY(ensure_into(ctx->dev[PD_TRACES], b_out + sizeof(PadOut) * n, d0));
  std::vector<PadTrace> meta(n);
  std::vector<PadOut> res(n);
  uint32_t* d_scratch = nullptr;  // sized once for the largest chunk: the launches of a device call follow each other without a wait
  if (samples || calls) {
    uint64_t words = 1;
    for (const PadChunk& c : chunks) words = std::max(words, c.scratch_words);
    HIP_TRY(ensure_into(ctx->dev[PD_SCRATCH], words, d_scratch));
  }
  auto report = [&](uint32_t t) {
    const PadOut& o = res[t];
    out->status[t] = o.status;
    out->nsamples_out[t] = o.nsamples_out; out->ncalls_out[t] = o.ncalls_out;
    if (o.status == TRACYHIP_PAD_DEFERRED) { ctx->pad_stats.pad_deferred += 1; return; }  // status and zero sizes, nothing else
    if (o.status == TRACYHIP_PAD_TOO_SMALL) ctx->pad_stats.pad_too_small += 1;
    out->leading_gaps[t] = o.leading; out->trailing_gaps[t] = o.trailing; out->step[t] = o.step;
  };
  for (const PadChunk& c : chunks) {
    const uint32_t m = c.t1 - c.t0;
    uint64_t scratch_words = 0;
    for (uint32_t t = c.t0; t < c.t1; ++t) {
      meta[t] = pad_trace_desc(job, out, c, host, t, scratch_words);
      if (samples || calls) scratch_words += pad_scratch_words(job, t);
    }
    HIP_TRY(hipMemcpyAsync(d0 + sizeof(PadTrace) * c.t0, meta.data() + c.t0, sizeof(PadTrace) * m, hipMemcpyHostToDevice, ctx->stream));
    PadArgs a{};
    a.tr = reinterpret_cast<const PadTrace*>(d0) + c.t0;
    a.out = reinterpret_cast<PadOut*>(d0 + b_out) + c.t0;
    a.ntraces = m;
    a.scratch = d_scratch;
    Layout lo;  // the staged results of a host chunk
    uint64_t o_sig = 0, o_pos = 0, o_byte[4] = {0, 0, 0, 0};
    uint8_t* const want_byte[4] = {out->primary, out->secondary, out->consensus, out->estqual};
    if (host) {
      // inputs: the elements of each span, first element at the part's start
      Layout li;
      const uint64_t i_pos = li.add(c.bc.size() * 4), i_row = li.add(c.row.size());
      const uint8_t* const in_byte[4] = {job->primary, job->secondary, job->consensus, job->estqual};
      uint64_t i_byte[4];
      for (int k = 0; k < 4; ++k) i_byte[k] = li.add(want_byte[k] ? c.bc.size() : 0);
      const uint64_t i_sig = li.add(samples ? c.sig.size() * sb : 0);
      uint8_t* din; HIP_TRY(ensure_into(ctx->dev[PD_IN], li.total(), din));
      auto up = [&](uint64_t at, const void* src, uint64_t bytes) {
        return bytes ? hipMemcpyAsync(din + at, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
      };
      HIP_TRY(up(i_pos, job->bcpos + c.bc.lo, c.bc.size() * 4));
      HIP_TRY(up(i_row, job->rows + c.row.lo, c.row.size()));
      for (int k = 0; k < 4; ++k)
        if (want_byte[k]) HIP_TRY(up(i_byte[k], in_byte[k] + c.bc.lo, c.bc.size()));
      if (samples) HIP_TRY(up(i_sig, static_cast<const uint8_t*>(job->signal) + c.sig.lo * sb, c.sig.size() * sb));
      a.bcpos = reinterpret_cast<const int32_t*>(din + i_pos);
      a.rows = din + i_row;
      if (want_byte[0]) a.primary = din + i_byte[0];
      if (want_byte[1]) a.secondary = din + i_byte[1];
      if (want_byte[2]) a.consensus = din + i_byte[2];
      if (want_byte[3]) a.estqual = din + i_byte[3];
      if (samples) a.signal = din + i_sig;
      o_sig = lo.add(samples ? c.osig.size() * sb : 0);
      o_pos = lo.add(out->bcpos ? c.ocall.size() * 4 : 0);
      for (int k = 0; k < 4; ++k) o_byte[k] = lo.add(want_byte[k] ? c.ocall.size() : 0);
      uint8_t* dout; HIP_TRY(ensure_into(ctx->dev[PD_OUT], lo.total(), dout));
      if (samples) a.o_signal = dout + o_sig;
      if (out->bcpos) a.o_bcpos = reinterpret_cast<int32_t*>(dout + o_pos);
      if (want_byte[0]) a.o_primary = dout + o_byte[0];
      if (want_byte[1]) a.o_secondary = dout + o_byte[1];
      if (want_byte[2]) a.o_consensus = dout + o_byte[2];
      if (want_byte[3]) a.o_estqual = dout + o_byte[3];
    } else {
      a.signal = job->signal; a.bcpos = job->bcpos; a.rows = job->rows;
      a.primary = job->primary; a.secondary = job->secondary; a.consensus = job->consensus; a.estqual = job->estqual;
      a.o_signal = out->signal; a.o_bcpos = out->bcpos;
      a.o_primary = out->primary; a.o_secondary = out->secondary; a.o_consensus = out->consensus; a.o_estqual = out->estqual;
    }
    if (ctx->timing) {
      uint64_t moved = 0;
      if (samples)
        for (uint32_t t = c.t0; t < c.t1; ++t) moved += 8ull * sb * job->nsamples[t];  // (read once, written at least once)
      if ((rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, moved))) return rc;
    }
    const dim3 grid((m + kPadWaves - 1) / kPadWaves), block(64 * kPadWaves);
    if (sb == 2) hipLaunchKernelGGL(pad_kernel<true>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(pad_kernel<false>, grid, block, 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    if ((rc = timing_end(ctx))) return rc;
    if (!host) continue;  // device payloads: the results of all chunks come back behind the last launch
    HIP_TRY(hipMemcpyAsync(res.data() + c.t0, a.out, sizeof(PadOut) * m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx_sync(ctx));
    timing_collect(ctx);
    // exactly what was reported goes back, straight into the caller's arrays; regions that follow each other on both sides travel as one copy
    const uint8_t* dout = static_cast<const uint8_t*>(ctx->dev[PD_OUT].p);
    RunMerger<1, CopyBackRun<1>> rs{{samples ? sb : 0}, {ctx, {dout + o_sig}, {static_cast<uint8_t*>(out->signal)}}};
    RunMerger<5, CopyBackRun<5>> rcall{{out->bcpos ? 4u : 0u}, {ctx, {dout + o_pos}, {reinterpret_cast<uint8_t*>(out->bcpos)}}};
    for (int k = 0; k < 4; ++k) {
      rcall.width[1 + k] = want_byte[k] ? 1 : 0;
      rcall.emit.src[1 + k] = dout + o_byte[k]; rcall.emit.dst[1 + k] = want_byte[k];
    }
    for (uint32_t t = c.t0; t < c.t1; ++t) {
      report(t);
      if (res[t].status != TRACYHIP_PAD_OK) continue;
      if (samples) HIP_TRY(rs.add(meta[t].out_sig_off, out->sample_offset[t], 4ull * res[t].nsamples_out));
      if (calls) HIP_TRY(rcall.add(meta[t].out_call_off, out->call_offset[t], res[t].ncalls_out));
    }
    if (samples || calls) {
      HIP_TRY(rs.flush());
      HIP_TRY(rcall.flush());
      HIP_TRY(ctx_sync(ctx));
    }
  }
  if (!host) {
    HIP_TRY(hipMemcpyAsync(res.data(), d0 + b_out, sizeof(PadOut) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx_sync(ctx));  // the one synchronisation of a device call: the sizes are what the caller allocates by
    timing_collect(ctx);
    for (uint32_t t = 0; t < n; ++t) report(t);
  }
  return TRACYHIP_OK;
}

int tracyhip_pad_traces_async(tracyhip_ctx* ctx, const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out) {
  if (!ctx || !job || !out) return set_error(TRACYHIP_ERR_ARG, "null context / job / result");
  const tracyhip_pad_job j = *job;
  const tracyhip_pad_result o = *out;
  return async_submit(ctx, [=]() { return tracyhip_pad_traces(ctx, &j, mem, &o); });
}

}  // extern "C"
