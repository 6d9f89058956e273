// pad.hip -- tracyhip_pad_traces: chromatograms and basecalls re-spaced along their alignment rows on the device (hard trim trim.h:77-99,
// reverseComplementTrace trim.h:125-150, alignmentTracePadding json.h:383-472), equal in every field to the host chain of tracy_amd/host
// for every trace it answers; the rest is DEFERRED to the host.
//
// One wave per trace, four traces per workgroup; the per-trace body and its closed forms are pad_wave.h's (compiled for the host wave by
// tests/emu/emu_pad.cpp), the wave dev_wave.h's SoloWave.  Each wave owns 3 KB of the workgroup's LDS, the moving tile of its insert
// list.  What is refused before a device is touched, the cut into chunks and the descriptors are pad_plan.h's; the frame of the call --
// chunk loop, descriptor and result buffer, waits -- is two_pass.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "dev_wave.h"
#include "pad_plan.h"
#include "pad_wave.h"
#include "two_pass.h"

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

int tracyhip_last_pad_stats(tracyhip_ctx* ctx, tracyhip_pad_stats* out) { return last_stats(ctx, &tracyhip_ctx::pad_stats, out); }

int tracyhip_pad_traces(tracyhip_ctx* ctx, const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out) {
  int rc = validate(job, mem, out);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const bool host = mem == TRACYHIP_MEM_HOST;
  TwoPass<PadTrace, PadOut, PadChunk> f{ctx, job->ntraces, host};
  rc = f.begin("tracyhip_pad_traces", "trace", PD_TRACES, &tracyhip_ctx::pad_stats, &tracyhip_pad_stats::pad_chunks,
               [&](uint64_t limit, std::vector<PadChunk>& chunks, uint32_t* bad_t) { return pad_cut_chunks(job, out, host, limit, chunks, bad_t); });
  if (rc != TRACYHIP_OK || f.chunks.empty()) return rc;
  const uint32_t sb = job->sample_bytes;
  const bool samples = pad_wants_samples(out), calls = pad_wants_calls(out);
  uint32_t* d_scratch = nullptr;  // sized once for the largest chunk: the launches of a device call follow each other without a wait
  if (samples || calls) {
    uint64_t words = 1;
    for (const PadChunk& c : f.chunks) words = std::max(words, c.scratch_words);
    HIP_TRY(ensure_into(ctx->dev[PD_SCRATCH], words, d_scratch));
  }
  uint8_t* const want_byte[4] = {out->primary, out->secondary, out->consensus, out->estqual};
  uint64_t o_sig = 0, o_pos = 0, o_byte[4] = {0, 0, 0, 0};  // the staged results of a host chunk
  return f.run(
      samples || calls,
      [&](const PadChunk& c) {
        const uint32_t m = c.t1 - c.t0;
        uint64_t scratch_words = 0;
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          f.meta[t] = pad_trace_desc(job, out, c, host, t, scratch_words);
          if (samples || calls) scratch_words += pad_scratch_words(job, t);
        }
        HIP_TRY(f.upload(c));
        PadArgs a{};
        a.tr = f.desc_ptr(c);
        a.out = f.out_ptr(c);
        a.ntraces = m;
        a.scratch = d_scratch;
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
          Layout lo;
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
        int rc;
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
        return timing_end(ctx);
      },
      [&](uint32_t t) {
        const PadOut& o = f.res[t];
        out->status[t] = o.status;
        out->nsamples_out[t] = o.nsamples_out; out->ncalls_out[t] = o.ncalls_out;
        if (o.status == TRACYHIP_PAD_DEFERRED) { ctx->pad_stats.pad_deferred += 1; return; }  // status and zero sizes, nothing else
        if (o.status == TRACYHIP_PAD_TOO_SMALL) ctx->pad_stats.pad_too_small += 1;
        out->leading_gaps[t] = o.leading; out->trailing_gaps[t] = o.trailing; out->step[t] = o.step;
      },
      [&](const PadChunk& c) {
        const uint8_t* dout = static_cast<const uint8_t*>(ctx->dev[PD_OUT].p);
        RunMerger<1, CopyBackRun<1>> rs{{samples ? sb : 0}, {ctx, {dout + o_sig}, {static_cast<uint8_t*>(out->signal)}}};
        RunMerger<5, CopyBackRun<5>> rcall{{out->bcpos ? 4u : 0u}, {ctx, {dout + o_pos}, {reinterpret_cast<uint8_t*>(out->bcpos)}}};
        for (int k = 0; k < 4; ++k) {
          rcall.width[1 + k] = want_byte[k] ? 1 : 0;
          rcall.emit.src[1 + k] = dout + o_byte[k]; rcall.emit.dst[1 + k] = want_byte[k];
        }
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          if (f.res[t].status != TRACYHIP_PAD_OK) continue;
          if (samples) HIP_TRY(rs.add(f.meta[t].out_sig_off, out->sample_offset[t], 4ull * f.res[t].nsamples_out));
          if (calls) HIP_TRY(rcall.add(f.meta[t].out_call_off, out->call_offset[t], f.res[t].ncalls_out));
        }
        HIP_TRY(rs.flush());
        HIP_TRY(rcall.flush());
        return TRACYHIP_OK;
      });
}

int tracyhip_pad_traces_async(tracyhip_ctx* ctx, const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out) {
  return async_twin(tracyhip_pad_traces, ctx, job, mem, out);
}

}  // extern "C"
