// basecall.hip -- tracyhip_basecall_traces: raw chromatograms in, basecalls + qualities + peak table + trims + profiles out, on the device
// (basecall abif.h:408-511, estimateQualities / findBestTraceSection abif.h:164-253, trimTrace trim.h:35-73, createProfile
// profile.h:21-52), bit-identical with the host chain of tracy_amd/host for every trace it answers; the rest is DEFERRED to the host.
//
// One wave per trace, four traces per workgroup; the per-trace body, its data flow and its floating-point rules are basecall_wave.h's
// (compiled for the host wave by tests/emu/emu_basecall.cpp), the wave dev_wave.h's SoloWave.  Each wave owns 8 KB of the workgroup's
// LDS: the chromatogram tile of the 64 basecalls it is working on, later the neighbourhoods of the quality scans.  What is refused
// before a device is touched, the cut into chunks and the descriptors are basecall_plan.h's.
//
// Floating point: float where the reference holds a float (window borders, ratios, the profile's sums and fractions), double where it
// promotes (border arithmetic, mean spacing, spread, quality scaling, the 0.25 blend, the trim limit); every rounding point is listed at
// the top of basecall_wave.h.  No contraction (the pragma below and the build's -ffp-contract=off: 60.0 - scaling * p gives other
// qualities fused), fp32 division correctly rounded (hipcc's default; this file must not be built with fast-math).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "basecall_plan.h"
#include "basecall_wave.h"
#include "capi_internal.h"
#include "dev_wave.h"

#pragma clang fp contract(off)

using namespace tracyhip;

static_assert(TRACYHIP_BASECALL_OK == kBcStatusOk && TRACYHIP_BASECALL_DEFERRED == kBcStatusDeferred, "status codes");

namespace {

constexpr uint32_t kBcWaves = 4;  // traces per workgroup

template <bool S16>
__global__ __launch_bounds__(64 * kBcWaves) void basecall_kernel(BasecallArgs a) {
  const uint32_t t = blockIdx.x * kBcWaves + (threadIdx.x >> 6);
  if (t >= a.ntraces) return;  // (the whole wave)
  SoloWave<kBcWaves, kBcLdsBytes> w;
  basecall_wave_body<S16>(w, a, t);
}

int validate(const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) {
  const char* why = basecall_validate(job, mem, out);
  return why ? set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: %s", why) : TRACYHIP_OK;
}

}  // namespace

extern "C" {

int tracyhip_basecall_validate(const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) { return validate(job, mem, out); }

// Host payloads go through in chunks of consecutive traces whose staged chromatogram fits the workspace limit
// (tracyhip_set_workspace_limit; 256 MB without one) -- the results are the same for any limit -- device payloads in one.  A trace
// whose signal_offset + 4 * nsamples or pos_offset + npos leaves 64 bits is refused with TRACYHIP_ERR_RANGE before the first launch:
// nothing is written.  (The cut is ragged_plan.h's cut_spans.  The frame is not two_pass.h's: this call keeps its descriptors per chunk and
// waits per chunk with device payloads too, so folding it in would change its stream order.)
int tracyhip_basecall_traces(tracyhip_ctx* ctx, const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) {
  int rc = validate(job, mem, out);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const uint32_t n = job->ntraces;
  if (n == 0) return TRACYHIP_OK;
  rc = ctx_begin(ctx);
  if (rc != TRACYHIP_OK) return rc;
  const bool host = mem == TRACYHIP_MEM_HOST;
  const uint32_t sb = job->sample_bytes;
  float stringency = job->trim_stringency;
  if (stringency != 0) stringency = stringency > 9 ? 9.0f : stringency < 1 ? 1.0f : stringency;  // as the commands clamp -t
  std::vector<BasecallChunk> chunks;
  uint32_t bad_t = 0;
  if (!basecall_cut_chunks(job, host, ctx->ws_limit ? ctx->ws_limit : 256ull << 20, chunks, &bad_t))
    return set_error(TRACYHIP_ERR_RANGE, "tracyhip_basecall_traces: an offset + length of trace %u leaves 64 bits", bad_t);
  // the payloads in the order of `widths`; null: not wanted
  uint8_t* const user[7] = {out->primary, out->secondary, out->consensus, out->estqual, reinterpret_cast<uint8_t*>(out->bcpos),
                            reinterpret_cast<uint8_t*>(out->peaks), reinterpret_cast<uint8_t*>(out->profiles)};
  const uint32_t widths[7] = {1, 1, 1, 1, 4, 16, 24};
  std::vector<BasecallTrace> meta;
  std::vector<BasecallOut> res;
  for (const BasecallChunk& c : chunks) {
    const uint32_t m = c.t1 - c.t0;
    meta.resize(m);
    uint64_t scratch_words = 0;
    for (uint32_t i = 0; i < m; ++i) {
      meta[i] = basecall_trace_desc(job, c, host, c.t0 + i, scratch_words);
      scratch_words += basecall_scratch_words(job, c.t0 + i);
    }
    const size_t b_out = (sizeof(BasecallTrace) * m + 15) & ~size_t(15);
    uint8_t* d0; HIP_TRY(ensure_into(ctx->dev[DB_BCALL_TRACES], b_out + sizeof(BasecallOut) * m, d0));
    HIP_TRY(hipMemcpyAsync(d0, meta.data(), sizeof(BasecallTrace) * m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx->dev[DB_BCALL_SCRATCH].ensure(std::max<uint64_t>(scratch_words, 1) * 4));
    BasecallArgs a{};
    a.signal = job->signal;
    a.pos = job->basecallpos;
    uint8_t* dev[7];  // where the launch writes payload k
    std::copy(user, user + 7, dev);
    Layout lo;  // host: the wanted payloads of the chunk, back to back in one staging buffer
    if (host) {
      HIP_TRY(ctx->dev[DB_BCALL_SIGNAL].ensure(c.sig.size() * sb + 16));
      HIP_TRY(hipMemcpyAsync(ctx->dev[DB_BCALL_SIGNAL].p, static_cast<const uint8_t*>(job->signal) + c.sig.lo * sb, c.sig.size() * sb, hipMemcpyHostToDevice, ctx->stream));
      a.signal = ctx->dev[DB_BCALL_SIGNAL].p;
      HIP_TRY(ctx->dev[DB_BCALL_POS].ensure(c.pos.size() * 4 + 16));
      if (c.pos.size()) HIP_TRY(hipMemcpyAsync(ctx->dev[DB_BCALL_POS].p, job->basecallpos + c.pos.lo, c.pos.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      a.pos = static_cast<const int32_t*>(ctx->dev[DB_BCALL_POS].p);
      for (int k = 0; k < 7; ++k) lo.add(user[k] ? c.pos.size() * widths[k] : 0);
      uint8_t* d4; HIP_TRY(ensure_into(ctx->dev[DB_BCALL_PAY], lo.total(), d4));
      for (int k = 0; k < 7; ++k) dev[k] = user[k] ? d4 + lo.at[k] : nullptr;
    }
    a.tr = reinterpret_cast<const BasecallTrace*>(d0);
    a.out = reinterpret_cast<BasecallOut*>(d0 + b_out);
    a.scratch = static_cast<uint32_t*>(ctx->dev[DB_BCALL_SCRATCH].p);
    a.primary = dev[0]; a.secondary = dev[1]; a.consensus = dev[2]; a.estqual = dev[3];
    a.bcpos = reinterpret_cast<int32_t*>(dev[4]); a.peaks = reinterpret_cast<int32_t*>(dev[5]); a.profiles = reinterpret_cast<float*>(dev[6]);
    a.ntraces = m;
    a.sigratio = job->sigratio;
    a.stringency = stringency;
    const dim3 grid((m + kBcWaves - 1) / kBcWaves), block(64 * kBcWaves);
    if (sb == 2) hipLaunchKernelGGL(basecall_kernel<true>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(basecall_kernel<false>, grid, block, 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    res.resize(m);
    HIP_TRY(hipMemcpyAsync(res.data(), a.out, sizeof(BasecallOut) * m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx_sync(ctx));  // the one synchronisation of a device call: bc_len is the HOST length[] of the seqset the caller builds next
    // host payloads: exactly bc_len entries per answered trace go back, straight into the caller's arrays (the rest of a trace's region
    // stays as the caller left it); a batch of ordinary traces, their regions full and following each other, is one run
    const bool staged = lo.at[lo.n] != 0;  // (never with device payloads)
    RunMerger<7, CopyBackRun<7>> back{{}, {ctx, {}, {}}};
    for (int k = 0; k < 7; ++k) {
      back.width[k] = user[k] ? widths[k] : 0;
      back.emit.src[k] = dev[k]; back.emit.dst[k] = user[k];
    }
    for (uint32_t i = 0; i < m; ++i) {
      const BasecallOut& o = res[i];
      const uint32_t t = c.t0 + i;
      out->status[t] = o.status;
      out->bc_len[t] = o.status == TRACYHIP_BASECALL_OK ? o.bc_len : 0;
      if (o.status != TRACYHIP_BASECALL_OK) continue;  // deferred: nothing else is written
      out->trim_left[t] = o.trim_left;
      out->trim_right[t] = o.trim_right;
      out->best_section[t] = o.best_section;
      if (staged) HIP_TRY(back.add(meta[i].pos_off, job->pos_offset[t], o.bc_len));
    }
    if (staged) {
      HIP_TRY(back.flush());
      HIP_TRY(ctx_sync(ctx));
    }
  }
  return TRACYHIP_OK;
}

int tracyhip_basecall_traces_async(tracyhip_ctx* ctx, const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) {
  return async_twin(tracyhip_basecall_traces, ctx, job, mem, out);
}

}  // extern "C"
