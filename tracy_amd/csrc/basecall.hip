// basecall.hip -- tracyhip_basecall_traces: raw chromatograms in, basecalls + qualities + peak table + trims + profiles out, on the device
// (basecall abif.h:408-511, estimateQualities / findBestTraceSection abif.h:164-253, trimTrace trim.h:35-73, createProfile
// profile.h:21-52), bit-identical with the host chain of tracy_amd/host for every trace it answers; the rest is DEFERRED to the host.
//
// One wave per trace, four traces per workgroup; the per-trace body, its data flow and its floating-point rules are basecall_wave.h's
// (compiled for the host wave by tests/emu/emu_basecall.cpp).  Each wave owns 8 KB of the workgroup's LDS: the chromatogram tile of the
// 64 basecalls it is working on, later the neighbourhoods of the quality scans.  Waves never wait for each other: a wave's sync is a
// memory fence and a wave barrier, not a workgroup barrier.
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
#include "basecall_wave.h"
#include "capi_internal.h"

#pragma clang fp contract(off)

using namespace tracyhip;

static_assert(TRACYHIP_BASECALL_OK == kBcStatusOk && TRACYHIP_BASECALL_DEFERRED == kBcStatusDeferred, "status codes");

namespace {

constexpr uint32_t kBcWaves = 4;  // traces per workgroup

struct BasecallDevWave {
  __device__ __forceinline__ uint32_t lane() const { return threadIdx.x & 63u; }
  __device__ __forceinline__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ __forceinline__ uint32_t bcast(uint32_t x, uint32_t src_lane) const { return (uint32_t)__shfl((int)x, (int)src_lane, 64); }
  // the wave's own LDS and global writes become visible to its own lanes: no other wave shares them
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void sync_global() const { sync(); }
  __device__ __forceinline__ char* lds() const {
    __shared__ __attribute__((aligned(16))) char bc_smem[kBcWaves * kBcLdsBytes];
    return bc_smem + (threadIdx.x >> 6) * kBcLdsBytes;
  }
  template <class F>
  __device__ __forceinline__ uint32_t reduce(uint32_t x, F f) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = f(x, (uint32_t)__shfl_xor((int)x, o, 64));
    return x;
  }
  __device__ __forceinline__ uint32_t sum(uint32_t x) const { return reduce(x, [](uint32_t a, uint32_t b) { return a + b; }); }
  __device__ __forceinline__ uint32_t umin(uint32_t x) const { return reduce(x, [](uint32_t a, uint32_t b) { return a < b ? a : b; }); }
  __device__ __forceinline__ uint32_t umax(uint32_t x) const { return reduce(x, [](uint32_t a, uint32_t b) { return a > b ? a : b; }); }
  __device__ __forceinline__ uint32_t excl_sum(uint32_t x) const {  // sum of the lanes below (Hillis-Steele, six shuffles)
    uint32_t v = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)v, o, 64);
      if ((int)lane() >= o) v += y;
    }
    return v - x;
  }
};

template <bool S16>
__global__ __launch_bounds__(64 * kBcWaves) void basecall_kernel(BasecallArgs a) {
  const uint32_t t = blockIdx.x * kBcWaves + (threadIdx.x >> 6);
  if (t >= a.ntraces) return;  // (the whole wave)
  BasecallDevWave w;
  basecall_wave_body<S16>(w, a, t);
}

int validate(const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) {
  if (!job || !out) return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: null job / result");
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: bad mem");
  if (job->sample_bytes != 2 && job->sample_bytes != 4) return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: sample_bytes must be 2 or 4");
  if (std::isnan(job->sigratio)) return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: sigratio is not a number");
  if (std::isnan(job->trim_stringency) || job->trim_stringency < 0) return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: trim_stringency must be 0 or positive");
  if (job->ntraces == 0) return TRACYHIP_OK;
  if (!job->signal || !job->signal_offset || !job->nsamples || !job->basecallpos || !job->pos_offset || !job->npos)
    return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: null signal / basecallpos or one of their offset and length arrays");
  if (reinterpret_cast<uintptr_t>(job->signal) % job->sample_bytes || reinterpret_cast<uintptr_t>(job->basecallpos) % 4)
    return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: signal / basecallpos not aligned to their element size");
  if (!out->status || !out->bc_len || !out->trim_left || !out->trim_right || !out->best_section)
    return set_error(TRACYHIP_ERR_ARG, "tracyhip_basecall_traces: null per-trace result array (status, bc_len, trim_left, trim_right, best_section)");
  return TRACYHIP_OK;
}

// device addresses of the payload results a launch writes
struct Payload {
  uint8_t *primary = nullptr, *secondary = nullptr, *consensus = nullptr, *estqual = nullptr;
  int32_t *bcpos = nullptr, *peaks = nullptr;
  float* profiles = nullptr;
};

}  // namespace

extern "C" {

int tracyhip_basecall_validate(const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) { return validate(job, mem, out); }

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
  auto answerable = [&](uint32_t t) { return job->npos[t] >= 1 && job->npos[t] <= kBcMaxPos && job->nsamples[t] >= 3 && job->nsamples[t] <= kBcMaxSamples; };
  // host payloads go through in chunks of consecutive traces (at most ~256 MB of staged chromatogram), device payloads in one
  const uint64_t chunk_bytes = 256ull << 20;
  std::vector<BasecallTrace> meta;
  std::vector<BasecallOut> res;
  for (uint32_t t0 = 0; t0 < n;) {
    uint64_t slo = ~0ull, shi = 0, plo = ~0ull, phi = 0;
    uint32_t t1 = t0;
    for (; t1 < n; ++t1) {
      const uint64_t a0 = job->signal_offset[t1], a1 = a0 + 4ull * job->nsamples[t1], p0 = job->pos_offset[t1], p1 = p0 + job->npos[t1];
      const uint64_t nslo = std::min(slo, a0), nshi = std::max(shi, a1);
      if (host && t1 > t0 && (nshi - nslo) * sb > chunk_bytes) break;
      slo = nslo; shi = nshi;
      plo = std::min(plo, p0); phi = std::max(phi, p1);
    }
    const uint32_t m = t1 - t0;
    if (!host) slo = plo = 0;
    const uint64_t span = phi - plo;  // result elements of the chunk
    meta.resize(m);
    uint64_t scratch_words = 0;
    for (uint32_t i = 0; i < m; ++i) {
      const uint32_t t = t0 + i;
      meta[i] = BasecallTrace{job->signal_offset[t] - slo, job->pos_offset[t] - plo, scratch_words, job->nsamples[t], job->npos[t]};
      if (answerable(t)) scratch_words += 3ull * job->npos[t] + 1;
    }
    const size_t b_meta = 0, b_out = (b_meta + sizeof(BasecallTrace) * m + 15) & ~size_t(15), b_end = b_out + sizeof(BasecallOut) * m;
    uint8_t* d0; HIP_TRY(ensure_into(ctx->dev[DB_BCALL_TRACES], b_end, d0));
    HIP_TRY(hipMemcpyAsync(d0 + b_meta, meta.data(), sizeof(BasecallTrace) * m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx->dev[DB_BCALL_SCRATCH].ensure(std::max<uint64_t>(scratch_words, 1) * 4));
    BasecallArgs a{};
    a.signal = job->signal;
    a.pos = job->basecallpos;
    Payload pl;
    // the wanted payloads of a host chunk, back to back in one staging buffer in the order of `widths`
    const void* wanted[7] = {out->primary, out->secondary, out->consensus, out->estqual, out->bcpos, out->peaks, out->profiles};
    const uint32_t widths[7] = {1, 1, 1, 1, 4, 16, 24};
    uint64_t at[8] = {0};
    if (host) {
      HIP_TRY(ctx->dev[DB_BCALL_SIGNAL].ensure((shi - slo) * sb + 16));
      HIP_TRY(hipMemcpyAsync(ctx->dev[DB_BCALL_SIGNAL].p, static_cast<const uint8_t*>(job->signal) + slo * sb, (shi - slo) * sb, hipMemcpyHostToDevice, ctx->stream));
      a.signal = ctx->dev[DB_BCALL_SIGNAL].p;
      HIP_TRY(ctx->dev[DB_BCALL_POS].ensure(span * 4 + 16));
      if (span) HIP_TRY(hipMemcpyAsync(ctx->dev[DB_BCALL_POS].p, job->basecallpos + plo, span * 4, hipMemcpyHostToDevice, ctx->stream));
      a.pos = static_cast<const int32_t*>(ctx->dev[DB_BCALL_POS].p);
      for (int k = 0; k < 7; ++k) at[k + 1] = at[k] + (wanted[k] ? ((span * widths[k] + 15) & ~15ull) : 0);
      uint8_t* d4; HIP_TRY(ensure_into(ctx->dev[DB_BCALL_PAY], at[7] + 16, d4));
      if (out->primary) pl.primary = d4 + at[0];
      if (out->secondary) pl.secondary = d4 + at[1];
      if (out->consensus) pl.consensus = d4 + at[2];
      if (out->estqual) pl.estqual = d4 + at[3];
      if (out->bcpos) pl.bcpos = reinterpret_cast<int32_t*>(d4 + at[4]);
      if (out->peaks) pl.peaks = reinterpret_cast<int32_t*>(d4 + at[5]);
      if (out->profiles) pl.profiles = reinterpret_cast<float*>(d4 + at[6]);
    } else {
      pl.primary = out->primary; pl.secondary = out->secondary; pl.consensus = out->consensus; pl.estqual = out->estqual;
      pl.bcpos = out->bcpos; pl.peaks = out->peaks; pl.profiles = out->profiles;
    }
    a.tr = reinterpret_cast<const BasecallTrace*>(d0 + b_meta);
    a.out = reinterpret_cast<BasecallOut*>(d0 + b_out);
    a.scratch = static_cast<uint32_t*>(ctx->dev[DB_BCALL_SCRATCH].p);
    a.primary = pl.primary; a.secondary = pl.secondary; a.consensus = pl.consensus; a.estqual = pl.estqual;
    a.bcpos = pl.bcpos; a.peaks = pl.peaks; a.profiles = pl.profiles;
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
    uint8_t* dsts[7] = {out->primary, out->secondary, out->consensus, out->estqual, reinterpret_cast<uint8_t*>(out->bcpos),
                        reinterpret_cast<uint8_t*>(out->peaks), reinterpret_cast<uint8_t*>(out->profiles)};
    // host payloads: exactly bc_len entries per answered trace go back, straight into the caller's arrays.  Traces whose regions follow
    // each other and are full (bc_len == npos) travel as one copy per payload kind -- a batch of ordinary traces is one run.
    uint64_t run_rel = 0, run_dst = 0, run_len = 0;
    auto flush = [&]() -> hipError_t {
      for (int k = 0; k < 7 && run_len; ++k) {
        if (!dsts[k]) continue;
        const hipError_t e = hipMemcpyAsync(dsts[k] + run_dst * widths[k], static_cast<uint8_t*>(ctx->dev[DB_BCALL_PAY].p) + at[k] + run_rel * widths[k],
                                            run_len * widths[k], hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) return e;
      }
      run_len = 0;
      return hipSuccess;
    };
    for (uint32_t i = 0; i < m; ++i) {
      const BasecallOut& o = res[i];
      const uint32_t t = t0 + i;
      out->status[t] = o.status;
      out->bc_len[t] = o.status == TRACYHIP_BASECALL_OK ? o.bc_len : 0;
      if (o.status != TRACYHIP_BASECALL_OK) continue;  // deferred: nothing else is written
      out->trim_left[t] = o.trim_left;
      out->trim_right[t] = o.trim_right;
      out->best_section[t] = o.best_section;
      if (!host || !at[7] || !o.bc_len) continue;
      const uint64_t rel = meta[i].pos_off, dst = job->pos_offset[t];
      if (run_len && (rel != run_rel + run_len || dst != run_dst + run_len)) HIP_TRY(flush());
      if (!run_len) { run_rel = rel; run_dst = dst; }
      run_len += o.bc_len;
      if (o.bc_len != job->npos[t]) HIP_TRY(flush());  // (the rest of the trace's region stays as the caller left it)
    }
    if (host && at[7]) {
      HIP_TRY(flush());
      HIP_TRY(ctx_sync(ctx));
    }
    t0 = t1;
  }
  return TRACYHIP_OK;
}

int tracyhip_basecall_traces_async(tracyhip_ctx* ctx, const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out) {
  if (!ctx || !job || !out) return set_error(TRACYHIP_ERR_ARG, "null context / job / result");
  const tracyhip_basecall_job j = *job;
  const tracyhip_basecall_result o = *out;
  return async_submit(ctx, [=]() { return tracyhip_basecall_traces(ctx, &j, mem, &o); });
}

}  // extern "C"
