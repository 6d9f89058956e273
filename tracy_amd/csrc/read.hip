// read.hip -- tracyhip_read_traces: ABIF and SCF file images turned into chromatograms, call positions, letters and qualities on the device
// (readab abif.h:286-405, traceFormat scf.h:18-34, readscf scf.h:38-102), equal in every field to tracy_amd/host/trace_io.hpp for every
// file it answers; the rest is DEFERRED to the host reader.
//
// Two launches: one wave per file scans header and directory into a descriptor (the sizes-only form ends here), one wave per (file, tile)
// writes the payloads.  Four waves per workgroup; the bodies are read_wave.h's (compiled for the host wave by tests/emu/emu_read.cpp), the
// wave dev_wave.h's SoloWave without LDS of its own.  What is refused before a device is touched, the bound, the cut into chunks and the
// descriptors are read_plan.h's; the frame of the call -- chunk loop, descriptor and result buffer, waits -- is two_pass.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "dev_wave.h"
#include "read_plan.h"
#include "read_wave.h"
#include "two_pass.h"

using namespace tracyhip;

static_assert(TRACYHIP_READ_OK == kReadStatusOk && TRACYHIP_READ_DEFERRED == kReadStatusDeferred && TRACYHIP_READ_TOO_SMALL == kReadStatusTooSmall, "status codes");

namespace {

constexpr uint32_t kReadWaves = 4;  // waves per workgroup

using ReadWave = SoloWave<kReadWaves, 16>;  // (lds() is never called: no LDS is allocated)

__global__ __launch_bounds__(64 * kReadWaves) void read_scan_kernel(ReadArgs a) {
  const uint32_t t = blockIdx.x * kReadWaves + (threadIdx.x >> 6);
  if (t >= a.ntraces) return;  // (the whole wave)
  ReadWave w;
  read_scan_body(w, a, t);
}

template <bool S16>
__global__ __launch_bounds__(64 * kReadWaves) void read_emit_kernel(ReadArgs a) {
  const uint32_t tile = blockIdx.x * kReadWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  ReadWave w;
  read_emit_body<S16>(w, a, tile);
}

int validate(const tracyhip_read_job* job, int mem, const tracyhip_read_result* out) {
  const char* why = read_validate(job, mem, out);
  return why ? set_error(TRACYHIP_ERR_ARG, "tracyhip_read_traces: %s", why) : TRACYHIP_OK;
}

}  // namespace

extern "C" {

int tracyhip_read_validate(const tracyhip_read_job* job, int mem, const tracyhip_read_result* out) { return validate(job, mem, out); }

int tracyhip_read_bound(uint32_t file_len, uint32_t* nsamples_max, uint32_t* ncalls_max) {
  if (!nsamples_max || !ncalls_max) return set_error(TRACYHIP_ERR_ARG, "tracyhip_read_bound: null nsamples_max / ncalls_max");
  *nsamples_max = read_bound_samples(file_len);
  *ncalls_max = read_bound_calls(file_len);
  return TRACYHIP_OK;
}

int tracyhip_last_read_stats(tracyhip_ctx* ctx, tracyhip_read_stats* out) { return last_stats(ctx, &tracyhip_ctx::read_stats, out); }

int tracyhip_read_traces(tracyhip_ctx* ctx, const tracyhip_read_job* job, int mem, const tracyhip_read_result* out) {
  int rc = validate(job, mem, out);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const bool host = mem == TRACYHIP_MEM_HOST;
  TwoPass<ReadFile, ReadDesc, ReadChunk> f{ctx, job->ntraces, host};
  rc = f.begin("tracyhip_read_traces", "trace", DB_READ_FILES, &tracyhip_ctx::read_stats, &tracyhip_read_stats::read_chunks,
               [&](uint64_t limit, std::vector<ReadChunk>& chunks, uint32_t* bad_t) { return read_cut_chunks(job, out, host, limit, chunks, bad_t); });
  if (rc != TRACYHIP_OK || f.chunks.empty()) return rc;
  const uint32_t sb = job->sample_bytes;
  const bool samples = read_wants_samples(out), calls = read_wants_calls(out);
  uint8_t* const want_byte[3] = {out->basecalls1, out->basecalls2, out->qual};
  uint64_t o_sig = 0, o_pos = 0, o_byte[3] = {0, 0, 0};  // the staged results of a host chunk
  return f.run(
      samples || calls,
      [&](const ReadChunk& c) {
        const uint32_t m = c.t1 - c.t0;
        uint32_t tile_first = 0;
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          f.meta[t] = read_file_desc(job, out, c, host, t, tile_first);
          tile_first += read_file_tiles(job->file_len[t]);
        }
        HIP_TRY(f.upload(c));
        ReadArgs a{};
        a.fl = f.desc_ptr(c);
        a.desc = f.out_ptr(c);
        a.ntraces = m; a.ntiles = tile_first; a.sample_bytes = sb;
        if (host) {
          uint8_t* din; HIP_TRY(ensure_into(ctx->dev[DB_READ_IN], c.in.size() + 16, din));
          if (c.in.size()) HIP_TRY(hipMemcpyAsync(din, job->bytes + c.in.lo, c.in.size(), hipMemcpyHostToDevice, ctx->stream));
          a.bytes = din;
          Layout lo;
          o_sig = lo.add(samples ? c.osig.size() * sb : 0);
          o_pos = lo.add(out->basecallpos ? c.ocall.size() * 4 : 0);
          for (int k = 0; k < 3; ++k) o_byte[k] = lo.add(want_byte[k] ? c.ocall.size() : 0);
          uint8_t* dout; HIP_TRY(ensure_into(ctx->dev[DB_READ_OUT], lo.total(), dout));
          if (samples) a.o_signal = dout + o_sig;
          if (out->basecallpos) a.o_pos = reinterpret_cast<int32_t*>(dout + o_pos);
          if (want_byte[0]) a.o_b1 = dout + o_byte[0];
          if (want_byte[1]) a.o_b2 = dout + o_byte[1];
          if (want_byte[2]) a.o_qual = dout + o_byte[2];
        } else {
          a.bytes = job->bytes;
          a.o_signal = out->signal; a.o_pos = out->basecallpos;
          a.o_b1 = out->basecalls1; a.o_b2 = out->basecalls2; a.o_qual = out->qual;
        }
        int rc;
        if (ctx->timing) {
          uint64_t moved = 0;  // (the images read once; what is written is about as much again at 16 bits, twice at 32)
          for (uint32_t t = c.t0; t < c.t1; ++t) moved += (uint64_t)job->file_len[t] * (samples ? 1 + sb / 2 : 1);
          if ((rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, moved))) return rc;
        }
        const dim3 block(64 * kReadWaves), sgrid((m + kReadWaves - 1) / kReadWaves), tgrid((a.ntiles + kReadWaves - 1) / kReadWaves);
        hipLaunchKernelGGL(read_scan_kernel, sgrid, block, 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        if (samples || calls) {
          if (sb == 2) hipLaunchKernelGGL(read_emit_kernel<true>, tgrid, block, 0, ctx->stream, a);
          else hipLaunchKernelGGL(read_emit_kernel<false>, tgrid, block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        return timing_end(ctx);
      },
      [&](uint32_t t) {
        const ReadDesc& o = f.res[t];
        out->status[t] = o.status; out->format[t] = o.format;
        out->nsamples[t] = o.nsamples; out->ncalls[t] = o.ncalls;
        if (o.status == TRACYHIP_READ_DEFERRED) ctx->read_stats.read_deferred += 1;
        if (o.status == TRACYHIP_READ_TOO_SMALL) ctx->read_stats.read_too_small += 1;
      },
      [&](const ReadChunk& c) {
        const uint8_t* dout = static_cast<const uint8_t*>(ctx->dev[DB_READ_OUT].p);
        RunMerger<1, CopyBackRun<1>> rs{{samples ? sb : 0}, {ctx, {dout + o_sig}, {static_cast<uint8_t*>(out->signal)}}};
        RunMerger<4, CopyBackRun<4>> rcall{{out->basecallpos ? 4u : 0u}, {ctx, {dout + o_pos}, {reinterpret_cast<uint8_t*>(out->basecallpos)}}};
        for (int k = 0; k < 3; ++k) {
          rcall.width[1 + k] = want_byte[k] ? 1 : 0;
          rcall.emit.src[1 + k] = dout + o_byte[k]; rcall.emit.dst[1 + k] = want_byte[k];
        }
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          if (f.res[t].status != TRACYHIP_READ_OK) continue;
          if (samples) HIP_TRY(rs.add(f.meta[t].out_sig_off, out->sample_offset[t], 4ull * f.res[t].nsamples));
          if (calls) HIP_TRY(rcall.add(f.meta[t].out_call_off, out->call_offset[t], f.res[t].ncalls));
        }
        HIP_TRY(rs.flush());
        HIP_TRY(rcall.flush());
        return TRACYHIP_OK;
      });
}

int tracyhip_read_traces_async(tracyhip_ctx* ctx, const tracyhip_read_job* job, int mem, const tracyhip_read_result* out) {
  return async_twin(tracyhip_read_traces, ctx, job, mem, out);
}

}  // extern "C"
