// render.hip -- tracyhip_render_traces: the per-trace text of the three writers of the commands (traceTxtOut abif.h:513-533,
// _traceJsonOut json.h:33-105, assemblyTrace json.h:120-194) composed on the device, equal byte for byte to tracy_amd/host for every
// trace it answers; the rest is DEFERRED to the host.
//
// Three launches: one wave per tile counts its bytes, one wave per trace scans its tiles (offsets, text_len, status), one wave per
// tile composes its items in LDS and stores them.  Four waves per workgroup, each with its own kRenderLdsBytes of LDS; the bodies are
// render_wave.h's (compiled for the host wave by tests/emu/emu_render.cpp), the wave dev_wave.h's SoloWave.  What is refused before a
// device is touched, the bound, the cut into chunks and the descriptors are render_plan.h's; the frame of the call -- chunk loop,
// descriptor and result buffer, waits -- is two_pass.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "dev_wave.h"
#include "render_plan.h"
#include "render_wave.h"
#include "two_pass.h"

using namespace tracyhip;

static_assert(TRACYHIP_RENDER_OK == kRenderStatusOk && TRACYHIP_RENDER_DEFERRED == kRenderStatusDeferred &&
              TRACYHIP_RENDER_TOO_SMALL == kRenderStatusTooSmall, "status codes");
static_assert(TRACYHIP_RENDER_TSV == kRenderTsv && TRACYHIP_RENDER_JSON == kRenderJson && TRACYHIP_RENDER_GAPPED == kRenderGapped, "forms");

namespace {

constexpr uint32_t kRenderWaves = 4;  // waves per workgroup

using RenderWave = SoloWave<kRenderWaves, kRenderLdsBytes>;

template <bool S16>
__global__ __launch_bounds__(64 * kRenderWaves) void render_count_kernel(RenderArgs a) {
  const uint32_t tile = blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;  // (the whole wave)
  RenderWave w;
  render_count_body<S16>(w, a, tile);
}

__global__ __launch_bounds__(64 * kRenderWaves) void render_scan_kernel(RenderArgs a) {
  const uint32_t t = blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  if (t >= a.ntraces) return;
  RenderWave w;
  render_scan_body(w, a, t);
}

template <bool S16>
__global__ __launch_bounds__(64 * kRenderWaves) void render_emit_kernel(RenderArgs a) {
  const uint32_t tile = blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  RenderWave w;
  render_emit_body<S16>(w, a, tile);
}

int validate(const tracyhip_render_job* job, int mem, const tracyhip_render_result* out) {
  const char* why = render_validate(job, mem, out);
  return why ? set_error(TRACYHIP_ERR_ARG, "tracyhip_render_traces: %s", why) : TRACYHIP_OK;
}

}  // namespace

extern "C" {

int tracyhip_render_validate(const tracyhip_render_job* job, int mem, const tracyhip_render_result* out) { return validate(job, mem, out); }

uint64_t tracyhip_render_bound(uint32_t form, uint32_t nsamples, uint32_t bc_len, uint32_t sample_bytes) {
  return render_bound(form, nsamples, bc_len, sample_bytes);
}

int tracyhip_last_render_stats(tracyhip_ctx* ctx, tracyhip_render_stats* out) { return last_stats(ctx, &tracyhip_ctx::render_stats, out); }

int tracyhip_render_traces(tracyhip_ctx* ctx, const tracyhip_render_job* job, int mem, const tracyhip_render_result* out) {
  int rc = validate(job, mem, out);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const bool host = mem == TRACYHIP_MEM_HOST, payload = out->text != nullptr, tsv = job->form == TRACYHIP_RENDER_TSV;
  TwoPass<RenderTrace, RenderOut, RenderChunk> f{ctx, job->ntraces, host};
  rc = f.begin("tracyhip_render_traces", "trace", DB_RENDER_TRACES, &tracyhip_ctx::render_stats, &tracyhip_render_stats::render_chunks,
               [&](uint64_t limit, std::vector<RenderChunk>& chunks, uint32_t* bad_t) { return render_cut_chunks(job, out, host, limit, chunks, bad_t); });
  if (rc != TRACYHIP_OK || f.chunks.empty()) return rc;
  const uint32_t sb = job->sample_bytes;
  uint64_t max_tiles = 1;  // sized once for the largest chunk: the launches of a device call follow each other without a wait
  for (const RenderChunk& c : f.chunks) max_tiles = std::max(max_tiles, c.tiles);
  uint32_t* d_tiles; HIP_TRY(ensure_into(ctx->dev[DB_RENDER_TILES], 2 * max_tiles, d_tiles));
  const uint8_t* d_text = nullptr;  // the staged text of a host chunk
  return f.run(
      payload,
      [&](const RenderChunk& c) {
        const uint32_t m = c.t1 - c.t0;
        uint32_t tile_first = 0;
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          f.meta[t] = render_trace_desc(job, out, c, host, t, tile_first);
          tile_first += render_trace_tiles(job, t);
        }
        HIP_TRY(f.upload(c));
        RenderArgs a{};
        a.tr = f.desc_ptr(c);
        a.out = f.out_ptr(c);
        a.ntraces = m; a.ntiles = tile_first; a.form = job->form;
        a.tile_bytes = d_tiles; a.tile_aux = d_tiles + max_tiles;
        if (host) {
          // inputs: the elements of each span, first element at the part's start
          Layout li;
          const uint64_t i_pos = li.add(c.bc.size() * 4);
          const uint8_t* const in_byte[4] = {job->primary, job->secondary, tsv ? job->consensus : nullptr, job->estqual};
          uint64_t i_byte[4];
          for (int k = 0; k < 4; ++k) i_byte[k] = li.add(in_byte[k] ? c.bc.size() : 0);
          const uint64_t i_sig = li.add(c.sig.size() * sb);
          uint8_t* din; HIP_TRY(ensure_into(ctx->dev[DB_RENDER_IN], li.total(), din));
          auto up = [&](uint64_t at, const void* src, uint64_t bytes) {
            return bytes ? hipMemcpyAsync(din + at, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
          };
          HIP_TRY(up(i_pos, job->bcpos + c.bc.lo, c.bc.size() * 4));
          for (int k = 0; k < 4; ++k)
            if (in_byte[k]) HIP_TRY(up(i_byte[k], in_byte[k] + c.bc.lo, c.bc.size()));
          HIP_TRY(up(i_sig, static_cast<const uint8_t*>(job->signal) + c.sig.lo * sb, c.sig.size() * sb));
          a.bcpos = reinterpret_cast<const int32_t*>(din + i_pos);
          a.primary = din + i_byte[0]; a.secondary = din + i_byte[1];
          a.consensus = in_byte[2] ? din + i_byte[2] : nullptr;
          a.estqual = din + i_byte[3];
          a.signal = din + i_sig;
          if (payload) {
            uint8_t* dout; HIP_TRY(ensure_into(ctx->dev[DB_RENDER_OUT], c.text.size() + 16, dout));
            a.text = dout;
          }
          d_text = a.text;
        } else {
          a.signal = job->signal; a.bcpos = job->bcpos;
          a.primary = job->primary; a.secondary = job->secondary; a.consensus = tsv ? job->consensus : nullptr; a.estqual = job->estqual;
          a.text = out->text;
        }
        int rc;
        if (ctx->timing) {
          uint64_t moved = 0;
          for (uint32_t t = c.t0; t < c.t1; ++t) moved += 4ull * sb * job->nsamples[t] * (payload ? 2 : 1);  // (the chromatogram, once per pass)
          if ((rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, moved))) return rc;
        }
        const dim3 block(64 * kRenderWaves), tgrid((a.ntiles + kRenderWaves - 1) / kRenderWaves), sgrid((m + kRenderWaves - 1) / kRenderWaves);
        if (a.ntiles) {
          if (sb == 2) hipLaunchKernelGGL(render_count_kernel<true>, tgrid, block, 0, ctx->stream, a);
          else hipLaunchKernelGGL(render_count_kernel<false>, tgrid, block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(render_scan_kernel, sgrid, block, 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        if (payload && a.ntiles) {
          if (sb == 2) hipLaunchKernelGGL(render_emit_kernel<true>, tgrid, block, 0, ctx->stream, a);
          else hipLaunchKernelGGL(render_emit_kernel<false>, tgrid, block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        return timing_end(ctx);
      },
      [&](uint32_t t) {
        out->status[t] = f.res[t].status;
        out->text_len[t] = f.res[t].text_len;
        if (f.res[t].status == TRACYHIP_RENDER_DEFERRED) ctx->render_stats.render_deferred += 1;
        if (f.res[t].status == TRACYHIP_RENDER_TOO_SMALL) ctx->render_stats.render_too_small += 1;
      },
      [&](const RenderChunk& c) {
        RunMerger<1, CopyBackRun<1>> rt{{1u}, {ctx, {d_text}, {out->text}}};
        for (uint32_t t = c.t0; t < c.t1; ++t)
          if (f.res[t].status == TRACYHIP_RENDER_OK) HIP_TRY(rt.add(f.meta[t].text_off, out->text_offset[t], f.res[t].text_len));
        HIP_TRY(rt.flush());
        return TRACYHIP_OK;
      });
}

int tracyhip_render_traces_async(tracyhip_ctx* ctx, const tracyhip_render_job* job, int mem, const tracyhip_render_result* out) {
  return async_twin(tracyhip_render_traces, ctx, job, mem, out);
}

}  // extern "C"
