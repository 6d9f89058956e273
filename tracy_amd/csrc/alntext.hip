// alntext.hip -- tracyhip_render_alignments: the text the writers of `align` and `decompose` print from the two gapped rows of an alignment
// (plotAlignment fmindex.h:329-427, the FASTA of sage.h:328-339, the tail of traceAlignJsonOut json.h:208-216) composed on the device,
// equal byte for byte to tracy_amd/host for every alignment it answers, the rest DEFERRED to the host; and tracyhip_reference_slices:
// the oriented reference slice of a CHAR-reference align job (reverseComplement fmindex.h:11-25 + substr).
//
// The launches are render.hip's three -- one wave per tile counts its bytes, one wave per alignment scans its tiles (offsets, text_len,
// status), one wave per tile composes its items in LDS and stores them -- and, for a plot, one in front: one wave per tile of columns
// counts the letters of both rows, which the line breaks and the counters of every later tile depend on.  Four waves per workgroup, each with
// its own kAlnLdsBytes of LDS; the bodies are alntext_wave.h's (compiled for the host wave by tests/emu/emu_alntext.cpp), the wave
// dev_wave.h's SoloWave.  What is refused before a device is touched, the bound, the cut into chunks and the descriptors are
// alntext_plan.h's; the frame of tracyhip_render_alignments -- chunk loop, descriptor and result buffer, waits -- is two_pass.h's
// (tracyhip_reference_slices is a single pass over stage_in / stage_out and stays outside it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "alntext_plan.h"
#include "alntext_wave.h"
#include "capi_internal.h"
#include "dev_wave.h"
#include "two_pass.h"

using namespace tracyhip;

static_assert(TRACYHIP_ALNTEXT_OK == kAlnStatusOk && TRACYHIP_ALNTEXT_DEFERRED == kAlnStatusDeferred && TRACYHIP_ALNTEXT_TOO_SMALL == kAlnStatusTooSmall,
              "status codes");
static_assert(TRACYHIP_ALNTEXT_PLOT == kAlnPlot && TRACYHIP_ALNTEXT_FASTA == kAlnFasta && TRACYHIP_ALNTEXT_JSON == kAlnJson, "forms");

namespace {

constexpr uint32_t kAlnWaves = 4;  // waves per workgroup

using AlnWave = SoloWave<kAlnWaves, kAlnLdsBytes>;

__global__ __launch_bounds__(64 * kAlnWaves) void alntext_letters_kernel(AlnArgs a) {
  const uint32_t ct = blockIdx.x * kAlnWaves + (threadIdx.x >> 6);
  if (ct >= a.ncoltiles) return;  // (the whole wave)
  AlnWave w;
  alntext_letters_body(w, a, ct);
}

__global__ __launch_bounds__(64 * kAlnWaves) void alntext_count_kernel(AlnArgs a) {
  const uint32_t tile = blockIdx.x * kAlnWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;  // (the whole wave)
  AlnWave w;
  alntext_count_body(w, a, tile);
}

__global__ __launch_bounds__(64 * kAlnWaves) void alntext_scan_kernel(AlnArgs a) {
  const uint32_t t = blockIdx.x * kAlnWaves + (threadIdx.x >> 6);
  if (t >= a.n) return;
  AlnWave w;
  alntext_scan_body(w, a, t);
}

__global__ __launch_bounds__(64 * kAlnWaves) void alntext_emit_kernel(AlnArgs a) {
  const uint32_t tile = blockIdx.x * kAlnWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  AlnWave w;
  alntext_emit_body(w, a, tile);
}

__global__ __launch_bounds__(64 * kAlnWaves) void slice_kernel(SliceArgs a) {
  const uint32_t tile = blockIdx.x * kAlnWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  DevWaveOps<false> w;
  slice_body(w, a, tile);
}

int validate(const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out) {
  const char* why = alntext_validate(job, mem, out);
  return why ? set_error(TRACYHIP_ERR_ARG, "tracyhip_render_alignments: %s", why) : TRACYHIP_OK;
}

int validate_slices(const tracyhip_slices_job* job, int mem, const uint8_t* out, const uint64_t* out_offset) {
  bool range = false;
  uint32_t bad = 0;
  const char* why = slices_validate(job, mem, out, out_offset, &range, &bad);
  if (!why) return TRACYHIP_OK;
  return range ? set_error(TRACYHIP_ERR_RANGE, "tracyhip_reference_slices: %s (slice %u)", why, bad)
               : set_error(TRACYHIP_ERR_ARG, "tracyhip_reference_slices: %s", why);
}

}  // namespace

extern "C" {

int tracyhip_render_alignments_validate(const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out) {
  return validate(job, mem, out);
}

uint64_t tracyhip_render_alignments_bound(uint32_t form, uint32_t linelimit, uint32_t cols, uint32_t name0_len, uint32_t name1_len) {
  return alntext_bound(form, linelimit, cols, name0_len, name1_len);
}

int tracyhip_last_alntext_stats(tracyhip_ctx* ctx, tracyhip_alntext_stats* out) { return last_stats(ctx, &tracyhip_ctx::alntext_stats, out); }

int tracyhip_render_alignments(tracyhip_ctx* ctx, const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out) {
  int rc = validate(job, mem, out);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const bool host = mem == TRACYHIP_MEM_HOST, payload = out->text != nullptr;
  TwoPass<AlnDesc, AlnOut, AlnChunk> f{ctx, job->n, host};
  rc = f.begin("tracyhip_render_alignments", "alignment", DB_ALNTEXT_DESC, &tracyhip_ctx::alntext_stats, &tracyhip_alntext_stats::alntext_chunks,
               [&](uint64_t limit, std::vector<AlnChunk>& chunks, uint32_t* bad_t) { return alntext_cut_chunks(job, out, host, limit, chunks, bad_t); });
  if (rc != TRACYHIP_OK || f.chunks.empty()) return rc;
  uint64_t max_tiles = 1, max_coltiles = 1;  // sized once for the largest chunk: the launches of a device call follow each other without a wait
  for (const AlnChunk& c : f.chunks) { max_tiles = std::max(max_tiles, c.tiles); max_coltiles = std::max(max_coltiles, c.coltiles); }
  uint32_t* d_tiles; HIP_TRY(ensure_into(ctx->dev[DB_ALNTEXT_TILES], 3 * max_tiles + 2 * max_coltiles, d_tiles));
  const uint8_t* d_text = nullptr;  // the staged text of a host chunk
  return f.run(
      payload,
      [&](const AlnChunk& c) {
        const uint32_t m = c.t1 - c.t0;
        uint32_t tile_first = 0, col_first = 0;
        uint64_t moved = 0;
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          f.meta[t] = alntext_desc(job, out, c, host, t, tile_first, col_first);
          tile_first += alntext_tiles(job, t);
          col_first += alntext_coltiles(job, t);
          moved += 2ull * job->cols[t] * (payload ? 2 : 1);  // (both rows, once per pass)
        }
        HIP_TRY(f.upload(c));
        AlnArgs a{};
        a.al = f.desc_ptr(c);
        a.out = f.out_ptr(c);
        a.n = m; a.ntiles = tile_first; a.ncoltiles = col_first; a.form = job->form;
        a.key = job->form == TRACYHIP_ALNTEXT_PLOT ? job->key : 0u;
        a.linelimit = job->form == TRACYHIP_ALNTEXT_PLOT ? job->linelimit : 1u;
        a.tile_bytes = d_tiles; a.tile_aux = d_tiles + max_tiles; a.col_letters = d_tiles + 3 * max_tiles;
        if (host) {
          // inputs: the bytes of each span, first byte at the part's start
          Layout li;
          const uint64_t i_r0 = li.add(c.rows.size()), i_r1 = li.add(c.rows.size()), i_nm = li.add(c.names.size());
          uint8_t* din; HIP_TRY(ensure_into(ctx->dev[DB_ALNTEXT_IN], li.total(), din));
          auto up = [&](uint64_t at, const void* src, uint64_t bytes) {
            return bytes ? hipMemcpyAsync(din + at, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
          };
          HIP_TRY(up(i_r0, job->rows0 + c.rows.lo, c.rows.size()));
          HIP_TRY(up(i_r1, job->rows1 + c.rows.lo, c.rows.size()));
          HIP_TRY(up(i_nm, job->names + c.names.lo, c.names.size()));
          a.rows0 = din + i_r0; a.rows1 = din + i_r1; a.names = din + i_nm;
          if (payload) {
            uint8_t* dout; HIP_TRY(ensure_into(ctx->dev[DB_ALNTEXT_OUT], c.text.size() + 16, dout));
            a.text = dout;
          }
          d_text = a.text;
        } else {
          a.rows0 = job->rows0; a.rows1 = job->rows1; a.names = job->names;
          a.text = out->text;
        }
        int rc;
        if (ctx->timing && (rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, moved))) return rc;
        const dim3 block(64 * kAlnWaves), tgrid((a.ntiles + kAlnWaves - 1) / kAlnWaves), sgrid((m + kAlnWaves - 1) / kAlnWaves);
        if (a.ncoltiles) {
          hipLaunchKernelGGL(alntext_letters_kernel, dim3((a.ncoltiles + kAlnWaves - 1) / kAlnWaves), block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        if (a.ntiles) {
          hipLaunchKernelGGL(alntext_count_kernel, tgrid, block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(alntext_scan_kernel, sgrid, block, 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        if (payload && a.ntiles) {
          hipLaunchKernelGGL(alntext_emit_kernel, tgrid, block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        return timing_end(ctx);
      },
      [&](uint32_t t) {
        out->status[t] = f.res[t].status;
        out->text_len[t] = f.res[t].text_len;
        if (f.res[t].status == TRACYHIP_ALNTEXT_DEFERRED) ctx->alntext_stats.alntext_deferred += 1;
        if (f.res[t].status == TRACYHIP_ALNTEXT_TOO_SMALL) ctx->alntext_stats.alntext_too_small += 1;
      },
      [&](const AlnChunk& c) {
        RunMerger<1, CopyBackRun<1>> rt{{1u}, {ctx, {d_text}, {out->text}}};
        for (uint32_t t = c.t0; t < c.t1; ++t)
          if (f.res[t].status == TRACYHIP_ALNTEXT_OK) HIP_TRY(rt.add(f.meta[t].text_off, out->text_offset[t], f.res[t].text_len));
        HIP_TRY(rt.flush());
        return TRACYHIP_OK;
      });
}

int tracyhip_render_alignments_async(tracyhip_ctx* ctx, const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out) {
  return async_twin(tracyhip_render_alignments, ctx, job, mem, out);
}

int tracyhip_reference_slices_validate(const tracyhip_slices_job* job, int mem, const uint8_t* out, const uint64_t* out_offset) {
  return validate_slices(job, mem, out, out_offset);
}

int tracyhip_reference_slices(tracyhip_ctx* ctx, const tracyhip_slices_job* job, int mem, uint8_t* out, const uint64_t* out_offset) {
  int rc = validate_slices(job, mem, out, out_offset);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const uint32_t n = job->n;
  if (n == 0) return TRACYHIP_OK;
  rc = ctx_begin(ctx);
  if (rc != TRACYHIP_OK) return rc;
  const bool host = mem == TRACYHIP_MEM_HOST;
  // host payloads: the span of the references the slices read and the span of the result travel as one copy each
  Span refs, outs;
  std::vector<SliceDesc> meta(n);
  uint64_t tiles = 0;
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t r = job->ref_index ? job->ref_index[t] : t;
    refs.add(job->refs.offset[r], job->refs.length[r]);
    outs.add(out_offset[t], job->slice_len[t]);
  }
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t r = job->ref_index ? job->ref_index[t] : t;
    SliceDesc& d = meta[t];
    d = SliceDesc{};
    d.ref_off = job->refs.offset[r] - (host ? refs.lo : 0);
    d.out_off = out_offset[t] - (host ? outs.lo : 0);
    d.ref_len = job->refs.length[r]; d.begin = job->slice_begin[t]; d.len = job->slice_len[t];
    d.tile_first = (uint32_t)tiles;
    d.forward = job->forward[t] ? 1u : 0u;
    tiles += slice_tiles(d.len);
  }
  if (tiles >= (1ull << 31)) return set_error(TRACYHIP_ERR_RANGE, "tracyhip_reference_slices: more than 2^31 tiles of output");
  if (tiles == 0) return TRACYHIP_OK;
  SliceDesc* d_meta; HIP_TRY(ensure_into(ctx->dev[DB_ALNTEXT_DESC], (size_t)n, d_meta));
  HIP_TRY(hipMemcpyAsync(d_meta, meta.data(), sizeof(SliceDesc) * n, hipMemcpyHostToDevice, ctx->stream));
  SliceArgs a{};
  a.sl = d_meta; a.n = n; a.ntiles = (uint32_t)tiles;
  const void* d_refs = nullptr;
  void* d_out = nullptr;
  if ((rc = stage_in(ctx, ctx->dev[DB_ALNTEXT_IN], static_cast<const uint8_t*>(job->refs.data) + (host ? refs.lo : 0), host ? refs.size() : 0, mem, &d_refs))) return rc;
  if ((rc = stage_out(ctx, ctx->dev[DB_ALNTEXT_OUT], out + (host ? outs.lo : 0), host ? outs.size() : 0, mem, false, &d_out))) return rc;
  a.refs = static_cast<const uint8_t*>(d_refs);
  a.out = static_cast<uint8_t*>(d_out);
  hipLaunchKernelGGL(slice_kernel, dim3((a.ntiles + kAlnWaves - 1) / kAlnWaves), dim3(64 * kAlnWaves), 0, ctx->stream, a);
  HIP_TRY(hipGetLastError());
  if (!host) {
    HIP_TRY(ctx_sync(ctx));  // (the descriptors are this call's own: the upload has left them before it returns)
    return TRACYHIP_OK;
  }
  // exactly the bytes of the slices go back: a result buffer may hold other things between them
  RunMerger<1, CopyBackRun<1>> rt{{1u}, {ctx, {a.out}, {out}}};
  for (uint32_t t = 0; t < n; ++t) HIP_TRY(rt.add(meta[t].out_off, out_offset[t], meta[t].len));
  HIP_TRY(rt.flush());
  HIP_TRY(ctx_sync(ctx));
  return TRACYHIP_OK;
}

int tracyhip_reference_slices_async(tracyhip_ctx* ctx, const tracyhip_slices_job* job, int mem, uint8_t* out, const uint64_t* out_offset) {
  if (!ctx || !job) return set_error(TRACYHIP_ERR_ARG, "null context / job");
  const tracyhip_slices_job j = *job;
  return async_submit(ctx, [=]() { return tracyhip_reference_slices(ctx, &j, mem, out, out_offset); });
}

}  // extern "C"
