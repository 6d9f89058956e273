// dcptext.hip -- tracyhip_render_decompositions: the text `tracy decompose` prints from the decompose results themselves (the .decomp
// table of writeDecomposition decompose.h:622-632, the report tail of traceAlleleAlignJsonOut json.h:327-381, the record lines of the
// VCF) composed on the device, equal byte for byte to tracy_amd/host for every trace it answers, the rest DEFERRED to the host.
//
// The launches are render.hip's three -- one wave per tile counts its bytes, one wave per trace scans its tiles (offsets, text_len,
// status), one wave per tile writes its items at their exact offsets.  Four waves per workgroup; the bodies are dcptext_wave.h's
// (compiled for the host wave by tests/emu/emu_dcptext.cpp), the wave dev_wave.h's.  What is refused before a device is touched, the
// bound, the cut into chunks and the descriptors are dcptext_plan.h's; the frame -- chunk loop, descriptor and result buffer, waits -- is
// two_pass.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "dcptext_plan.h"
#include "dcptext_wave.h"
#include "dev_wave.h"
#include "two_pass.h"

using namespace tracyhip;

static_assert(TRACYHIP_DCPTEXT_OK == kDcpStatusOk && TRACYHIP_DCPTEXT_DEFERRED == kDcpStatusDeferred && TRACYHIP_DCPTEXT_TOO_SMALL == kDcpStatusTooSmall,
              "status codes");
static_assert(TRACYHIP_DCPTEXT_DECOMP == kDcpDecomp && TRACYHIP_DCPTEXT_JSON == kDcpJson && TRACYHIP_DCPTEXT_VCF == kDcpVcf, "forms");

namespace {

constexpr uint32_t kDcpWaves = 4;  // waves per workgroup

using DcpWave = DevWaveOps<false>;  // (the bodies share nothing but what the wave's own shuffles carry)

__global__ __launch_bounds__(64 * kDcpWaves) void dcptext_count_kernel(DcpArgs a) {
  const uint32_t tile = blockIdx.x * kDcpWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;  // (the whole wave)
  DcpWave w;
  dcptext_count_body(w, a, tile);
}

__global__ __launch_bounds__(64 * kDcpWaves) void dcptext_scan_kernel(DcpArgs a) {
  const uint32_t t = blockIdx.x * kDcpWaves + (threadIdx.x >> 6);
  if (t >= a.n) return;
  DcpWave w;
  dcptext_scan_body(w, a, t);
}

__global__ __launch_bounds__(64 * kDcpWaves) void dcptext_emit_kernel(DcpArgs a) {
  const uint32_t tile = blockIdx.x * kDcpWaves + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  DcpWave w;
  dcptext_emit_body(w, a, tile);
}

int validate(const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out) {
  bool range = false;
  uint32_t bad = 0;
  const char* why = dcptext_validate(job, mem, out, &range, &bad);
  if (!why) return TRACYHIP_OK;
  return range ? set_error(TRACYHIP_ERR_RANGE, "tracyhip_render_decompositions: %s (trace %u)", why, bad)
               : set_error(TRACYHIP_ERR_ARG, "tracyhip_render_decompositions: %s", why);
}

}  // namespace

extern "C" {

int tracyhip_render_decompositions_validate(const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out) {
  return validate(job, mem, out);
}

uint64_t tracyhip_render_decompositions_bound(uint32_t form, const tracyhip_dcptext_shape* shape) {
  return shape ? dcptext_bound(form, *shape) : 0;
}

int tracyhip_last_dcptext_stats(tracyhip_ctx* ctx, tracyhip_dcptext_stats* out) { return last_stats(ctx, &tracyhip_ctx::dcptext_stats, out); }

int tracyhip_render_decompositions(tracyhip_ctx* ctx, const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out) {
  int rc = validate(job, mem, out);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const bool host = mem == TRACYHIP_MEM_HOST, payload = out->text != nullptr;
  const bool table = dcptext_reads_table(job->form), calls = dcptext_reads_calls(job->form), json = job->form == TRACYHIP_DCPTEXT_JSON;
  TwoPass<DcpDesc, DcpOut, DcpChunk> f{ctx, job->n, host};
  rc = f.begin("tracyhip_render_decompositions", "trace", DB_DCPTEXT_DESC, &tracyhip_ctx::dcptext_stats, &tracyhip_dcptext_stats::dcptext_chunks,
               [&](uint64_t limit, std::vector<DcpChunk>& chunks, uint32_t* bad_t) { return dcptext_cut_chunks(job, out, host, limit, chunks, bad_t); });
  if (rc != TRACYHIP_OK || f.chunks.empty()) return rc;
  uint64_t max_tiles = 1;  // sized once for the largest chunk: the launches of a device call follow each other without a wait
  for (const DcpChunk& c : f.chunks) max_tiles = std::max(max_tiles, c.tiles);
  uint32_t* d_tiles; HIP_TRY(ensure_into(ctx->dev[DB_DCPTEXT_TILES], 2 * max_tiles, d_tiles));
  const uint8_t* d_text = nullptr;  // the staged text of a host chunk
  return f.run(
      payload,
      [&](const DcpChunk& c) {
        const uint32_t m = c.t1 - c.t0;
        uint32_t tile_first = 0;
        uint64_t moved = 0;
        for (uint32_t t = c.t0; t < c.t1; ++t) {
          f.meta[t] = dcptext_desc(job, out, c, host, t, tile_first);
          tile_first += dcptext_tiles(job, t);
          if (json) moved += 2ull * ((uint64_t)job->cols[0][t] + job->cols[1][t] + job->cols[2][t]) * (payload ? 2 : 0);  // (rows in, text out)
          if (table) moved += 8ull * job->dcp_rows[t] * (payload ? 2 : 1);
        }
        HIP_TRY(f.upload(c));
        DcpArgs a{};
        a.tr = f.desc_ptr(c);
        a.out = f.out_ptr(c);
        a.n = m; a.ntiles = tile_first; a.form = job->form;
        a.qual_cut = job->qual_cut; a.max_variants = calls ? job->max_variants : 1u; a.max_text = calls ? job->max_text : 2u;
        a.tile_bytes = d_tiles; a.tile_aux = d_tiles + max_tiles;
        if (host) {
          // inputs: the elements of each span, first element at the part's start; the variants of the places the chunk's traces lie at, first place first
          const uint64_t nrec = c.var.size() * job->max_variants, ntext = c.var.size() * job->max_text, nvn = c.var.size();  // (no place without calls)
          Layout li;
          const uint64_t i_di = li.add(4 * c.dcp.size()), i_de = li.add(4 * c.dcp.size());
          uint64_t i_r0[3], i_r1[3];
          for (int k = 0; k < 3; ++k) { i_r0[k] = li.add(c.rows[k].size()); i_r1[k] = li.add(c.rows[k].size()); }
          const uint64_t i_bp = li.add(4 * c.bc.size()), i_bq = li.add(c.bc.size());
          const uint64_t i_var = li.add(sizeof(tracyhip_variant) * nrec), i_vt = li.add(ntext), i_vn = li.add(4 * nvn), i_nm = li.add(c.names.size());
          uint8_t* din; HIP_TRY(ensure_into(ctx->dev[DB_DCPTEXT_IN], li.total(), din));
          auto up = [&](uint64_t at, const void* src, uint64_t bytes) {
            return bytes ? hipMemcpyAsync(din + at, src, bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
          };
          if (table) {
            HIP_TRY(up(i_di, job->dcp_indel + c.dcp.lo, 4 * c.dcp.size()));
            HIP_TRY(up(i_de, job->dcp_err + c.dcp.lo, 4 * c.dcp.size()));
          }
          for (int k = 0; json && k < 3; ++k) {
            HIP_TRY(up(i_r0[k], job->rows0[k] + c.rows[k].lo, c.rows[k].size()));
            HIP_TRY(up(i_r1[k], job->rows1[k] + c.rows[k].lo, c.rows[k].size()));
          }
          if (calls) {
            HIP_TRY(up(i_bp, job->bcpos + c.bc.lo, 4 * c.bc.size()));
            HIP_TRY(up(i_bq, job->estqual + c.bc.lo, c.bc.size()));
            HIP_TRY(up(i_var, job->var + c.var.lo * job->max_variants, sizeof(tracyhip_variant) * nrec));
            HIP_TRY(up(i_vt, job->var_text + c.var.lo * job->max_text, ntext));
            HIP_TRY(up(i_vn, job->var_n + c.var.lo, 4 * nvn));
            HIP_TRY(up(i_nm, job->names + c.names.lo, c.names.size()));
          }
          a.dcp_indel = reinterpret_cast<const int32_t*>(din + i_di); a.dcp_err = reinterpret_cast<const int32_t*>(din + i_de);
          for (int k = 0; k < 3; ++k) { a.rows0[k] = din + i_r0[k]; a.rows1[k] = din + i_r1[k]; }
          a.bcpos = reinterpret_cast<const int32_t*>(din + i_bp); a.estqual = din + i_bq;
          a.var = reinterpret_cast<const tracyhip_variant*>(din + i_var); a.var_text = din + i_vt;
          a.var_n = reinterpret_cast<const uint32_t*>(din + i_vn); a.names = din + i_nm;
          if (payload) {
            uint8_t* dout; HIP_TRY(ensure_into(ctx->dev[DB_DCPTEXT_OUT], c.text.size() + 16, dout));
            a.text = dout;
          }
          d_text = a.text;
        } else {
          a.dcp_indel = job->dcp_indel; a.dcp_err = job->dcp_err;
          for (int k = 0; k < 3; ++k) { a.rows0[k] = job->rows0[k]; a.rows1[k] = job->rows1[k]; }
          a.bcpos = job->bcpos; a.estqual = job->estqual;
          a.var = job->var; a.var_text = job->var_text; a.var_n = job->var_n; a.names = job->names;
          a.text = out->text;
        }
        int rc;
        if (ctx->timing && (rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, moved))) return rc;
        const dim3 block(64 * kDcpWaves), tgrid((a.ntiles + kDcpWaves - 1) / kDcpWaves), sgrid((m + kDcpWaves - 1) / kDcpWaves);
        if (a.ntiles) {
          hipLaunchKernelGGL(dcptext_count_kernel, tgrid, block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(dcptext_scan_kernel, sgrid, block, 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        if (payload && a.ntiles) {
          hipLaunchKernelGGL(dcptext_emit_kernel, tgrid, block, 0, ctx->stream, a);
          HIP_TRY(hipGetLastError());
        }
        return timing_end(ctx);
      },
      [&](uint32_t t) {
        out->status[t] = f.res[t].status;
        out->text_len[t] = f.res[t].text_len;
        if (f.res[t].status == TRACYHIP_DCPTEXT_DEFERRED) ctx->dcptext_stats.dcptext_deferred += 1;
        if (f.res[t].status == TRACYHIP_DCPTEXT_TOO_SMALL) ctx->dcptext_stats.dcptext_too_small += 1;
      },
      [&](const DcpChunk& c) {
        RunMerger<1, CopyBackRun<1>> rt{{1u}, {ctx, {d_text}, {out->text}}};
        for (uint32_t t = c.t0; t < c.t1; ++t)
          if (f.res[t].status == TRACYHIP_DCPTEXT_OK) HIP_TRY(rt.add(f.meta[t].text_off, out->text_offset[t], f.res[t].text_len));
        HIP_TRY(rt.flush());
        return TRACYHIP_OK;
      });
}

int tracyhip_render_decompositions_async(tracyhip_ctx* ctx, const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out) {
  return async_twin(tracyhip_render_decompositions, ctx, job, mem, out);
}

}  // extern "C"
