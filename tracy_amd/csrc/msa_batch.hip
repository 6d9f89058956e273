// msa_batch.hip -- the row-block kernels of `tracy assemble` (assemble_wave.h: msa_merge, msa_profile, msa_consensus) over lists of
// merges, shared by the reference-guided chain (assemble.hip: one merge per group and chain step) and the de novo tree (denovo.hip:
// one merge per tree node of a height), and the host code both calls run around them: the view of their common result fields
// (GroupOut: trace-less calls, payload staging, the final copy-back), one batch of traceback sweeps (TraceBatch), one batch of merges
// up to its synchronisation, msa_consensus of a chunk, the tail of the strand-score stage.  Each call keeps its own plan -- who is
// aligned with whom, in which order, in which chunks -- and its own buffers (the AB_* / DN_* roles of capi_internal.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "dev_wave.h"

using namespace tracyhip;

namespace {

// one wave per (merge, row of the merged block)
__global__ __launch_bounds__(64) void msa_merge_kernel(const AsmStep* __restrict__ steps, const uint8_t* __restrict__ ops, const uint32_t* __restrict__ ops_len) {
  const AsmStep s = steps[blockIdx.x];
  const uint32_t r = blockIdx.y;
  if (r >= s.left.n + s.right.n) return;
  const uint32_t L = ops_len[s.slot];
  if (L > s.cap) return;
  MsaDevWave w;
  const bool left = r < s.left.n;
  msa_merge_row_wave(w, ops + s.ops_off, L, left ? s.left : s.right, left ? r : r - s.left.n, left, s.dst + (uint64_t)r * L, s.span + 2 * r);
}

// one wave per (merge, 64 columns); the grid covers the longest capacity, waves past a merge's columns leave
__global__ __launch_bounds__(64) void msa_profile_kernel(const AsmStep* __restrict__ steps, const uint32_t* __restrict__ ops_len) {
  const AsmStep s = steps[blockIdx.x];
  if (!s.prof) return;
  const uint32_t L = ops_len[s.slot];
  const uint32_t b = blockIdx.y * 64u;
  if (b >= L || L > s.cap) return;
  MsaDevWave w;
  msa_profile_wave(w, s.dst, s.left.n + s.right.n, L, s.span, b, s.prof);
  const uint32_t j = b + threadIdx.x;
  if (j < L) s.colclass[j] = (uint8_t)column_class(s.prof, L, j);  // (this lane's own six stores)
}

// one wave per finished group
__global__ __launch_bounds__(64) void msa_consensus_kernel(const AsmFinal* __restrict__ fin, const uint32_t* __restrict__ ops_len) {
  const AsmFinal f = fin[blockIdx.x];
  const uint32_t L = ops_len[f.slot];
  if (L > f.cap) return;
  MsaDevWave w;
  msa_consensus_wave(w, f.rows, f.rows_used, L, f.span, f.cov_threshold, f.gapped, f.cons, f.qual, f.cons_len);
}

}  // namespace

namespace tracyhip {

hipError_t launch_msa_merge(const AsmStep* steps, uint32_t n, uint32_t max_rows, const uint8_t* ops, const uint32_t* ops_len, hipStream_t st) {
  if (n == 0 || max_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(msa_merge_kernel, dim3(n, max_rows), dim3(64), 0, st, steps, ops, ops_len);
  return hipGetLastError();
}

hipError_t launch_msa_profile(const AsmStep* steps, uint32_t n, uint64_t max_cap, const uint32_t* ops_len, hipStream_t st) {
  if (n == 0 || max_cap == 0) return hipSuccess;
  hipLaunchKernelGGL(msa_profile_kernel, dim3(n, (uint32_t)((max_cap + 63) / 64)), dim3(64), 0, st, steps, ops_len);
  return hipGetLastError();
}

hipError_t launch_msa_consensus(const AsmFinal* fin, uint32_t n, const uint32_t* ops_len, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(msa_consensus_kernel, dim3(n), dim3(64), 0, st, fin, ops_len);
  return hipGetLastError();
}

// ---- group batches: the host code around the kernels ----

int GroupOut::clear_counts(tracyhip_ctx* ctx, int mem) const {
  for (uint32_t* p : {nrows, ncol, cons_len}) {
    if (mem == TRACYHIP_MEM_HOST) std::memset(p, 0, 4 * (size_t)ng);
    else HIP_TRY(hipMemsetAsync(p, 0, 4 * (size_t)ng, ctx->stream));
  }
  if (mem != TRACYHIP_MEM_HOST) HIP_TRY(ctx_sync(ctx));
  return TRACYHIP_OK;
}

int GroupOut::bind(tracyhip_ctx* ctx, int mem, uint64_t ext_rows, uint64_t ext_col) {
  d_rows = rows; d_gapped = gapped; d_cons = cons; d_qual = qual;
  d_clen = cons_len;
  if (mem == TRACYHIP_MEM_HOST) {
    const uint64_t er = (std::max<uint64_t>(ext_rows, 1) + 255) & ~255ull, ec = (std::max<uint64_t>(ext_col, 1) + 255) & ~255ull;
    uint8_t* q; HIP_TRY(ensure_into(ctx->dev[AB_PAY], er + 3 * ec + sizeof(uint32_t) * (size_t)ng, q));
    d_rows = q; d_gapped = q + er; d_cons = q + er + ec; d_qual = q + er + 2 * ec;
    d_clen = reinterpret_cast<uint32_t*>(q + er + 3 * ec);
  }
  HIP_TRY(hipMemsetAsync(d_clen, 0, sizeof(uint32_t) * (size_t)ng, ctx->stream));
  return TRACYHIP_OK;
}

AsmFinal GroupOut::final_entry(uint32_t g, const int32_t* span, uint32_t rows_used, uint32_t slot, uint32_t cap, float fraction_called) const {
  const int32_t cov_threshold = (int32_t)(fraction_called * (float)(size_t)rows_used);  // float x size_t, msa.h:196
  const uint64_t co = col_offset[g];
  return AsmFinal{d_rows + rows_offset[g], span, rows_used, slot, cov_threshold, cap, d_gapped + co, d_cons + co, d_qual + co, d_clen + g};
}

int put_result(tracyhip_ctx* ctx, int mem, void* user, const void* host, size_t bytes) {
  if (mem == TRACYHIP_MEM_HOST) std::memcpy(user, host, bytes);
  else HIP_TRY(hipMemcpyAsync(user, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return TRACYHIP_OK;
}

int GroupOut::copy_back(tracyhip_ctx* ctx, int mem, const uint32_t* h_nrows, const uint32_t* h_ncol) const {
  int rc;
  if ((rc = put_result(ctx, mem, nrows, h_nrows, 4 * (size_t)ng)) || (rc = put_result(ctx, mem, ncol, h_ncol, 4 * (size_t)ng))) return rc;
  if (mem != TRACYHIP_MEM_HOST) return TRACYHIP_OK;  // (the kernels wrote the caller's payload arrays)
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemcpyAsync(cons_len, d_clen, 4 * (size_t)ng, hipMemcpyDeviceToHost, st));
  for (uint32_t g = 0; g < ng; ++g) {  // only what the group wrote (the columns past cons_len hold no result)
    if (!h_nrows[g]) continue;
    const uint64_t ro = rows_offset[g], co = col_offset[g];
    HIP_TRY(hipMemcpyAsync(rows + ro, d_rows + ro, (uint64_t)h_nrows[g] * h_ncol[g], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(gapped + co, d_gapped + co, h_ncol[g], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cons + co, d_cons + co, h_ncol[g], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(qual + co, d_qual + co, h_ncol[g], hipMemcpyDeviceToHost, st));
  }
  return TRACYHIP_OK;
}

PairDesc prof_pair_desc(uint64_t a1_off, uint32_t m, uint64_t a2_off, uint32_t n, bool row4_zero) {
  PairDesc d{};
  d.a1_off = a1_off;
  d.a2_off = a2_off;
  d.m = m; d.n = n;
  d.a1_stride = m; d.a2_stride = n;
  d.flags = row4_zero ? PAIR_ROW4_ZERO : 0u;
  return d;
}

void TraceBatch::add(uint64_t a1_off, uint32_t m, uint64_t a2_off, uint32_t n, bool row4_zero, int K, uint32_t out) {
  const uint32_t P = num_passes(m, K);
  PairDesc d = prof_pair_desc(a1_off, m, a2_off, n, row4_zero);
  d.bits_off = words;
  d.scratch_off = scr;
  d.out = out;
  hd[k.size()] = d;
  k.push_back(K);
  words += (uint64_t)P * steps_per_pass(n) * 64;
  if (P > 1) scr += (uint64_t)n + 2;
}

int TraceBatch::upload(tracyhip_ctx* ctx, DpArgs& a) const {
  const uint64_t need = words * 8 + scr * 8;
  if (need > limit)
    return set_error(TRACYHIP_ERR_OOM, "a batch of tracebacks needs %llu bytes of planes, workspace limit is %llu", (unsigned long long)need,
                     (unsigned long long)limit);
  HIP_TRY(ctx->dev[DB_BITS].ensure(std::max<uint64_t>(words * 8, 8)));
  if (scr) HIP_TRY(ctx->dev[DB_SCRATCH].ensure(scr * 8));
  a.bits = static_cast<uint64_t*>(ctx->dev[DB_BITS].p);
  a.bits32 = static_cast<uint32_t*>(ctx->dev[DB_BITS].p);
  a.scratch = static_cast<int32_t*>(ctx->dev[DB_SCRATCH].p);
  HIP_TRY(hipMemcpyAsync(dd, hd, sizeof(PairDesc) * k.size(), hipMemcpyHostToDevice, ctx->stream));
  return TRACYHIP_OK;
}

int msa_merge_batch(tracyhip_ctx* ctx, DpArgs& a, const TraceBatch& tb, const AsmStep* h_step, AsmStep* d_step, uint32_t* h_len, uint32_t lo,
                    uint32_t hi) {
  const uint32_t n = (uint32_t)tb.k.size();
  hipStream_t st = ctx->stream;
  uint32_t max_rows = 0;
  uint64_t max_cap = 0;
  bool any_prof = false;
  for (uint32_t j = 0; j < n; ++j) {
    max_rows = std::max(max_rows, h_step[j].left.n + h_step[j].right.n);
    max_cap = std::max<uint64_t>(max_cap, h_step[j].cap);
    any_prof |= h_step[j].prof != nullptr;
  }
  int rc;
  if ((rc = tb.upload(ctx, a))) return rc;
  HIP_TRY(hipMemcpyAsync(d_step, h_step, sizeof(AsmStep) * n, hipMemcpyHostToDevice, st));
  if ((rc = prof_trace_runs(ctx, a, tb.hd, tb.dd, tb.k.data(), 0, n, tb.ops, tb.ops_off, tb.ops_len))) return rc;
  if ((rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return rc;
  HIP_TRY(launch_msa_merge(d_step, n, max_rows, tb.ops, tb.ops_len, st));
  if (any_prof) HIP_TRY(launch_msa_profile(d_step, n, max_cap, tb.ops_len, st));
  if ((rc = timing_end(ctx))) return rc;
  // the op counts: the columns of what the next batch aligns against
  HIP_TRY(hipMemcpyAsync(h_len + lo, tb.ops_len + lo, sizeof(uint32_t) * (hi - lo), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx_sync(ctx));
  return TRACYHIP_OK;
}

int msa_consensus_batch(tracyhip_ctx* ctx, const AsmFinal* h_fin, AsmFinal* d_fin, uint32_t nf, const uint32_t* ops_len) {
  if (nf == 0) return TRACYHIP_OK;
  HIP_TRY(hipMemcpyAsync(d_fin, h_fin, sizeof(AsmFinal) * nf, hipMemcpyHostToDevice, ctx->stream));
  int rc;
  if ((rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return rc;
  HIP_TRY(launch_msa_consensus(d_fin, nf, ops_len, ctx->stream));
  return timing_end(ctx);
}

int prof_score_stage(tracyhip_ctx* ctx, const tracyhip_params* prm, bool wide, DpArgs& a, const PairDesc* hd, const PairDesc* dd, const int* k,
                     uint32_t nu, int32_t* h_scores, size_t nscores, uint64_t max_mn, std::vector<std::pair<uint32_t, int>>& narrow_launches) {
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx->dev[DB_ERR].ensure(kErrBytes));
  a.err = static_cast<int32_t*>(ctx->dev[DB_ERR].p);  // (a context's first call: the words did not exist when the caller built `a`)
  HIP_TRY(hipMemsetAsync(a.err, 0, sizeof(int32_t) * kErrWords, st));
  int rc;
  if ((rc = prof_score_runs(ctx, prm, wide, a, hd, dd, k, 0, nu, narrow_launches))) return rc;
  int32_t herr[kErrWords] = {};
  if (nscores) HIP_TRY(hipMemcpyAsync(h_scores, a.scores, sizeof(int32_t) * nscores, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(herr, a.err, sizeof(herr), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx_sync(ctx));
  return range_verdict(prm, herr, narrow_launches, max_mn, kTagShift);
}

}  // namespace tracyhip
