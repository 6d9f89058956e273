// prof_batch.hip -- what the profile x profile batches share: tracyhip_gotoh_score / align over two profile sets (capi.hip
// build_problem), tracyhip_consensus_traces (consensus.hip) and tracyhip_assemble_traces (assemble.hip).
//
// Device side: the reverse complement of a list of profiles and their classes (row 4 all zero -> the 16-term score body; the class of
// every column for the screened substitution scores).  Host side: the launch loop of the two batch calls -- one launch per run of
// equal strip height and term count over a sorted descriptor list, as a score form and a traceback form.  Each call keeps its own
// chunk plan, buffers and result staging; run_dp keeps its own loop (five stages, four modes).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "capi_internal.h"
#include "launch.h"

using namespace tracyhip;

namespace {

// revcomp of every profile of the list (orc_revcomp_profile / profile.h:74-90): rows A<->T, C<->G swapped, N and gap kept, columns
// reversed; profile s is written at rev_base + its own offset.  One workgroup per profile.
__global__ __launch_bounds__(256) void prof_revcomp_kernel(const ProfSeq* __restrict__ seqs, const float* __restrict__ in, float* __restrict__ out,
                                                           uint64_t rev_base) {
  const ProfSeq s = seqs[blockIdx.x];
  const float* p = in + s.off;
  float* q = out + rev_base + s.off;
  const uint64_t n = s.len;
  for (uint32_t j = threadIdx.x; j < s.len; j += blockDim.x) {
    const uint64_t src = n - 1 - j;
    q[0 * n + j] = p[3 * n + src];
    q[1 * n + j] = p[2 * n + src];
    q[2 * n + j] = p[1 * n + src];
    q[3 * n + j] = p[0 * n + src];
    q[4 * n + j] = p[4 * n + src];
    q[5 * n + j] = p[5 * n + src];
  }
}

// is row 4 ('N') zero over a whole profile?  (NaN counts as non-zero.)  colclass (or null): the class of every column
// (dp_kernels.h column_class), stored at the index of the column's row-0 element.  One wave per profile.
__global__ __launch_bounds__(64) void prof_classify_kernel(const ProfSeq* __restrict__ seqs, const float* __restrict__ data, uint8_t* __restrict__ zero,
                                                           uint8_t* __restrict__ colclass) {
  const ProfSeq s = seqs[blockIdx.x];
  bool nz = false;
  for (uint32_t j = threadIdx.x; j < s.len; j += 64) {
    nz |= !(data[s.off + 4ull * s.len + j] == 0.0f);
    if (colclass) colclass[s.off + j] = (uint8_t)column_class(data + s.off, s.len, j);
  }
  const unsigned long long any = __ballot(nz);
  if (threadIdx.x == 0) zero[blockIdx.x] = any ? 0 : 1;
}

// end of the run that starts at unit j: the units up to `hi` of j's strip height and term count
uint32_t run_end(const PairDesc* hd, uint32_t per, const int* k, uint32_t j, uint32_t hi) {
  const uint32_t r4 = hd[(size_t)per * j].flags & PAIR_ROW4_ZERO;
  uint32_t e = j;
  while (e < hi && k[e] == k[j] && (hd[(size_t)per * e].flags & PAIR_ROW4_ZERO) == r4) ++e;
  return e;
}

}  // namespace

namespace tracyhip {

hipError_t launch_prof_revcomp(const ProfSeq* seqs, uint32_t n, const float* in, float* out, uint64_t rev_base, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(prof_revcomp_kernel, dim3(n), dim3(256), 0, st, seqs, in, out, rev_base);
  return hipGetLastError();
}

hipError_t launch_prof_classify(const ProfSeq* seqs, uint32_t n, const float* data, uint8_t* zero, uint8_t* colclass, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(prof_classify_kernel, dim3(n), dim3(64), 0, st, seqs, data, zero, colclass);
  return hipGetLastError();
}

int prof_score_runs(tracyhip_ctx* ctx, const tracyhip_params* prm, bool wide, const DpArgs& args, const PairDesc* hd, const PairDesc* dd,
                    const int* k, uint32_t lo, uint32_t hi, std::vector<std::pair<uint32_t, int>>& narrow_launches, uint32_t per) {
  DpArgs a = args;
  a.walk_ops = nullptr; a.walk_ops_off = nullptr; a.walk_ops_len = nullptr;
  int trc;
  for (uint32_t j = lo; j < hi;) {
    const uint32_t e = run_end(hd, per, k, j, hi);
    uint64_t mn = 0, cells = 0;
    for (uint32_t u = j; u < e; ++u) {
      const PairDesc& d = hd[per * (size_t)u];
      mn = std::max<uint64_t>(mn, (uint64_t)d.m + d.n);
      cells += (uint64_t)per * d.m * d.n;
    }
    const bool a16 = !wide && !ctx->knobs.no_narrow && arith16_ok(prm, mn, 0);
    if (a16) narrow_launches.emplace_back((uint32_t)mn, 0);
    a.pairs = dd + per * (size_t)j;
    if ((trc = timing_begin(ctx, TRACYHIP_TIMER_SCORE, cells, 0))) return trc;
    HIP_TRY(launch_gotoh_prof(k[j], false, (hd[per * (size_t)j].flags & PAIR_ROW4_ZERO) != 0, a16, a, per * (e - j), ctx->stream));
    if ((trc = timing_end(ctx))) return trc;
    j = e;
  }
  return TRACYHIP_OK;
}

int prof_trace_runs(tracyhip_ctx* ctx, const DpArgs& args, const PairDesc* hd, const PairDesc* dd, const int* k, uint32_t lo, uint32_t hi,
                    uint8_t* ops, const uint64_t* ops_off, uint32_t* ops_len) {
  DpArgs a = args;
  const bool fused_walk = !ctx->knobs.no_fused_walk;
  if (fused_walk) { a.walk_ops = ops; a.walk_ops_off = ops_off; a.walk_ops_len = ops_len; }
  int trc;
  for (uint32_t j = lo; j < hi;) {
    const uint32_t e = run_end(hd, 1, k, j, hi);
    uint64_t cells = 0;
    for (uint32_t u = j; u < e; ++u) cells += (uint64_t)hd[u].m * hd[u].n;
    a.pairs = dd + j;
    if ((trc = timing_begin(ctx, TRACYHIP_TIMER_TRACE, cells, cells / 2))) return trc;
    HIP_TRY(launch_gotoh_prof(k[j], true, (hd[j].flags & PAIR_ROW4_ZERO) != 0, false, a, e - j, ctx->stream));
    if ((trc = timing_end(ctx))) return trc;
    if (!fused_walk) {
      WalkArgs wa{};
      wa.pairs = dd + j; wa.bits = a.bits; wa.ops = ops; wa.ops_off = ops_off; wa.ops_len = ops_len; wa.err = a.err; wa.npairs = e - j; wa.K = k[j];
      if ((trc = timing_begin(ctx, TRACYHIP_TIMER_WALK, 0, 0))) return trc;
      HIP_TRY(launch_gotoh_walk(wa, ctx->stream));
      if ((trc = timing_end(ctx))) return trc;
    }
    j = e;
  }
  return TRACYHIP_OK;
}

}  // namespace tracyhip
