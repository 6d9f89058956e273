// msa_batch.hip -- the row-block kernels of `tracy assemble` (assemble_wave.h: msa_merge, msa_profile, msa_consensus) over lists of
// merges, shared by the reference-guided chain (assemble.hip: one merge per group and chain step) and the de novo tree (denovo.hip:
// one merge per tree node of a height).  Each call keeps its own plan, buffers and descriptors (AsmStep / AsmFinal, capi_internal.h).
#include <hip/hip_runtime.h>

#include "capi_internal.h"

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

}  // namespace tracyhip
