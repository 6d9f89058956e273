// variants.hip -- the variant calling of `tracy decompose -v` on the device (indigo.h:397-443 over variants.h:34-126):
//   tracyhip_call_variants       the stage: callVariants of both allele alignments of every trace, insertVariant, the sort, variantCallIndex
//   tracyhip_decompose_variants  the section for a batch: from the results of tracyhip_decompose_traces to the variant lists
//
// One wave per trace runs variants_wave.h; its two per-allele event lists live in a slice of VB_EVENTS that belongs to the
// workgroup, which takes traces blockIdx.x, + gridDim.x, ...  The pipeline is planned by the host from one read of the decompose
// results: forward traces get the rows of their two allele alignments from the existing alignment_rows kernel, straight from the
// job's payloads; reverse traces get reverse complements of allele and slice (var_revcomp_kernel), one traceback batch through
// build_problem + run_dp, what tracyhip_gotoh_align runs -- the exact path, bit-identical with the oracle's gotoh -- and rows from its op strings.  A host caller
// receives the used records and text only: they are packed on the device (var_pack_*), copied, and put in place by the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "dev_wave.h"
#include "launch.h"
#include "pipe_internal.h"
#include "variants_wave.h"

using namespace tracyhip;

namespace {

constexpr uint32_t kVarMaxVariants = 1024;
// (tests/test_gpu_batch_rounds.py builds its batch sizes on 2048 and reads it from this line)
constexpr uint32_t kVarWaves = 2048;  // resident workgroups of variants_kernel: eight per CU, each with its two event lists in VB_EVENTS

struct VarDevWave : DevWaveOps<true> {  // the wave of variants_wave.h: one workgroup of 64 threads
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

struct VarAln {  // one two-row alignment
  const uint8_t* row0;
  const uint8_t* row1;
  const uint32_t* len;  // its column count, on the device
  int32_t pos;          // rs.pos
  uint32_t pad;
};
struct VarDesc {  // one trace
  VarAln a[2];
  uint32_t forward, bc_len;
  uint32_t skip;  // no variants are called (status != 0): var_n 0, flags 0
  uint32_t out;   // its index in the result arrays
  uint32_t trim_left, trim_right;  // the trace's own pair (variantCallIndex; a scalar call writes its pair into every record)
};
struct VarArgs {
  const VarDesc* desc;
  uint32_t n, max_variants, max_text;
  VarEvent* ev;
  tracyhip_variant* var;
  uint8_t* text;
  uint32_t* var_n;
  uint32_t* var_flags;
};

__global__ __launch_bounds__(64) void variants_kernel(VarArgs a) {
  VarDevWave w;
  VarEvent* ev = a.ev + (size_t)blockIdx.x * 2u * a.max_variants;
  for (uint32_t i = blockIdx.x; i < a.n; i += gridDim.x) {
    const VarDesc d = a.desc[i];
    if (d.skip) {
      if (threadIdx.x == 0) { a.var_n[d.out] = 0; a.var_flags[d.out] = 0; }
      continue;
    }
    VarTrace t;
    for (int k = 0; k < 2; ++k) {
      t.row0[k] = d.a[k].row0; t.row1[k] = d.a[k].row1; t.len[k] = *d.a[k].len; t.pos0[k] = d.a[k].pos;
    }
    t.forward = d.forward; t.bc_len = d.bc_len;
    variants_wave(w, t, d.trim_left, d.trim_right, a.max_variants, a.max_text, ev, a.var + (size_t)d.out * a.max_variants,
                  a.text + (size_t)d.out * a.max_text, a.var_n + d.out, a.var_flags + d.out);
  }
}

// reverseComplement (the reference's table: ACGTN in either case -> upper-case complement; any other letter leaves the byte of the
// OUTPUT position as it was) of bytes [begin, begin + len) of a sequence -- of its reverse complement when flip is set (a reference
// the decompose call oriented itself)
struct VarRcDesc {
  const uint8_t* src;
  uint64_t dst;
  uint32_t src_len, begin, len, flip;
};
__device__ __forceinline__ uint8_t var_rc_letter(uint8_t c) {
  switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    case 'N': case 'n': return 'N';
    default: return 0;
  }
}
__global__ __launch_bounds__(256) void var_revcomp_kernel(const VarRcDesc* __restrict__ desc, uint8_t* __restrict__ out) {
  const VarRcDesc d = desc[blockIdx.x];
  auto view = [&](uint32_t i) -> uint8_t {
    const uint32_t p = d.begin + i;
    if (!d.flip) return d.src[p];
    const uint8_t c = var_rc_letter(d.src[d.src_len - 1u - p]);
    return c ? c : d.src[p];
  };
  for (uint32_t i = threadIdx.x; i < d.len; i += 256) {
    const uint8_t c = var_rc_letter(view(d.len - 1u - i));
    out[d.dst + i] = c ? c : view(i);
  }
}

// where every trace's used records / text bytes begin when they are packed back to back: off[0 .. nt] records, off[nt + 1 .. 2 nt + 1]
// bytes (the last of each: the totals).  One workgroup; a thread sums a contiguous stretch of traces.
// (tests/test_gpu_batch_rounds.py builds its batch sizes on the 1024 threads and reads them from the next line)
__global__ __launch_bounds__(1024) void var_pack_scan_kernel(const uint32_t* __restrict__ var_n, const tracyhip_variant* __restrict__ var, uint32_t max_variants,
                                                             uint32_t nt, uint64_t* __restrict__ off) {
  __shared__ uint64_t srec[1024], stext[1024];
  const uint32_t per = (nt + 1023u) / 1024u;
  const uint32_t lo = min(nt, threadIdx.x * per), hi = min(nt, lo + per);
  auto text_used = [&](uint32_t t, uint32_t n) -> uint64_t {  // (the text is packed in record order: the last record ends it)
    if (!n) return 0;
    const tracyhip_variant& v = var[(size_t)t * max_variants + n - 1u];
    return (uint64_t)v.alt_off + v.alt_len;
  };
  uint64_t r = 0, x = 0;
  for (uint32_t t = lo; t < hi; ++t) { const uint32_t n = var_n[t]; r += n; x += text_used(t, n); }
  srec[threadIdx.x] = r; stext[threadIdx.x] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t ar = 0, ax = 0;
    for (uint32_t i = 0; i < 1024; ++i) {
      const uint64_t pr = srec[i], px = stext[i];
      srec[i] = ar; stext[i] = ax;
      ar += pr; ax += px;
    }
    off[nt] = ar; off[2 * (size_t)nt + 1] = ax;
  }
  __syncthreads();
  r = srec[threadIdx.x]; x = stext[threadIdx.x];
  for (uint32_t t = lo; t < hi; ++t) {
    const uint32_t n = var_n[t];
    off[t] = r; off[(size_t)nt + 1 + t] = x;
    r += n; x += text_used(t, n);
  }
}
__global__ __launch_bounds__(64) void var_pack_copy_kernel(const uint32_t* __restrict__ var_n, const tracyhip_variant* __restrict__ var, const uint8_t* __restrict__ text,
                                                           uint32_t max_variants, uint32_t max_text, uint32_t nt, const uint64_t* __restrict__ off,
                                                           tracyhip_variant* __restrict__ prec, uint8_t* __restrict__ ptext) {
  const uint32_t t = blockIdx.x;
  const uint32_t n = var_n[t];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(var + (size_t)t * max_variants);
  uint32_t* dst = reinterpret_cast<uint32_t*>(prec + off[t]);
  for (uint32_t i = threadIdx.x; i < 8u * n; i += 64) dst[i] = src[i];
  const uint64_t x0 = off[(size_t)nt + 1 + t], x1 = off[(size_t)nt + 2 + t];
  for (uint64_t i = threadIdx.x; i < x1 - x0; i += 64) ptext[x0 + i] = text[(size_t)t * max_text + i];
}

bool var_caps_ok(uint32_t max_variants, uint32_t max_text) {
  if (max_variants < 1 || max_variants > kVarMaxVariants)
    return set_error(TRACYHIP_ERR_RANGE, "max_variants must be in [1, %u] (got %u)", kVarMaxVariants, max_variants), false;
  if (max_text < 2) return set_error(TRACYHIP_ERR_RANGE, "max_text must hold one variant at least (2 bytes; got %u)", max_text), false;
  return true;
}

// the four result arrays on the device: the caller's (MEM_DEVICE) or the context's staging copies
struct VarOut {
  tracyhip_variant* var = nullptr;
  uint8_t* text = nullptr;
  uint32_t* n = nullptr;
  uint32_t* flags = nullptr;
};
int var_out_begin(tracyhip_ctx* ctx, uint32_t nt, const tracyhip_variants_result& r, int mem, VarOut& o) {
  if (mem == TRACYHIP_MEM_DEVICE) { o.var = r.var; o.text = r.text; o.n = r.var_n; o.flags = r.var_flags; return TRACYHIP_OK; }
  HIP_TRY(ensure_into(ctx->dev[VB_OUT_REC], (size_t)nt * r.max_variants, o.var));
  HIP_TRY(ensure_into(ctx->dev[VB_OUT_TEXT], (size_t)nt * r.max_text, o.text));
  HIP_TRY(ensure_into(ctx->dev[VB_OUT_N], 2 * (size_t)nt, o.n));
  o.flags = o.n + nt;
  return TRACYHIP_OK;
}
int launch_variants(tracyhip_ctx* ctx, const VarDesc* d_desc, uint32_t n, const tracyhip_variants_result& r, const VarOut& o) {
  if (n == 0) return TRACYHIP_OK;
  const uint32_t grid = std::min(n, kVarWaves);
  VarArgs a{};
  a.desc = d_desc; a.n = n; a.max_variants = r.max_variants; a.max_text = r.max_text;
  HIP_TRY(ensure_into(ctx->dev[VB_EVENTS], (size_t)kVarWaves * 2u * r.max_variants, a.ev));
  a.var = o.var; a.text = o.text; a.var_n = o.n; a.var_flags = o.flags;
  int trc;
  if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return trc;
  hipLaunchKernelGGL(variants_kernel, dim3(grid), dim3(64), 0, ctx->stream, a);
  HIP_TRY(hipGetLastError());
  return timing_end(ctx);
}
// the end of both calls: waits for the stream; a host caller's arrays receive the used records and text.  truncated: traces flagged.
int var_out_end(tracyhip_ctx* ctx, uint32_t nt, const tracyhip_variants_result& r, int mem, const VarOut& o, uint32_t* truncated) {
  hipStream_t st = ctx->stream;
  *truncated = 0;
  if (mem == TRACYHIP_MEM_DEVICE) {
    std::vector<uint32_t> fl(nt);
    HIP_TRY(hipMemcpyAsync(fl.data(), o.flags, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx_sync(ctx));
    for (uint32_t t = 0; t < nt; ++t) *truncated += fl[t] & 1u;
    return TRACYHIP_OK;
  }
  uint64_t* d_off; HIP_TRY(ensure_into(ctx->dev[VB_PACK_OFF], 2 * (size_t)nt + 2, d_off));
  hipLaunchKernelGGL(var_pack_scan_kernel, dim3(1), dim3(1024), 0, st, o.n, o.var, r.max_variants, nt, d_off);
  HIP_TRY(hipGetLastError());
  std::vector<uint64_t> off(2 * (size_t)nt + 2);
  HIP_TRY(hipMemcpyAsync(off.data(), d_off, 8 * off.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(r.var_n, o.n, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(r.var_flags, o.flags, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx_sync(ctx));
  for (uint32_t t = 0; t < nt; ++t) *truncated += r.var_flags[t] & 1u;
  const uint64_t nrec = off[nt], nbytes = off[2 * (size_t)nt + 1];
  if (nrec == 0) return TRACYHIP_OK;
  tracyhip_variant* d_prec; HIP_TRY(ensure_into(ctx->dev[VB_PACK_REC], (size_t)nrec, d_prec));
  uint8_t* d_ptext; HIP_TRY(ensure_into(ctx->dev[VB_PACK_TEXT], (size_t)nbytes, d_ptext));
  hipLaunchKernelGGL(var_pack_copy_kernel, dim3(nt), dim3(64), 0, st, o.n, o.var, o.text, r.max_variants, r.max_text, nt, d_off, d_prec, d_ptext);
  HIP_TRY(hipGetLastError());
  std::unique_ptr<tracyhip_variant[]> prec(new tracyhip_variant[nrec]);
  std::unique_ptr<uint8_t[]> ptext(new uint8_t[nbytes]);
  HIP_TRY(hipMemcpyAsync(prec.get(), d_prec, sizeof(tracyhip_variant) * (size_t)nrec, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ptext.get(), d_ptext, (size_t)nbytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx_sync(ctx));
  parallel_for(nt, [&](uint32_t lo, uint32_t hi, uint32_t) {
    for (uint32_t t = lo; t < hi; ++t) {
      if (!r.var_n[t]) continue;
      std::memcpy(r.var + (size_t)t * r.max_variants, prec.get() + off[t], sizeof(tracyhip_variant) * (size_t)r.var_n[t]);
      std::memcpy(r.text + (size_t)t * r.max_text, ptext.get() + off[(size_t)nt + 1 + t], (size_t)(off[(size_t)nt + 2 + t] - off[(size_t)nt + 1 + t]));
    }
  });
  return TRACYHIP_OK;
}

// a pointer of the caller's against the `mem` it names: device memory passed as MEM_HOST, or pageable host memory passed as MEM_DEVICE
int check_mem_kind(const void* p, int mem, const char* what) {
  hipPointerAttribute_t at{};
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) (void)hipGetLastError();  // (memory the runtime does not know: pageable host memory)
  const bool known = e == hipSuccess && at.type != hipMemoryTypeUnregistered;
  if (mem == TRACYHIP_MEM_HOST && known && at.type == hipMemoryTypeDevice)
    return set_error(TRACYHIP_ERR_ARG, "%s is device memory, the call says TRACYHIP_MEM_HOST", what);
  if (mem == TRACYHIP_MEM_DEVICE && !known) return set_error(TRACYHIP_ERR_ARG, "%s is not device memory, the call says TRACYHIP_MEM_DEVICE", what);
  return TRACYHIP_OK;
}

int variants_validate(const tracyhip_decompose_job* job, const tracyhip_decompose_result* res, const uint32_t* slice_pos, const tracyhip_params* prm,
                      int mem, const tracyhip_variants_result* out) {
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return set_error(TRACYHIP_ERR_ARG, "bad mem kind");
  if (!job || !res || !out) return set_error(TRACYHIP_ERR_ARG, "null job / decompose result / variants result");
  if (!prm) return set_error(TRACYHIP_ERR_ARG, "null params");
  if (!var_caps_ok(out->max_variants, out->max_text)) return TRACYHIP_ERR_RANGE;
  if (job->ntraces == 0) return TRACYHIP_OK;
  if (!out->var || !out->text || !out->var_n || !out->var_flags) return set_error(TRACYHIP_ERR_ARG, "null result arrays (var / text / var_n / var_flags)");
  if (!slice_pos) return set_error(TRACYHIP_ERR_ARG, "null slice_pos");
  if ((job->trim_left_each == nullptr) != (job->trim_right_each == nullptr))
    return set_error(TRACYHIP_ERR_ARG, "job: trim_left_each and trim_right_each must be given together");
  if (job->trim_left_each) {
    for (uint32_t t = 0; t < job->ntraces; ++t)
      if (job->trim_left_each[t] > 0x7fffffffu || job->trim_right_each[t] > 0x7fffffffu)
        return set_error(TRACYHIP_ERR_ARG, "job: trim of trace %u above INT32_MAX", t);
  } else if (job->dprm.trim_left < 0 || job->dprm.trim_right < 0) return set_error(TRACYHIP_ERR_ARG, "negative trim");
  if (!job->bc.primary || !job->bc.bc_offset || !job->bc.bc_len) return set_error(TRACYHIP_ERR_ARG, "job: null primary / bc_offset / bc_len");
  if (job->refs.kind != TRACYHIP_SEQ_CHAR || !job->refs.data || !job->refs.offset || !job->refs.length)
    return set_error(TRACYHIP_ERR_ARG, "job: refs must be a CHAR set with data / offset / length");
  if (!res->status || !res->forward) return set_error(TRACYHIP_ERR_ARG, "decompose result: null status / forward");
  if (!res->secdecomp) return set_error(TRACYHIP_ERR_ARG, "decompose result: null secdecomp");
  for (int k = 0; k < 2; ++k) {
    if (!res->slice_begin[k] || !res->slice_len[k] || !res->ref_pos[k])
      return set_error(TRACYHIP_ERR_ARG, "decompose result: null slice_begin / slice_len / ref_pos of allele %d", k + 1);
    if (!res->ops[k] || !res->ops_offset[k] || !res->ops_len[k]) return set_error(TRACYHIP_ERR_ARG, "decompose result: null ops / ops_offset / ops_len of allele %d", k + 1);
  }
  for (uint32_t t = 0; t < job->ntraces; ++t)
    if ((job->ref_index ? job->ref_index[t] : t) >= job->refs.count) return set_error(TRACYHIP_ERR_ARG, "trace %u indexes past the reference set", t);
  return TRACYHIP_OK;
}

// what the host keeps alive per chunk until the stream has been waited for (the uploads read these vectors)
struct ChunkHost {
  std::vector<VarDesc> desc;
  std::vector<PairDesc> pairs;  // [forward allele 1 | forward allele 2 | re-alignments]
  std::vector<VarRcDesc> rc;
  std::vector<uint64_t> off1, off2, voff;
  std::vector<uint64_t> foff[2];  // a forward alignment's ops offset less the first offset of the chunk's region, by trace of the chunk
  std::vector<uint32_t> len1, len2;
};

int variants_run(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_decompose_result* res, const uint32_t* slice_pos,
                 const tracyhip_params* prm, int mem, const tracyhip_variants_result* out) {
  const uint32_t nt = job->ntraces;
  hipStream_t st = ctx->stream;
  DevBuf* const B = ctx->dev;
  const bool host = mem == TRACYHIP_MEM_HOST;
  int rc;
  if ((rc = check_mem_kind(out->var, mem, "var")) || (rc = check_mem_kind(res->ops[0], mem, "the decompose result's ops")) ||
      (rc = check_mem_kind(job->bc.primary, mem, "the job's primary basecalls")))
    return rc;
  double stage_ms[4] = {0, 0, 0, 0};  // plan, re-alignments, rows + scan, results
  auto clock_now = [] { return std::chrono::steady_clock::now(); };
  auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(clock_now() - t).count(); };
  auto t_stage = clock_now();

  // ---- what the host plans from: one read of the per-trace results (a host caller's arrays are read in place) ----
  std::vector<uint8_t> v_fwd;
  std::vector<int32_t> v_status;
  std::vector<uint32_t> v_u32[8];
  const uint8_t* h_fwd = res->forward;
  const int32_t* h_status = res->status;
  const uint32_t *h_sb[2] = {res->slice_begin[0], res->slice_begin[1]}, *h_sl[2] = {res->slice_len[0], res->slice_len[1]};
  const uint32_t *h_rp[2] = {res->ref_pos[0], res->ref_pos[1]}, *h_ol[2] = {res->ops_len[0], res->ops_len[1]};
  if (!host) {
    v_fwd.resize(nt); v_status.resize(nt);
    HIP_TRY(hipMemcpyAsync(v_fwd.data(), res->forward, nt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(v_status.data(), res->status, 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
    const uint32_t* src[8] = {h_sb[0], h_sb[1], h_sl[0], h_sl[1], h_rp[0], h_rp[1], h_ol[0], h_ol[1]};
    for (int i = 0; i < 8; ++i) {
      v_u32[i].resize(nt);
      HIP_TRY(hipMemcpyAsync(v_u32[i].data(), src[i], 4 * (size_t)nt, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx_sync(ctx));
    h_fwd = v_fwd.data(); h_status = v_status.data();
    for (int k = 0; k < 2; ++k) { h_sb[k] = v_u32[k].data(); h_sl[k] = v_u32[2 + k].data(); h_rp[k] = v_u32[4 + k].data(); h_ol[k] = v_u32[6 + k].data(); }
  }

  // ---- per trace: the trimmed allele (trimmedSeq), its reference, whether it is called and on which strand ----
  const TrimSrc trims = trims_of(job);
  struct Tr { uint64_t a_off, r_off; uint32_t m, r_len; bool usable, rev; };
  std::vector<Tr> T(nt);
  uint32_t usable = 0, nrev = 0;
  uint64_t ext_bc = 0, ext_ops[2] = {0, 0}, max_mn = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t L = job->bc.bc_len[t], ri = job->ref_index ? job->ref_index[t] : t;
    const uint32_t tl = trims.left(t), tr = trims.right(t);
    const bool trim = !((uint64_t)tl + tr + 1 >= L);
    Tr x{};
    x.a_off = job->bc.bc_offset[t] + (trim ? tl : 0u);
    x.m = trim ? L - tl - tr : L;
    x.r_off = job->refs.offset[ri]; x.r_len = job->refs.length[ri];
    x.usable = h_status[t] == 0;
    x.rev = x.usable && !h_fwd[t];
    ext_bc = std::max<uint64_t>(ext_bc, job->bc.bc_offset[t] + L);
    if (x.usable) {
      ++usable;
      nrev += x.rev ? 1u : 0u;
      for (int k = 0; k < 2; ++k) {
        if ((uint64_t)h_sb[k][t] + h_sl[k][t] > x.r_len)
          return set_error(TRACYHIP_ERR_ARG, "trace %u: slice %d [%u, +%u) leaves its reference of %u", t, k + 1, h_sb[k][t], h_sl[k][t], x.r_len);
        if (!x.rev && h_ol[k][t] > (uint64_t)x.m + h_sl[k][t])
          return set_error(TRACYHIP_ERR_ARG, "trace %u: ops_len[%d] = %u exceeds allele + slice", t, k, h_ol[k][t]);
        if (!x.rev) ext_ops[k] = std::max<uint64_t>(ext_ops[k], res->ops_offset[k][t] + h_ol[k][t]);
        max_mn = std::max<uint64_t>(max_mn, (uint64_t)x.m + h_sl[k][t]);
      }
    }
    T[t] = x;
  }
  tracyhip_params p10 = *prm;
  p10.hfree = 1; p10.vfree = 0;  // AlignConfig<true, false>, indigo.h:414
  if ((rc = check_params(&p10, max_mn))) return rc;

  // ---- the payloads on the device ----
  const void *d_pri, *d_sec, *d_refs, *d_fops[2];
  if ((rc = stage_in(ctx, B[VB_IN_PRIMARY], job->bc.primary, ext_bc, mem, &d_pri))) return rc;
  if ((rc = stage_in(ctx, B[VB_IN_SECDECOMP], res->secdecomp, ext_bc, mem, &d_sec))) return rc;
  if ((rc = stage_in(ctx, B[VB_IN_REFS], job->refs.data, seqset_extent(job->refs), mem, &d_refs))) return rc;
  if ((rc = stage_in(ctx, B[VB_IN_OPS0], res->ops[0], ext_ops[0], mem, &d_fops[0]))) return rc;
  if ((rc = stage_in(ctx, B[VB_IN_OPS1], res->ops[1], ext_ops[1], mem, &d_fops[1]))) return rc;
  const uint32_t* d_folen[2] = {res->ops_len[0], res->ops_len[1]};
  if (host) {
    uint32_t* d_len; HIP_TRY(ensure_into(B[VB_LEN], 2 * (size_t)nt, d_len));
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(hipMemcpyAsync(d_len + (size_t)k * nt, res->ops_len[k], 4 * (size_t)nt, hipMemcpyHostToDevice, st));
      d_folen[k] = d_len + (size_t)k * nt;
    }
  }
  VarOut o;
  if ((rc = var_out_begin(ctx, nt, *out, mem, o))) return rc;

  // ---- chunks of consecutive traces whose rows (two per alignment), reverse complements and op strings fit the workspace limit.  A
  // forward alignment's rows sit where its ops sit in the caller's layout: a chunk holds the span of its traces' regions ----
  struct Chunk {
    uint32_t lo, hi, nrev, nfwd;
    uint64_t flo[2], fhi[2], rev_bytes;
    uint64_t rows() const { return (fhi[0] - flo[0]) + (fhi[1] - flo[1]) + rev_bytes; }
    uint64_t bytes() const { return 2 * rows() + 2 * rev_bytes; }
  };
  uint64_t limit = 0;
  if ((rc = workspace_limit(ctx, B[DB_ROWS0].cap + B[DB_ROWS1].cap + B[VB_SEQ].cap + B[VB_OPS].cap, &limit))) return rc;
  std::vector<Chunk> chunks;
  {
    const Chunk fresh{0, 0, 0, 0, {~0ull, ~0ull}, {0, 0}, 0};
    auto with = [&](Chunk c, uint32_t t) {
      const Tr& x = T[t];
      if (x.usable && x.rev) {
        ++c.nrev;
        for (int k = 0; k < 2; ++k) c.rev_bytes += (uint64_t)x.m + h_sl[k][t];
      } else if (x.usable) {
        ++c.nfwd;
        for (int k = 0; k < 2; ++k) {
          c.flo[k] = std::min<uint64_t>(c.flo[k], res->ops_offset[k][t]);
          c.fhi[k] = std::max<uint64_t>(c.fhi[k], res->ops_offset[k][t] + h_ol[k][t]);
        }
      }
      c.hi = t + 1;
      return c;
    };
    auto norm = [](Chunk c) { for (int k = 0; k < 2; ++k) if (c.fhi[k] < c.flo[k] || c.flo[k] == ~0ull) c.flo[k] = c.fhi[k] = 0; return c; };
    Chunk c = fresh;
    for (uint32_t t = 0; t < nt; ++t) {
      Chunk n = with(c, t);
      if (norm(n).bytes() > limit) {
        if (c.hi == c.lo) return set_error(TRACYHIP_ERR_OOM, "trace %u needs %llu bytes of rows and op strings, workspace limit is %llu", t,
                                           (unsigned long long)norm(n).bytes(), (unsigned long long)limit);
        chunks.push_back(norm(c));
        c = fresh; c.lo = c.hi = t;
        n = with(c, t);
        if (norm(n).bytes() > limit) return set_error(TRACYHIP_ERR_OOM, "trace %u needs %llu bytes of rows and op strings, workspace limit is %llu", t,
                                                      (unsigned long long)norm(n).bytes(), (unsigned long long)limit);
      }
      c = n;
    }
    if (c.hi > c.lo) chunks.push_back(norm(c));
  }
  // every buffer at its largest before the first launch (a buffer that grows frees what it outgrows)
  uint64_t max_rows = 1, max_rev = 1;
  uint32_t max_n = 0, max_pairs = 0, max_nrev = 0;
  for (const Chunk& c : chunks) {
    max_rows = std::max(max_rows, c.rows()); max_rev = std::max(max_rev, c.rev_bytes);
    max_n = std::max(max_n, c.hi - c.lo); max_pairs = std::max(max_pairs, 2 * (c.nfwd + c.nrev)); max_nrev = std::max(max_nrev, c.nrev);
  }
  uint8_t *d_rows0, *d_rows1, *d_seq, *d_vops;
  HIP_TRY(ensure_into(B[DB_ROWS0], (size_t)max_rows, d_rows0));
  HIP_TRY(ensure_into(B[DB_ROWS1], (size_t)max_rows, d_rows1));
  HIP_TRY(ensure_into(B[VB_SEQ], (size_t)max_rev, d_seq));
  HIP_TRY(ensure_into(B[VB_OPS], (size_t)max_rev, d_vops));
  VarDesc* d_desc; HIP_TRY(ensure_into(B[VB_DESC], (size_t)max_n, d_desc));
  PairDesc* d_pairs; HIP_TRY(ensure_into(B[VB_PAIRS], (size_t)std::max(1u, max_pairs), d_pairs));
  VarRcDesc* d_rc; HIP_TRY(ensure_into(B[VB_RCDESC], (size_t)std::max(1u, 4 * max_nrev), d_rc));
  uint32_t* d_vlen; HIP_TRY(ensure_into(B[VB_OPS_LEN], (size_t)std::max(1u, 2 * max_nrev), d_vlen));
  // offsets the alignment_rows launches index by PairDesc::out: [allele 1 of every trace | allele 2 | the chunk's re-alignments]
  uint64_t* d_off; HIP_TRY(ensure_into(B[VB_OPS_OFF], 2 * (size_t)nt + 2 * (size_t)max_nrev + 1, d_off));
  stage_ms[0] += since(t_stage);
  int32_t herr[kErrWords] = {};  // error words of the last traceback batch, judged behind the wait that follows it
  bool verdict_due = false;

  std::deque<ChunkHost> keep;
  int trc;
  for (const Chunk& c : chunks) {
    t_stage = clock_now();
    keep.emplace_back();
    ChunkHost& h = keep.back();
    const uint32_t n = c.hi - c.lo;
    h.desc.resize(n);
    for (int k = 0; k < 2; ++k) h.foff[k].assign(n, 0);
    // the chunk's rows: [forward allele 1 | forward allele 2 | re-alignments]; a forward alignment at its ops offset less the region's first
    const uint64_t reg[3] = {0, c.fhi[0] - c.flo[0], (c.fhi[0] - c.flo[0]) + (c.fhi[1] - c.flo[1])};
    h.pairs.reserve(2 * (size_t)(c.nfwd + c.nrev));
    std::vector<PairDesc> second;
    second.reserve(c.nfwd);
    uint64_t seq_at = 0, ops_at = 0;
    uint32_t slot = 0;
    for (uint32_t t = c.lo; t < c.hi; ++t) {
      const Tr& x = T[t];
      VarDesc d{};
      d.forward = h_fwd[t] ? 1u : 0u; d.bc_len = job->bc.bc_len[t]; d.skip = x.usable ? 0u : 1u; d.out = t;
      d.trim_left = trims.left(t); d.trim_right = trims.right(t);
      if (x.usable && !x.rev) {
        for (int k = 0; k < 2; ++k) {
          PairDesc p{};
          p.a1_off = x.a_off; p.a2_off = x.r_off + h_sb[k][t]; p.m = x.m; p.n = h_sl[k][t]; p.a1_stride = p.m; p.a2_stride = p.n; p.out = t;
          (k ? second : h.pairs).push_back(p);
          h.foff[k][t - c.lo] = res->ops_offset[k][t] - c.flo[k];
          const uint64_t at = reg[k] + h.foff[k][t - c.lo];
          d.a[k] = VarAln{d_rows0 + at, d_rows1 + at, d_folen[k] + t, (int32_t)(slice_pos[t] + h_rp[k][t]), 0u};
        }
      } else if (x.rev) {
        const bool flip = !job->oriented;  // the decompose call reverse-complemented the reference itself
        for (int k = 0; k < 2; ++k) {
          const uint32_t sl = h_sl[k][t];
          h.rc.push_back(VarRcDesc{static_cast<const uint8_t*>(k ? d_sec : d_pri) + x.a_off, seq_at, x.m, 0u, x.m, 0u});
          h.off1.push_back(seq_at); h.len1.push_back(x.m);
          seq_at += x.m;
          h.rc.push_back(VarRcDesc{static_cast<const uint8_t*>(d_refs) + x.r_off, seq_at, x.r_len, h_sb[k][t], sl, flip ? 1u : 0u});
          h.off2.push_back(seq_at); h.len2.push_back(sl);
          seq_at += sl;
          h.voff.push_back(ops_at);
          const uint64_t at = reg[2] + ops_at;
          d.a[k] = VarAln{d_rows0 + at, d_rows1 + at, d_vlen + 2 * slot + k, (int32_t)(slice_pos[t] + h_rp[k][t]), 0u};
          ops_at += (uint64_t)x.m + sl;
        }
        ++slot;
      }
      h.desc[t - c.lo] = d;
    }
    const uint32_t nf = (uint32_t)h.pairs.size();
    h.pairs.insert(h.pairs.end(), second.begin(), second.end());
    for (uint32_t i = 0; i < 2 * c.nrev; ++i) {
      PairDesc p{};
      p.a1_off = h.off1[i]; p.a2_off = h.off2[i]; p.m = h.len1[i]; p.n = h.len2[i]; p.a1_stride = p.m; p.a2_stride = p.n; p.out = i;
      h.pairs.push_back(p);
    }
    HIP_TRY(hipMemcpyAsync(d_desc, h.desc.data(), sizeof(VarDesc) * (size_t)n, hipMemcpyHostToDevice, st));
    if (!h.pairs.empty()) HIP_TRY(hipMemcpyAsync(d_pairs, h.pairs.data(), sizeof(PairDesc) * h.pairs.size(), hipMemcpyHostToDevice, st));
    if (c.nfwd)
      for (int k = 0; k < 2; ++k) HIP_TRY(hipMemcpyAsync(d_off + (size_t)k * nt + c.lo, h.foff[k].data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
    stage_ms[0] += since(t_stage);

    // ---- reverse traces: reverse complements, the traceback batch (one synchronisation), then rows like the rest ----
    if (c.nrev) {
      t_stage = clock_now();
      HIP_TRY(hipMemcpyAsync(d_rc, h.rc.data(), sizeof(VarRcDesc) * h.rc.size(), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_off + 2 * (size_t)nt, h.voff.data(), 8 * h.voff.size(), hipMemcpyHostToDevice, st));
      if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 2 * seq_at))) return trc;
      hipLaunchKernelGGL(var_revcomp_kernel, dim3((uint32_t)h.rc.size()), dim3(256), 0, st, d_rc, d_seq);
      HIP_TRY(hipGetLastError());
      if ((trc = timing_end(ctx))) return trc;
      tracyhip_pairs pr{};
      pr.npairs = 2 * c.nrev;
      pr.a1 = tracyhip_seqset{TRACYHIP_SEQ_CHAR, d_seq, h.off1.data(), h.len1.data(), pr.npairs};
      pr.a2 = tracyhip_seqset{TRACYHIP_SEQ_CHAR, d_seq, h.off2.data(), h.len2.data(), pr.npairs};
      {  // what tracyhip_gotoh_align runs for these strings, queued without its wait
        DpProblem pb;
        DpProblemLease lease(ctx, pb);
        uint64_t mn = 0;
        if ((rc = build_problem(ctx, &pr, TRACYHIP_MEM_DEVICE, false, pb, &mn))) return rc;
        if ((rc = run_dp(ctx, pb, &p10, false, true, nullptr, d_vops, d_off + 2 * (size_t)nt, d_vlen, DP_PLAIN, nullptr, herr))) return rc;
        verdict_due = true;
      }
      stage_ms[1] += since(t_stage);
    }
    t_stage = clock_now();
    if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return trc;
    for (int k = 0; k < 3; ++k) {
      RowsArgs ra{};
      ra.npairs = k < 2 ? c.nfwd : 2 * c.nrev;
      if (!ra.npairs) continue;
      ra.pairs = d_pairs + (k == 0 ? 0u : k == 1 ? nf : 2 * nf);
      ra.a1 = k == 0 ? d_pri : k == 1 ? d_sec : d_seq;
      ra.a2 = k < 2 ? d_refs : d_seq;
      ra.ops = k < 2 ? static_cast<const uint8_t*>(d_fops[k]) + c.flo[k] : d_vops;  // (ops and rows share one offset per pair: the region's first is taken off both)
      ra.ops_off = d_off + (size_t)k * nt;
      ra.ops_len = k < 2 ? d_folen[k] : d_vlen;
      ra.rows0 = d_rows0 + reg[k];
      ra.rows1 = d_rows1 + reg[k];
      HIP_TRY(launch_alignment_rows(ra, st));
    }
    if ((trc = timing_end(ctx))) return trc;
    if ((rc = launch_variants(ctx, d_desc, n, *out, o))) return rc;
    // the chunk's one wait, behind its scan: the next traceback batch reuses the context's pinned descriptors.  The last chunk's is the
    // first wait of var_out_end.
    if (verdict_due && &c != &chunks.back()) {
      HIP_TRY(ctx_sync(ctx));
      verdict_due = false;
      if ((rc = range_verdict(&p10, herr, {}, max_mn, kTagShift))) return rc;
    }
    stage_ms[2] += since(t_stage);
  }

  t_stage = clock_now();
  uint32_t truncated = 0;
  if ((rc = var_out_end(ctx, nt, *out, mem, o, &truncated))) return rc;
  timing_collect(ctx);
  if (verdict_due && (rc = range_verdict(&p10, herr, {}, max_mn, kTagShift))) return rc;
  stage_ms[3] += since(t_stage);
  ctx->stats.var_traces = usable;
  ctx->stats.var_realigned = nrev;
  ctx->stats.var_truncated = truncated;
  ctx->stats.var_chunks = (uint32_t)chunks.size();
  if (ctx->knobs.verbose)
    std::fprintf(stderr, "tracyhip_decompose_variants: traces %u called %u reverse %u truncated %u chunks %zu | plan_ms %.3f | realign_ms %.3f | "
                 "rows_scan_ms %.3f | results_ms %.3f | host_syncs %u\n", nt, usable, nrev, truncated, chunks.size(), stage_ms[0], stage_ms[1],
                 stage_ms[2], stage_ms[3], ctx->stats.host_syncs);
  return TRACYHIP_OK;
}

}  // namespace

extern "C" {

int tracyhip_call_variants(tracyhip_ctx* ctx, uint32_t ntraces, const uint8_t* rows0, const uint8_t* rows1, const uint64_t* rows_offset,
                           const uint32_t* rows_len, const int32_t* pos, const uint8_t* forward, const uint32_t* bc_len, uint32_t trim_left,
                           uint32_t trim_right, uint32_t max_variants, uint32_t max_text, int mem, tracyhip_variant* var, uint8_t* text,
                           uint32_t* var_n, uint32_t* var_flags) {
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return set_error(TRACYHIP_ERR_ARG, "bad mem kind");
  if (!var_caps_ok(max_variants, max_text)) return TRACYHIP_ERR_RANGE;
  if (ntraces && (!rows0 || !rows1 || !rows_offset || !rows_len || !pos || !forward || !bc_len || !var || !text || !var_n || !var_flags))
    return set_error(TRACYHIP_ERR_ARG, "null argument");
  int rc = ctx_begin(ctx);
  if (rc) return rc;
  if (ntraces == 0) return TRACYHIP_OK;
  hipStream_t st = ctx->stream;
  uint64_t ext = 0;
  for (uint32_t i = 0; i < 2 * ntraces; ++i) ext = std::max<uint64_t>(ext, rows_offset[i] + rows_len[i]);
  const void *d_r0 = nullptr, *d_r1 = nullptr;
  if (ext && ((rc = stage_in(ctx, ctx->dev[DB_ROWS0], rows0, ext, mem, &d_r0)) || (rc = stage_in(ctx, ctx->dev[DB_ROWS1], rows1, ext, mem, &d_r1)))) return rc;
  if (!ext) d_r0 = d_r1 = rows0;  // (no alignment has a column: nothing is read)
  uint32_t* d_len; HIP_TRY(ensure_into(ctx->dev[VB_LEN], 2 * (size_t)ntraces, d_len));
  HIP_TRY(hipMemcpyAsync(d_len, rows_len, 8 * (size_t)ntraces, hipMemcpyHostToDevice, st));
  std::vector<VarDesc> hd(ntraces);
  for (uint32_t t = 0; t < ntraces; ++t) {
    VarDesc d{};
    for (uint32_t k = 0; k < 2; ++k) {
      const size_t i = 2 * (size_t)t + k;
      d.a[k] = VarAln{static_cast<const uint8_t*>(d_r0) + rows_offset[i], static_cast<const uint8_t*>(d_r1) + rows_offset[i], d_len + i, pos[i], 0u};
    }
    d.forward = forward[t] ? 1u : 0u; d.bc_len = bc_len[t]; d.skip = 0; d.out = t; d.trim_left = trim_left; d.trim_right = trim_right;
    hd[t] = d;
  }
  VarDesc* d_desc; HIP_TRY(ensure_into(ctx->dev[VB_DESC], (size_t)ntraces, d_desc));
  HIP_TRY(hipMemcpyAsync(d_desc, hd.data(), sizeof(VarDesc) * (size_t)ntraces, hipMemcpyHostToDevice, st));
  const tracyhip_variants_result r{var, text, var_n, var_flags, max_variants, max_text};
  VarOut o;
  if ((rc = var_out_begin(ctx, ntraces, r, mem, o))) return rc;
  if ((rc = launch_variants(ctx, d_desc, ntraces, r, o))) return rc;
  uint32_t truncated = 0;
  rc = var_out_end(ctx, ntraces, r, mem, o, &truncated);  // (waits for the stream: hd has been read)
  timing_collect(ctx);
  return rc;
}

int tracyhip_decompose_variants_validate(const tracyhip_decompose_job* job, const tracyhip_decompose_result* res, const uint32_t* slice_pos,
                                         const tracyhip_params* prm, int mem, const tracyhip_variants_result* out) {
  return variants_validate(job, res, slice_pos, prm, mem, out);
}

int tracyhip_decompose_variants(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_decompose_result* res,
                                const uint32_t* slice_pos, const tracyhip_params* prm, int mem, const tracyhip_variants_result* out) {
  int rc = variants_validate(job, res, slice_pos, prm, mem, out);  // (before any device is touched)
  if (rc) return rc;
  if ((rc = ctx_begin(ctx))) return rc;
  ctx->stats = tracyhip_call_stats{};
  ctx->stats.traces = job->ntraces;
  if (job->ntraces == 0) return check_params(prm, 0);
  return variants_run(ctx, job, res, slice_pos, prm, mem, out);
}

int tracyhip_decompose_variants_async(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_decompose_result* res,
                                      const uint32_t* slice_pos, const tracyhip_params* prm, int mem, const tracyhip_variants_result* out) {
  if (!ctx || !job || !res || !prm || !out) return set_error(TRACYHIP_ERR_ARG, "null context / job / decompose result / params / variants result");
  if (job->ntraces && !slice_pos) return set_error(TRACYHIP_ERR_ARG, "null slice_pos");
  const tracyhip_decompose_job j = *job;
  const tracyhip_decompose_result r = *res;
  const tracyhip_params q = *prm;
  const tracyhip_variants_result o = *out;
  auto sp = std::make_shared<std::vector<uint32_t>>(slice_pos, slice_pos + (slice_pos ? job->ntraces : 0));
  return async_submit(ctx, [=]() { return tracyhip_decompose_variants(ctx, &j, &r, sp->data(), &q, mem, &o); });
}

}  // extern "C"
