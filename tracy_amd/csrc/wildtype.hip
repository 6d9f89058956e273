// wildtype.hip -- tracyhip_align_traces with a wildtype-trace reference (sage.h:261-300 + :311): a plate of traces against one or a
// few control reads, each a second chromatogram used as a float profile (tracyhip_align_job::refs of kind PROFILE).
//
// Per trace: gotohScore(trimmed view, W) and gotohScore(trimmed view, revcomp W) in one profile x profile score launch; forward iff
// gsFwd > gsRev, decided on the device (wt_decide_kernel patches the traceback descriptor); gotoh(FULL profile, chosen strand)
// (traceback, fused walk); the _createAlignment rows when the caller wants them.  The reverse complement and the classes are made once
// per DISTINCT wildtype.  The stages are consensus_run's (consensus.hip) and the launch loops prof_batch.hip's; what is new is that
// the scores and the traceback of one trace have different heights, hence two launch orders (wildtype_plan.h).  Everything after
// the profile classes is queued on the stream without the host in between: two synchronisations per call (classes, end).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "launch.h"
#include "pipe_internal.h"
#include "wildtype_plan.h"

using namespace tracyhip;

namespace {

struct WtDecide {
  PairDesc* trace;          // the traceback descriptors of a chunk
  uint32_t n;
  const int32_t* sc;        // strand scores by trace: per = 2: {gsFwd, gsRev}; per = 1: the one score of a caller-oriented job
  uint32_t per;
  const uint8_t* oriented;  // per = 1: the caller's strand per trace
  uint64_t rev_base;        // where the reverse strands start in the wildtype buffer
  int32_t *score_fwd, *score_rev, *score_prelim;
  uint8_t* forward;
  uint32_t *slice_begin, *slice_len, *ref_pos;
};

// strand of every trace of a chunk from its two orientation scores (sage.h:293: forward iff gsFwd > gsRev, a tie is reverse); the
// traceback descriptor of a reverse trace moves onto the reverse strand.  The score descriptors are in another order than these: a
// trace's scores are found through PairDesc::out (the sweeps wrote them at 2 * trace / 2 * trace + 1), not by position.
__global__ void wt_decide_kernel(WtDecide a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t i = a.trace[j].out;
  const uint32_t cols = a.trace[j].n;
  int32_t f, r;
  bool fwd;
  if (a.per == 2) {
    f = a.sc[2ull * i];
    r = a.sc[2ull * i + 1];
    fwd = f > r;
    if (!fwd) a.trace[j].a2_off += a.rev_base;
  } else {
    f = a.sc[i];
    r = f;
    fwd = a.oriented[i] != 0;
  }
  a.score_fwd[i] = f;
  a.score_rev[i] = r;
  a.forward[i] = fwd ? 1 : 0;
  a.score_prelim[i] = fwd ? f : r;
  a.slice_begin[i] = 0;
  a.slice_len[i] = cols;
  a.ref_pos[i] = 0;
}

// (its one caller, wildtype_align below, has checked ref_index against the wildtype set and that every profile has columns: the
// geometry loop indexes through ref_index unchecked)
int wildtype_run(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm, int mem, const tracyhip_align_result* out,
                 bool wide) {
  const uint32_t nt = job->ntraces;
  hipStream_t st = ctx->stream;
  const tracyhip_seqset& sp = job->profiles;
  const tracyhip_seqset& sw = job->refs;
  const uint32_t nw = job->ref_index ? sw.count : nt;  // the distinct wildtypes
  const uint32_t per = job->oriented ? 1u : 2u;        // strands scored per trace
  const TrimSrc trims = trims_of(job);
  const bool want_rows = out->rows0 != nullptr;
  DevBuf* const B = ctx->dev;  // indexed by the WB_* roles (capi_internal.h)

  // ---- geometry: the trimmed view of every trace (createProfile's clamp: l + r >= mf gives 0 / 0) and its wildtype ----
  std::vector<WtTrace> tr(nt);
  std::vector<uint32_t> tl(nt), widx(nt);
  uint64_t e1 = 0, e2 = 0, max_mn = 0, ext = 0;
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t mf = sp.length[t];
    uint32_t l = trims.left(t), r = trims.right(t);
    if ((uint64_t)l + r >= mf) l = r = 0;
    const uint32_t w = job->ref_index ? job->ref_index[t] : t;
    tl[t] = l;
    widx[t] = w;
    tr[t] = WtTrace{mf, mf - l - r, sw.length[w], 0};
    e1 = std::max<uint64_t>(e1, sp.offset[t] + 6ull * mf);
    max_mn = std::max<uint64_t>(max_mn, (uint64_t)mf + sw.length[w]);
    ext = std::max<uint64_t>(ext, out->ops_offset[t] + mf + sw.length[w]);  // extent of ops / rows (capacity mf + n)
  }
  for (uint32_t w = 0; w < nw; ++w) e2 = std::max<uint64_t>(e2, sw.offset[w] + 6ull * sw.length[w]);
  int rc;
  if ((rc = check_params(prm, max_mn))) return rc;

  // ---- inputs: the traces where the caller has them (or staged), [W | revcomp W] of the distinct wildtypes in one buffer ----
  const void* d_a1v = nullptr;
  if ((rc = stage_in(ctx, ctx->dev[DB_IN1], sp.data, e1 * 4, mem, &d_a1v))) return rc;
  const float* d_a1 = static_cast<const float*>(d_a1v);
  float* d_a2; HIP_TRY(ensure_into(B[WB_W], per * e2, d_a2));
  HIP_TRY(hipMemcpyAsync(d_a2, sw.data, e2 * 4, mem == TRACYHIP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  const uint64_t rev_base = e2;
  {
    std::vector<ProfSeq> hs((size_t)nt + nw);
    for (uint32_t t = 0; t < nt; ++t) hs[t] = ProfSeq{sp.offset[t], sp.length[t], 0};
    for (uint32_t w = 0; w < nw; ++w) hs[nt + w] = ProfSeq{sw.offset[w], sw.length[w], 0};
    HIP_TRY(B[WB_SEQS].ensure(sizeof(ProfSeq) * hs.size()));
    HIP_TRY(hipMemcpyAsync(B[WB_SEQS].p, hs.data(), sizeof(ProfSeq) * hs.size(), hipMemcpyHostToDevice, st));
  }
  const ProfSeq* d_seqs = static_cast<const ProfSeq*>(B[WB_SEQS].p);
  int trc;
  if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 2 * 24ull * (e2 / 6)))) return trc;
  if (per == 2) HIP_TRY(launch_prof_revcomp(d_seqs + nt, nw, d_a2, d_a2, rev_base, st));
  // classes: row 4 of every trace (its full profile, once) and wildtype (the reverse strand has the same row 4), column classes of both strands
  uint8_t* d_zero; HIP_TRY(ensure_into(B[WB_CLASS], (size_t)nt + nw, d_zero));
  uint8_t* d_colclass = nullptr;
  if (!ctx->knobs.no_screen) HIP_TRY(ensure_into(B[WB_COLCLASS], per * e2, d_colclass));
  HIP_TRY(launch_prof_classify(d_seqs, nt, d_a1, d_zero, nullptr, st));
  HIP_TRY(launch_prof_classify(d_seqs + nt, nw, d_a2, d_zero + nt, d_colclass, st));
  if (d_colclass && per == 2) HIP_TRY(launch_prof_classify(d_seqs + nt, nw, d_a2 + rev_base, d_zero + nt, d_colclass + rev_base, st));
  if ((trc = timing_end(ctx))) return trc;
  std::vector<uint8_t> hz((size_t)nt + nw);
  HIP_TRY(hipMemcpyAsync(hz.data(), d_zero, hz.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx_sync(ctx));  // (the classes choose the score bodies)

  // ---- plan (wildtype_plan.h): the two orders, the chunks whose planes and boundary rows fit the workspace ----
  for (uint32_t t = 0; t < nt; ++t) tr[t].row4 = (hz[t] && hz[nt + widx[t]]) ? 1u : 0u;
  uint64_t limit;
  if ((rc = workspace_limit(ctx, ctx->dev[DB_BITS].cap + ctx->dev[DB_SCRATCH].cap, &limit))) return rc;
  WtPlan plan;
  if (!wildtype_plan(tr.data(), nt, limit, per, plan))
    return set_error(TRACYHIP_ERR_OOM, "trace %lld needs %llu bytes of traceback planes, workspace limit is %llu", (long long)plan.too_large,
                     (unsigned long long)plan.need, (unsigned long long)limit);
  // descriptors: score pairs (`per` per trace, in score order) then traceback pairs (one per trace, in trace order)
  PairDesc* hsd; HIP_TRY(ensure_into(ctx->pin[PB_DESC], (per + 1) * (size_t)nt, hsd));
  PairDesc* htd = hsd + per * (size_t)nt;
  for (uint32_t j = 0; j < nt; ++j) {
    {
      const uint32_t t = plan.score_order[j];
      const WtTrace& g = tr[t];
      PairDesc d = prof_pair_desc(sp.offset[t] + tl[t], g.mt, sw.offset[widx[t]], g.n, g.row4 != 0);
      d.a1_stride = g.mf;  // the trimmed view keeps the stride of the full profile
      d.scratch_off = plan.scratch_off[t];
      d.out = per * t;
      hsd[per * (size_t)j] = d;
      if (per == 2) {
        d.a2_off += rev_base;
        if (wt_passes(g.mt, wt_strip_height(g.mt)) > 1) d.scratch_off += (uint64_t)g.n + 2;
        d.out = 2 * t + 1;
        hsd[2 * (size_t)j + 1] = d;
      }
    }
    const uint32_t t = plan.trace_order[j];
    const WtTrace& g = tr[t];
    PairDesc d = prof_pair_desc(sp.offset[t], g.mf, sw.offset[widx[t]], g.n, g.row4 != 0);
    d.scratch_off = plan.scratch_off[t];
    d.bits_off = plan.bits_off[t];
    d.out = t;
    htd[j] = d;
  }
  uint64_t max_words = 0, max_scr = 0;
  for (const WtChunk& c : plan.chunks) { max_words = std::max(max_words, c.words); max_scr = std::max(max_scr, c.scratch); }
  PairDesc* dsd; HIP_TRY(ensure_into(ctx->dev[DB_DESC], (per + 1) * (size_t)nt, dsd));
  HIP_TRY(hipMemcpyAsync(dsd, hsd, sizeof(PairDesc) * (per + 1) * (size_t)nt, hipMemcpyHostToDevice, st));
  PairDesc* dtd = dsd + per * (size_t)nt;
  HIP_TRY(ctx->dev[DB_BITS].ensure(std::max<uint64_t>(max_words * 8, 8)));
  if (max_scr) HIP_TRY(ctx->dev[DB_SCRATCH].ensure(max_scr * 8));
  HIP_TRY(ctx->dev[DB_ERR].ensure(kErrBytes));
  HIP_TRY(hipMemsetAsync(ctx->dev[DB_ERR].p, 0, sizeof(int32_t) * kErrWords, st));
  int32_t* d_sc; HIP_TRY(ensure_into(B[WB_SC2], per * (size_t)nt, d_sc));
  uint64_t* d_off; HIP_TRY(ensure_into(B[WB_OFF], nt, d_off));
  HIP_TRY(ctx->pin[PB_OFF].ensure(sizeof(uint64_t) * (size_t)nt));
  std::memcpy(ctx->pin[PB_OFF].p, out->ops_offset, sizeof(uint64_t) * (size_t)nt);
  HIP_TRY(hipMemcpyAsync(d_off, ctx->pin[PB_OFF].p, sizeof(uint64_t) * (size_t)nt, hipMemcpyHostToDevice, st));
  const uint8_t* d_oriented = nullptr;
  if (per == 1) {
    HIP_TRY(B[WB_ORIENTED].ensure(nt));
    HIP_TRY(ctx->pin[PB_TMP].ensure(nt));
    std::memcpy(ctx->pin[PB_TMP].p, job->oriented, nt);
    HIP_TRY(hipMemcpyAsync(B[WB_ORIENTED].p, ctx->pin[PB_TMP].p, nt, hipMemcpyHostToDevice, st));
    d_oriented = static_cast<const uint8_t*>(B[WB_ORIENTED].p);
  }

  // per-trace results and payloads: the caller's (MEM_DEVICE) or staged (MEM_HOST); score_prelim is optional in both
  int32_t *o_sf = out->score_fwd, *o_sr = out->score_rev, *o_pre = out->score_prelim, *o_final = out->score_final;
  uint32_t *o_sb = out->slice_begin, *o_sl = out->slice_len, *o_rp = out->ref_pos, *o_len = out->ops_len;
  uint8_t *o_fwd = out->forward, *o_ops = out->ops, *o_r0 = out->rows0, *o_r1 = out->rows1;
  {
    const size_t per4 = 4 * (size_t)nt;
    uint8_t* p; HIP_TRY(ensure_into(B[WB_PAIR], 9 * per4, p));
    if (mem == TRACYHIP_MEM_HOST) {
      o_sf = reinterpret_cast<int32_t*>(p); o_sr = reinterpret_cast<int32_t*>(p + per4); o_final = reinterpret_cast<int32_t*>(p + 2 * per4);
      o_sb = reinterpret_cast<uint32_t*>(p + 3 * per4); o_sl = reinterpret_cast<uint32_t*>(p + 4 * per4); o_rp = reinterpret_cast<uint32_t*>(p + 5 * per4);
      o_len = reinterpret_cast<uint32_t*>(p + 6 * per4); o_fwd = p + 8 * per4;
      const uint64_t ea = (ext + 255) & ~255ull;  // (aligned sub-buffers)
      uint8_t* q; HIP_TRY(ensure_into(B[WB_PAY], (want_rows ? 3 : 1) * std::max<uint64_t>(ea, 256), q));
      o_ops = q;
      if (want_rows) { o_r0 = q + ea; o_r1 = q + 2 * ea; }
    }
    if (mem == TRACYHIP_MEM_HOST || !o_pre) o_pre = reinterpret_cast<int32_t*>(p + 7 * per4);
  }

  tracyhip_params p = *prm;
  p.hfree = 1;  // AlignConfig<true,false> semiglobal (sage.h:165), as in the rest of the call
  p.vfree = 0;
  DpArgs a = scoring_args(ctx, &p);
  a.a1 = d_a1;
  a.a2 = d_a2;
  a.bits = static_cast<uint64_t*>(ctx->dev[DB_BITS].p);
  a.bits32 = static_cast<uint32_t*>(ctx->dev[DB_BITS].p);
  a.scratch = static_cast<int32_t*>(ctx->dev[DB_SCRATCH].p);
  a.screen = ctx->knobs.no_screen ? 0 : 1;
  a.colcode = d_colclass;
  std::vector<std::pair<uint32_t, int>> narrow_launches;

  WtDecide wd{};
  wd.sc = d_sc; wd.per = per; wd.oriented = d_oriented; wd.rev_base = rev_base;
  wd.score_fwd = o_sf; wd.score_rev = o_sr; wd.score_prelim = o_pre; wd.forward = o_fwd;
  wd.slice_begin = o_sb; wd.slice_len = o_sl; wd.ref_pos = o_rp;

  for (const WtChunk& c : plan.chunks) {
    // orientation scores over the trimmed views: one launch per run of equal strip height (of mt) / term count
    a.scores = d_sc;
    if ((rc = prof_score_runs(ctx, &p, wide, a, hsd, dsd, plan.k_score.data(), c.lo, c.hi, narrow_launches, per))) return rc;
    const uint32_t cn = c.hi - c.lo;
    if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return trc;
    wd.trace = dtd + c.lo;
    wd.n = cn;
    hipLaunchKernelGGL(wt_decide_kernel, dim3((cn + 255) / 256), dim3(256), 0, st, wd);
    HIP_TRY(hipGetLastError());
    if ((trc = timing_end(ctx))) return trc;
    // gotoh(full profile, chosen strand): traceback planes + walk, runs by the strip height of mf
    a.scores = o_final;
    if ((rc = prof_trace_runs(ctx, a, htd, dtd, plan.k_trace.data(), c.lo, c.hi, o_ops, d_off, o_len))) return rc;
    if (want_rows) {
      RowsArgs ra{};
      ra.pairs = dtd + c.lo;
      ra.a1 = d_a1; ra.a2 = d_a2;
      ra.a1_profile = 1; ra.a2_profile = 1;
      ra.ops = o_ops; ra.ops_off = d_off; ra.ops_len = o_len;
      ra.rows0 = o_r0; ra.rows1 = o_r1;
      ra.npairs = cn;
      if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return trc;
      HIP_TRY(launch_alignment_rows(ra, st));
      if ((trc = timing_end(ctx))) return trc;
    }
  }

  // ---- one synchronisation: error words, results (MEM_HOST) ----
  int32_t herr[kErrWords] = {};
  HIP_TRY(hipMemcpyAsync(herr, ctx->dev[DB_ERR].p, sizeof(herr), hipMemcpyDeviceToHost, st));
  if (mem == TRACYHIP_MEM_HOST) {
    const size_t n4 = 4 * (size_t)nt;
    HIP_TRY(hipMemcpyAsync(out->score_fwd, o_sf, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->score_rev, o_sr, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->score_final, o_final, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->slice_begin, o_sb, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->slice_len, o_sl, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->ref_pos, o_rp, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->ops_len, o_len, n4, hipMemcpyDeviceToHost, st));
    if (out->score_prelim) HIP_TRY(hipMemcpyAsync(out->score_prelim, o_pre, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->forward, o_fwd, (size_t)nt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->ops, o_ops, ext, hipMemcpyDeviceToHost, st));
    if (want_rows) {
      HIP_TRY(hipMemcpyAsync(out->rows0, o_r0, ext, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out->rows1, o_r1, ext, hipMemcpyDeviceToHost, st));
    }
  }
  HIP_TRY(ctx_sync(ctx));
  timing_collect(ctx);
  const int verdict = range_verdict(&p, herr, narrow_launches, max_mn, kTagShift);
  if (verdict == kWiden) return kWiden;  // a 16-bit score launch met an un-normalised profile: the caller repeats on int32
  if (verdict != TRACYHIP_OK) return verdict;
  ctx->stats.wt_chunks = (uint32_t)plan.chunks.size();
  ctx->stats.stream_ordered = 1;
  return TRACYHIP_OK;
}

}  // namespace

namespace tracyhip {

// the wildtype branch of tracyhip_align_traces for one context; job, prm, mem and out have passed tracyhip_align_validate
int wildtype_align(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm, int mem, const tracyhip_align_result* out) {
  const uint32_t nt = job->ntraces;
  const tracyhip_seqset& sw = job->refs;
  if (!job->profiles.data) return set_error(TRACYHIP_ERR_ARG, "profiles: null data");
  if (!check_profile_columns(job->profiles, "profiles", 0, nt)) return TRACYHIP_ERR_ARG;
  if (job->ref_index) {
    for (uint32_t t = 0; t < nt; ++t)
      if (job->ref_index[t] >= sw.count)
        return set_error(TRACYHIP_ERR_ARG, "ref_index[%u] = %u, refs holds %u wildtype profiles", t, job->ref_index[t], sw.count);
  }
  if (!check_profile_columns(sw, "refs", 0, job->ref_index ? sw.count : nt)) return TRACYHIP_ERR_ARG;
  int rc = wildtype_run(ctx, job, prm, mem, out, false);
  if (rc == kWiden) rc = wildtype_run(ctx, job, prm, mem, out, true);
  if (rc == kWiden) rc = set_error(TRACYHIP_ERR_RANGE, "profile values outside the range of the score kernels");
  return rc;
}

}  // namespace tracyhip
