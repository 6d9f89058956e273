// consensus.hip -- tracyhip_consensus_traces: the hot section of `tracy consensus` (consensus.h:501-577) for a batch of trace pairs.
//
// Per pair: revcomp(second) on the device (profile.h:74-90, prof_batch.hip); gotohScore(first, second) and gotohScore(first,
// revcomp) in one profile x profile score launch (the launch loops are prof_batch.hip's); forward iff gsFwd > gsRev (decided on the
// device: cons_decide_kernel patches the traceback descriptors); gotoh of the chosen strand (traceback, fused walk);
// _createAlignment rows; the overlap test and pairwiseConsensus / gtLetter in consensus_kernel, one wave per pair.  Everything
// after the profile classes is queued on the stream without the host in between; the call synchronises once at its end (plus once
// for the classes, which choose the score kernels), then the host recomputes the columns the consensus screen flagged (consensus.h)
// and patches them in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "../host/consensus_out.hpp"
#include "capi_internal.h"
#include "consensus.h"
#include "launch.h"

using namespace tracyhip;

namespace {

// strand of every pair of a chunk from the two orientation scores (consensus.h:545: forward iff gsFwd > gsRev); the traceback
// descriptor then reads the reverse complement
__global__ void cons_decide_kernel(PairDesc* __restrict__ trace, uint32_t n, const int32_t* __restrict__ sc2, uint64_t rev_base,
                                   int32_t* __restrict__ score_fwd, int32_t* __restrict__ score_rev, uint8_t* __restrict__ forward) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = trace[j].out;
  const int32_t f = sc2[2ull * i], r = sc2[2ull * i + 1];
  const bool fwd = f > r;
  if (!fwd) trace[j].a2_off += rev_base;
  score_fwd[i] = f;
  score_rev[i] = r;
  forward[i] = fwd ? 1 : 0;
}

struct ConsArgs {
  const PairDesc* pairs;   // the traceback descriptors (a2_off already on the chosen strand)
  const float* a1;
  const float* a2;
  const uint8_t* rows0;
  const uint8_t* rows1;
  const uint64_t* off;     // per pair (PairDesc::out)
  const uint32_t* len;     // ops_len
  const uint16_t* gq;      // [kConsMaxPL + 1]
  uint8_t* cons;
  uint16_t* qual;
  uint32_t* cons_len;
  uint32_t* num_aligned;
  uint32_t* num_match;
  int32_t* status;
  ConsFixup* fix;
  uint32_t* nfix;          // counter; entries past fix_cap are counted, not written
  uint32_t fix_cap;
  uint32_t use_union, use_iupac, min_overlap;
  double match_fraction;
};

// pairwiseConsensus (consensus.h:189-238) after the overlap test (:540-549): one wave per pair.  Pass 1 counts aligned columns and
// matches; pass 2 walks the columns in rounds of 64 with the row positions s1 / s2 and the output slots as prefix counts of ballots.
__global__ __launch_bounds__(64) void consensus_kernel(ConsArgs a) {
  const PairDesc d = a.pairs[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const uint32_t t = d.out;
  const uint64_t off = a.off[t];
  const uint32_t L = a.len[t];
  const uint8_t* r0 = a.rows0 + off;
  const uint8_t* r1 = a.rows1 + off;
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t aligned = 0, match = 0;
  for (uint32_t b = 0; b < L; b += 64) {
    const uint32_t j = b + lane;
    bool al = false, mt = false;
    if (j < L) {
      const uint8_t c0 = r0[j], c1 = r1[j];
      al = c0 != '-' && c1 != '-';
      mt = al && c0 == c1;
    }
    aligned += (uint32_t)__popcll(__ballot(al));
    match += (uint32_t)__popcll(__ballot(mt));
  }
  const double frac = aligned ? (double)match / (double)aligned : 0.0;
  const bool ok = !(aligned < a.min_overlap || frac < a.match_fraction);
  if (lane == 0) {
    a.num_aligned[t] = aligned;
    a.num_match[t] = match;
    a.status[t] = ok ? TRACYHIP_CONS_OK : TRACYHIP_CONS_NO_OVERLAP;
  }
  if (!ok) {
    if (lane == 0) a.cons_len[t] = 0;
    return;
  }
  const float* p1 = a.a1 + d.a1_off;
  const float* p2 = a.a2 + d.a2_off;
  const uint64_t m = d.m, n = d.n;
  uint32_t s1 = 0, s2 = 0, slot = 0;
  for (uint32_t b = 0; b < L; b += 64) {
    const uint32_t j = b + lane;
    bool g0 = true, g1 = true;
    if (j < L) { g0 = r0[j] == '-'; g1 = r1[j] == '-'; }
    const uint64_t t0 = __ballot(!g0), t1 = __ballot(!g1);
    const uint32_t my1 = s1 + (uint32_t)__popcll(t0 & below), my2 = s2 + (uint32_t)__popcll(t1 & below);
    const bool al = !g0 && !g1;
    // an aligned column emits one letter; a column with a gap on one side emits the other side's with computeUnion (never two:
    // a column with both sides present is aligned)
    const bool emit = al || (a.use_union && (!g0 || !g1));
    const uint64_t o1 = __ballot(emit);
    const uint32_t out = slot + (uint32_t)__popcll(o1 & below);
    if (emit) {
      double cl[6];
      float f[6];
      if (al) {
        for (int k = 0; k < 6; ++k) f[k] = __fadd_rn(p1[k * m + my1], p2[k * n + my2]);  // float + float (consensus.h:177)
      } else if (!g0) {
        for (int k = 0; k < 6; ++k) f[k] = p1[k * m + my1];
      } else {
        for (int k = 0; k < 6; ++k) f[k] = p2[k * n + my2];
      }
      for (int k = 0; k < 6; ++k) cl[k] = (double)f[k];
      uint8_t letter;
      uint16_t q;
      const bool flag = cons_column(cl, a.use_iupac != 0, a.gq, &letter, &q);
      const uint64_t at = off + out;
      a.cons[at] = letter;
      a.qual[at] = q;
      if (flag) {
        const uint32_t w = atomicAdd(a.nfix, 1u);
        if (w < a.fix_cap) {
          ConsFixup fx;
          fx.slot = at;
          fx.pair = t;
          fx.pad = 0;
          for (int k = 0; k < 6; ++k) fx.cl[k] = f[k];
          a.fix[w] = fx;
        }
      }
    }
    s1 += (uint32_t)__popcll(t0);
    s2 += (uint32_t)__popcll(t1);
    slot += (uint32_t)__popcll(o1);
  }
  if (lane == 0) a.cons_len[t] = slot;
}

struct ConsPatch { uint64_t slot; uint32_t letter, qual; };
__global__ void cons_patch_kernel(const ConsPatch* __restrict__ p, uint32_t n, uint8_t* __restrict__ cons, uint16_t* __restrict__ qual) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  cons[p[i].slot] = (uint8_t)p[i].letter;
  qual[p[i].slot] = (uint16_t)p[i].qual;
}

bool check_profiles(const tracyhip_seqset& s, uint32_t np, const char* name) {
  if (!check_profile_set(s, name)) return false;
  if (s.count < np) return set_error(TRACYHIP_ERR_ARG, "%s: %u profiles for %u pairs", name, s.count, np), false;
  return check_profile_columns(s, name, 0, np);
}

int consensus_run(tracyhip_ctx* ctx, const tracyhip_consensus_job* job, const tracyhip_params* prm, int mem,
                  const tracyhip_consensus_result* out, bool wide) {
  const uint32_t np = job->npairs;
  hipStream_t st = ctx->stream;
  const tracyhip_seqset& s1 = job->first;
  const tracyhip_seqset& s2 = job->second;
  DevBuf* const B = ctx->dev;  // indexed by the CB_* roles (capi_internal.h)

  // ---- inputs: a1 where the caller has it (or staged), a2 = [second | revcomp(second)] in one buffer ----
  uint64_t e1 = 0, e2 = 0, max_mn = 0, ext = 0;
  for (uint32_t i = 0; i < np; ++i) {
    e1 = std::max<uint64_t>(e1, s1.offset[i] + 6ull * s1.length[i]);
    e2 = std::max<uint64_t>(e2, s2.offset[i] + 6ull * s2.length[i]);
    max_mn = std::max<uint64_t>(max_mn, (uint64_t)s1.length[i] + s2.length[i]);
    ext = std::max<uint64_t>(ext, out->offset[i] + s1.length[i] + s2.length[i]);  // extent of rows / ops / consensus (capacity m + n)
  }
  int rc;
  if ((rc = check_params(prm, max_mn))) return rc;
  const void* d_a1v = nullptr;
  if ((rc = stage_in(ctx, ctx->dev[DB_IN1], s1.data, e1 * 4, mem, &d_a1v))) return rc;
  const float* d_a1 = static_cast<const float*>(d_a1v);
  float* d_a2; HIP_TRY(ensure_into(B[CB_A2], 2 * e2, d_a2));
  HIP_TRY(hipMemcpyAsync(d_a2, s2.data, e2 * 4, mem == TRACYHIP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  const uint64_t rev_base = e2;
  {
    std::vector<ProfSeq> hs(2 * (size_t)np);
    for (uint32_t i = 0; i < np; ++i) {
      hs[i] = ProfSeq{s1.offset[i], s1.length[i], 0};
      hs[np + i] = ProfSeq{s2.offset[i], s2.length[i], 0};
    }
    HIP_TRY(B[CB_SEQS].ensure(sizeof(ProfSeq) * hs.size()));
    HIP_TRY(hipMemcpyAsync(B[CB_SEQS].p, hs.data(), sizeof(ProfSeq) * hs.size(), hipMemcpyHostToDevice, st));
  }
  const ProfSeq* d_seqs = static_cast<const ProfSeq*>(B[CB_SEQS].p);
  int trc;
  if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 2 * 24ull * (e2 / 6)))) return trc;
  HIP_TRY(launch_prof_revcomp(d_seqs + np, np, d_a2, d_a2, rev_base, st));
  // classes: row 4 of first, second (revcomp has the same row 4), column classes of both strands
  uint8_t* d_zero; HIP_TRY(ensure_into(B[CB_CLASS], 2 * (size_t)np, d_zero));
  uint8_t* d_colclass = nullptr;
  if (!ctx->knobs.no_screen) {
    HIP_TRY(ensure_into(B[CB_COLCLASS], 2 * e2, d_colclass));
  }
  HIP_TRY(launch_prof_classify(d_seqs, np, d_a1, d_zero, nullptr, st));
  HIP_TRY(launch_prof_classify(d_seqs + np, np, d_a2, d_zero + np, d_colclass, st));
  if (d_colclass)  // (the zero flags of the reverse strand land on the forward ones again: same row 4)
    HIP_TRY(launch_prof_classify(d_seqs + np, np, d_a2 + rev_base, d_zero + np, d_colclass + rev_base, st));
  if ((trc = timing_end(ctx))) return trc;
  std::vector<uint8_t> hz(2 * (size_t)np);
  HIP_TRY(hipMemcpyAsync(hz.data(), d_zero, hz.size(), hipMemcpyDeviceToHost, st));

  // ---- the gq table (once per context) ----
  if (!ctx->cons_gq_ready) {
    std::vector<uint16_t> tab(kConsMaxPL + 1);
    cons_gq_table(tab.data());
    HIP_TRY(B[CB_GQ].ensure(sizeof(uint16_t) * tab.size()));
    HIP_TRY(hipMemcpyAsync(B[CB_GQ].p, tab.data(), sizeof(uint16_t) * tab.size(), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(ctx_sync(ctx));  // (the classes choose the score bodies; the table upload is complete too)
  ctx->cons_gq_ready = true;

  // ---- plan: pairs by strip height and term count, chunks whose traceback planes + boundary rows fit the workspace ----
  std::vector<int> K(np);
  std::vector<uint32_t> order(np);
  for (uint32_t i = 0; i < np; ++i) {
    K[i] = choose_k(s1.length[i], MODE_PROF);
    order[i] = i;
  }
  auto row4 = [&](uint32_t i) { return hz[i] && hz[np + i]; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    if (K[x] != K[y]) return K[x] > K[y];
    return row4(x) > row4(y);
  });
  std::vector<int> k_sorted(np);  // strip heights in launch order
  for (uint32_t j = 0; j < np; ++j) k_sorted[j] = K[order[j]];
  uint64_t limit;
  if ((rc = workspace_limit(ctx, ctx->dev[DB_BITS].cap + ctx->dev[DB_SCRATCH].cap, &limit))) return rc;
  // descriptors: score pairs (2 per pair, in chunk order) then traceback pairs (1 per pair)
  PairDesc* hsd; HIP_TRY(ensure_into(ctx->pin[PB_DESC], 3 * (size_t)np, hsd));
  PairDesc* htd = hsd + 2 * (size_t)np;
  ChunkCut cut(limit);
  for (uint32_t j = 0; j < np; ++j) {
    const uint32_t i = order[j];
    const uint32_t m = s1.length[i], n = s2.length[i];
    const uint32_t P = num_passes(m, K[i]);
    const uint64_t words = (uint64_t)P * steps_per_pass(n) * 64;
    const uint64_t scr = P > 1 ? 2ull * ((uint64_t)n + 2) : 0;  // one boundary row per strand of the score launch (the traceback reuses the first)
    if (!cut.add(j, words * 8 + scr * 8, words, scr))
      return set_error(TRACYHIP_ERR_OOM, "pair %u needs %llu bytes of traceback planes, workspace limit is %llu", i,
                       (unsigned long long)cut.refused_bytes, (unsigned long long)limit);
    PairDesc d{};
    d.a1_off = s1.offset[i];
    d.a2_off = s2.offset[i];
    d.m = m;
    d.n = n;
    d.a1_stride = m;
    d.a2_stride = n;
    d.flags = row4(i) ? PAIR_ROW4_ZERO : 0u;
    d.scratch_off = cut.scratch_off;
    d.out = 2 * i;
    hsd[2 * (size_t)j] = d;
    d.a2_off = s2.offset[i] + rev_base;
    d.scratch_off = cut.scratch_off + (P > 1 ? (uint64_t)n + 2 : 0);
    d.out = 2 * i + 1;
    hsd[2 * (size_t)j + 1] = d;
    d.a2_off = s2.offset[i];
    d.scratch_off = cut.scratch_off;
    d.bits_off = cut.words_off;
    d.out = i;
    htd[j] = d;
  }
  const std::vector<CutChunk>& chunks = cut.finish();
  uint64_t max_words = 0, max_scr = 0;
  for (const CutChunk& c : chunks) { max_words = std::max(max_words, c.words); max_scr = std::max(max_scr, c.scratch); }
  PairDesc* dsd; HIP_TRY(ensure_into(ctx->dev[DB_DESC], 3 * (size_t)np, dsd));
  HIP_TRY(hipMemcpyAsync(dsd, hsd, sizeof(PairDesc) * 3 * (size_t)np, hipMemcpyHostToDevice, st));
  PairDesc* dtd = dsd + 2 * (size_t)np;
  HIP_TRY(ctx->dev[DB_BITS].ensure(std::max<uint64_t>(max_words * 8, 8)));
  if (max_scr) HIP_TRY(ctx->dev[DB_SCRATCH].ensure(max_scr * 8));
  HIP_TRY(ctx->dev[DB_ERR].ensure(kErrBytes));
  HIP_TRY(hipMemsetAsync(ctx->dev[DB_ERR].p, 0, sizeof(int32_t) * kErrWords, st));
  int32_t* d_sc2; HIP_TRY(ensure_into(B[CB_SC2], 2 * (size_t)np, d_sc2));
  uint8_t* d_ops; HIP_TRY(ensure_into(B[CB_OPS], std::max<uint64_t>(ext, 1), d_ops));
  uint64_t* d_off; HIP_TRY(ensure_into(B[CB_OFF], np, d_off));
  HIP_TRY(ctx->pin[PB_OFF].ensure(sizeof(uint64_t) * (size_t)np));
  std::memcpy(ctx->pin[PB_OFF].p, out->offset, sizeof(uint64_t) * (size_t)np);
  HIP_TRY(hipMemcpyAsync(d_off, ctx->pin[PB_OFF].p, sizeof(uint64_t) * (size_t)np, hipMemcpyHostToDevice, st));

  // per-pair results and payloads: the caller's (MEM_DEVICE) or staged (MEM_HOST)
  int32_t *o_sf = out->score_fwd, *o_sr = out->score_rev, *o_score = out->score, *o_status = out->status;
  uint8_t* o_fwd = out->forward;
  uint32_t *o_na = out->num_aligned, *o_nm = out->num_match, *o_len = out->ops_len, *o_clen = out->cons_len;
  uint8_t *o_r0 = out->rows0, *o_r1 = out->rows1, *o_cons = out->cons;
  uint16_t* o_qual = out->qual;
  if (mem == TRACYHIP_MEM_HOST) {
    const size_t per = 4 * (size_t)np;
    uint8_t* p; HIP_TRY(ensure_into(B[CB_PAIR], 9 * per, p));
    o_sf = reinterpret_cast<int32_t*>(p); o_sr = reinterpret_cast<int32_t*>(p + per); o_score = reinterpret_cast<int32_t*>(p + 2 * per);
    o_status = reinterpret_cast<int32_t*>(p + 3 * per); o_na = reinterpret_cast<uint32_t*>(p + 4 * per); o_nm = reinterpret_cast<uint32_t*>(p + 5 * per);
    o_len = reinterpret_cast<uint32_t*>(p + 6 * per); o_clen = reinterpret_cast<uint32_t*>(p + 7 * per); o_fwd = p + 8 * per;
    const uint64_t ea = (ext + 255) & ~255ull;  // (aligned sub-buffers)
    uint8_t* q; HIP_TRY(ensure_into(B[CB_PAY], 5 * std::max<uint64_t>(ea, 256), q));
    o_r0 = q; o_r1 = q + ea; o_cons = q + 2 * ea; o_qual = reinterpret_cast<uint16_t*>(q + 3 * ea);
  }
  const uint32_t fix_cap = std::max<uint32_t>(65536u, np * 4u);
  HIP_TRY(B[CB_FIX].ensure(sizeof(ConsFixup) * (size_t)fix_cap + 16));
  ConsFixup* d_fix = static_cast<ConsFixup*>(B[CB_FIX].p);
  uint32_t* d_nfix = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(B[CB_FIX].p) + sizeof(ConsFixup) * (size_t)fix_cap);
  HIP_TRY(hipMemsetAsync(d_nfix, 0, sizeof(uint32_t), st));

  DpArgs a = scoring_args(ctx, prm);
  a.a1 = d_a1;
  a.a2 = d_a2;
  a.bits = static_cast<uint64_t*>(ctx->dev[DB_BITS].p);
  a.bits32 = static_cast<uint32_t*>(ctx->dev[DB_BITS].p);
  a.scratch = static_cast<int32_t*>(ctx->dev[DB_SCRATCH].p);
  a.screen = ctx->knobs.no_screen ? 0 : 1;
  a.colcode = d_colclass;
  std::vector<std::pair<uint32_t, int>> narrow_launches;

  ConsArgs ca{};
  ca.a1 = d_a1; ca.a2 = d_a2;
  ca.rows0 = o_r0; ca.rows1 = o_r1;
  ca.off = d_off; ca.len = o_len;
  ca.gq = static_cast<const uint16_t*>(B[CB_GQ].p);
  ca.cons = o_cons; ca.qual = o_qual; ca.cons_len = o_clen;
  ca.num_aligned = o_na; ca.num_match = o_nm; ca.status = o_status;
  ca.fix = d_fix; ca.nfix = d_nfix; ca.fix_cap = fix_cap;
  ca.use_union = job->compute_union ? 1u : 0u;
  ca.use_iupac = job->iupac ? 1u : 0u;
  ca.min_overlap = job->min_overlap;
  ca.match_fraction = (double)job->match_fraction;

  for (const CutChunk& c : chunks) {
    // orientation scores: both strands of every pair of the chunk, one launch per run of equal strip height / term count
    a.scores = d_sc2;
    if ((rc = prof_score_runs(ctx, prm, wide, a, hsd, dsd, k_sorted.data(), c.lo, c.hi, narrow_launches))) return rc;
    const uint32_t cn = c.hi - c.lo;
    if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return trc;
    hipLaunchKernelGGL(cons_decide_kernel, dim3((cn + 255) / 256), dim3(256), 0, st, dtd + c.lo, cn, (const int32_t*)d_sc2, rev_base, o_sf, o_sr, o_fwd);
    HIP_TRY(hipGetLastError());
    if ((trc = timing_end(ctx))) return trc;
    // gotoh(first, chosen strand): traceback planes + walk
    a.scores = o_score;
    if ((rc = prof_trace_runs(ctx, a, htd, dtd, k_sorted.data(), c.lo, c.hi, d_ops, d_off, o_len))) return rc;
    // rows, then the consensus of the chunk
    RowsArgs ra{};
    ra.pairs = dtd + c.lo;
    ra.a1 = d_a1; ra.a2 = d_a2;
    ra.a1_profile = 1; ra.a2_profile = 1;
    ra.ops = d_ops; ra.ops_off = d_off; ra.ops_len = o_len;
    ra.rows0 = o_r0; ra.rows1 = o_r1;
    ra.npairs = cn;
    if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return trc;
    HIP_TRY(launch_alignment_rows(ra, st));
    ca.pairs = dtd + c.lo;
    hipLaunchKernelGGL(consensus_kernel, dim3(cn), dim3(64), 0, st, ca);
    HIP_TRY(hipGetLastError());
    if ((trc = timing_end(ctx))) return trc;
  }

  // ---- one synchronisation: error words, fix-up count, results (MEM_HOST) ----
  int32_t herr[kErrWords] = {};
  uint32_t nfix = 0;
  HIP_TRY(hipMemcpyAsync(herr, ctx->dev[DB_ERR].p, sizeof(herr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&nfix, d_nfix, sizeof(nfix), hipMemcpyDeviceToHost, st));
  if (mem == TRACYHIP_MEM_HOST) {
    const size_t n4 = 4 * (size_t)np;
    HIP_TRY(hipMemcpyAsync(out->score_fwd, o_sf, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->score_rev, o_sr, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->score, o_score, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->status, o_status, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->num_aligned, o_na, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->num_match, o_nm, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->ops_len, o_len, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->cons_len, o_clen, n4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->forward, o_fwd, (size_t)np, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->rows0, o_r0, ext, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->rows1, o_r1, ext, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->cons, o_cons, ext, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->qual, o_qual, 2 * ext, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx_sync(ctx));
  timing_collect(ctx);
  const int verdict = range_verdict(prm, herr, narrow_launches, max_mn, kTagShift);
  if (verdict == kWiden) return kWiden;  // a 16-bit score launch met an un-normalised profile: the caller repeats on int32
  if (verdict != TRACYHIP_OK) return verdict;
  ctx->stats.cons_chunks = (uint32_t)chunks.size();

  // ---- fix-ups: the screened columns by the host gtLetter ----
  if (nfix > fix_cap) {  // more than the list holds: run the consensus kernel again with a list that does
    HIP_TRY(B[CB_FIX].ensure(sizeof(ConsFixup) * (size_t)nfix + 16));
    ca.fix = static_cast<ConsFixup*>(B[CB_FIX].p);
    ca.nfix = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(B[CB_FIX].p) + sizeof(ConsFixup) * (size_t)nfix);
    ca.fix_cap = nfix;
    HIP_TRY(hipMemsetAsync(ca.nfix, 0, sizeof(uint32_t), st));
    for (const CutChunk& c : chunks) {
      ca.pairs = dtd + c.lo;
      hipLaunchKernelGGL(consensus_kernel, dim3(c.hi - c.lo), dim3(64), 0, st, ca);
      HIP_TRY(hipGetLastError());
    }
    if (mem == TRACYHIP_MEM_HOST) {
      HIP_TRY(hipMemcpyAsync(out->cons, o_cons, ext, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(out->qual, o_qual, 2 * ext, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx_sync(ctx));
    d_fix = ca.fix;
  }
  ctx->stats.cons_fixup_columns = nfix;
  if (nfix == 0) return TRACYHIP_OK;
  std::vector<ConsFixup> hf(nfix);
  HIP_TRY(hipMemcpy(hf.data(), d_fix, sizeof(ConsFixup) * (size_t)nfix, hipMemcpyDeviceToHost));
  tracy_amd::ConsensusOptions co;
  co.useIUPAC = job->iupac != 0;
  std::vector<ConsPatch> patch(nfix);
  for (uint32_t w = 0; w < nfix; ++w) {
    double cl[6];
    for (int k = 0; k < 6; ++k) cl[k] = (double)hf[w].cl[k];
    std::string letter;
    std::vector<uint32_t> q;
    tracy_amd::gtLetter(co, cl, letter, q);
    patch[w] = ConsPatch{hf[w].slot, (uint32_t)(uint8_t)letter[0], q[0]};
  }
  if (mem == TRACYHIP_MEM_HOST) {
    for (const ConsPatch& p : patch) { out->cons[p.slot] = (uint8_t)p.letter; out->qual[p.slot] = (uint16_t)p.qual; }
    return TRACYHIP_OK;
  }
  HIP_TRY(B[CB_PATCH].ensure(sizeof(ConsPatch) * patch.size()));
  HIP_TRY(hipMemcpyAsync(B[CB_PATCH].p, patch.data(), sizeof(ConsPatch) * patch.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(cons_patch_kernel, dim3((nfix + 255) / 256), dim3(256), 0, st, static_cast<const ConsPatch*>(B[CB_PATCH].p), nfix, o_cons, o_qual);
  HIP_TRY(hipGetLastError());
  HIP_TRY(ctx_sync(ctx));
  return TRACYHIP_OK;
}

}  // namespace

extern "C" {

int tracyhip_consensus_traces(tracyhip_ctx* ctx, const tracyhip_consensus_job* job, const tracyhip_params* prm, int mem,
                              const tracyhip_consensus_result* out) {
  int rc = ctx_begin(ctx);
  if (rc) return rc;
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return set_error(TRACYHIP_ERR_ARG, "bad mem kind");
  if (!job || !out) return set_error(TRACYHIP_ERR_ARG, "null job / result");
  if (!prm) return set_error(TRACYHIP_ERR_ARG, "null params");
  ctx->stats = tracyhip_call_stats{};
  ctx->stats.traces = job->npairs;
  ctx->stats.stream_ordered = 1;
  const uint32_t np = job->npairs;
  if (np == 0) return check_params(prm, 0);
  if (!check_profiles(job->first, np, "first") || !check_profiles(job->second, np, "second")) return TRACYHIP_ERR_ARG;
  if (!out->score_fwd || !out->score_rev || !out->forward || !out->score || !out->num_aligned || !out->num_match || !out->status ||
      !out->rows0 || !out->rows1 || !out->ops_len || !out->cons || !out->qual || !out->cons_len || !out->offset)
    return set_error(TRACYHIP_ERR_ARG, "null result arrays");
  rc = consensus_run(ctx, job, prm, mem, out, false);
  if (rc == kWiden) rc = consensus_run(ctx, job, prm, mem, out, true);
  return rc;
}

int tracyhip_consensus_traces_async(tracyhip_ctx* ctx, const tracyhip_consensus_job* job, const tracyhip_params* prm, int mem,
                                    const tracyhip_consensus_result* out) {
  if (!ctx || !job || !prm || !out) return set_error(TRACYHIP_ERR_ARG, "null context / job / params / result");
  const tracyhip_consensus_job j = *job;
  const tracyhip_params q = *prm;
  const tracyhip_consensus_result o = *out;
  return async_submit(ctx, [=]() { return tracyhip_consensus_traces(ctx, &j, &q, mem, &o); });
}

}  // extern "C"
