// assemble.hip -- tracyhip_assemble_traces: the reference-guided chain of `tracy assemble` (assemble.h:219-288) for a batch of groups.
//
// Per group: revcomp of every trace on the device (profile.h:74-90, prof_batch.hip); gotohScore of both strands against the group's
// reference in ONE profile x profile score launch for the whole batch (the launch loops are prof_batch.hip's); the matching traces,
// their strands and their order on the host (bookkeeping, as UPGMA is in msa.hpp); then the chain, STEP-BATCHED: step k of every
// group of a chunk that has more than k matching traces is one batch -- msa_profile of the rows so far (written at the end of step
// k - 1), gotoh(trace_k, that profile) through the traceback kernels of tracyhip_gotoh_align (fused walk), msa_merge with the trace
// as row 0.  Step 0 is gotoh(best, reference): both sides of its merge are input profiles, shown as their _profileConsChar rows.
// msa_consensus closes a chunk.  The three row-block kernels are msa_batch.hip's, shared with denovo.hip, and so is the host code
// around them (GroupOut, TraceBatch, msa_merge_batch, msa_consensus_batch, prof_score_stage); what stays here is the chain's own
// plan: who matches, in which order, which groups share a chunk, what step k of a group aligns against.
//
// The columns of step k are the op count of step k - 1, which only the device knows: the host reads the op counts back once per step
// and builds the next step's descriptors from them.  Workspaces are sized from the bound  columns <= n_ref + sum of the trace lengths
// (every step adds at most its trace's length), which is also the capacity the caller provides per group.
// Host synchronisations: classes, scores, one per chain step of a chunk, one at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "assemble_wave.h"
#include "capi_internal.h"
#include "launch.h"

using namespace tracyhip;

namespace {

int assemble_validate(const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem, const tracyhip_assemble_result* out) {
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return set_error(TRACYHIP_ERR_ARG, "bad mem kind");
  if (!job || !out) return set_error(TRACYHIP_ERR_ARG, "null job / result");
  if (!prm) return set_error(TRACYHIP_ERR_ARG, "null params");
  if (std::isnan(job->match_fraction)) return set_error(TRACYHIP_ERR_ARG, "match_fraction is not a number");
  if (std::isnan(job->fraction_called)) return set_error(TRACYHIP_ERR_ARG, "fraction_called is not a number");
  const uint32_t ng = job->ngroups;
  if (ng == 0) return TRACYHIP_OK;
  if (!job->group_first) return set_error(TRACYHIP_ERR_ARG, "null group_first");
  if (!check_profile_set(job->traces, "traces") || !check_profile_set(job->references, "references")) return TRACYHIP_ERR_ARG;
  if (!out->score_fwd || !out->score_rev || !out->forward || !out->rank || !out->nrows || !out->ncol || !out->rows || !out->gapped ||
      !out->cons || !out->qual || !out->cons_len || !out->rows_offset || !out->col_offset)
    return set_error(TRACYHIP_ERR_ARG, "null result arrays");
  for (uint32_t g = 0; g < ng; ++g) {
    if (job->group_first[g + 1] < job->group_first[g]) return set_error(TRACYHIP_ERR_ARG, "group_first decreases at group %u", g);
    if (job->group_first[g + 1] > job->traces.count)
      return set_error(TRACYHIP_ERR_ARG, "group %u ends at trace %u, the set holds %u", g, job->group_first[g + 1], job->traces.count);
    const uint32_t r = job->ref_index ? job->ref_index[g] : g;
    if (r >= job->references.count) return set_error(TRACYHIP_ERR_ARG, "group %u: reference %u of %u", g, r, job->references.count);
    if (!check_profile_columns(job->references, "references", r, r + 1)) return TRACYHIP_ERR_ARG;
  }
  if (!check_profile_columns(job->traces, "traces", job->group_first[0], job->group_first[ng])) return TRACYHIP_ERR_ARG;
  return TRACYHIP_OK;
}

struct Match { int32_t score; uint32_t idx; bool forward; };  // TraceScore (assemble.h:32-41)

int assemble_run(tracyhip_ctx* ctx, const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem, const tracyhip_assemble_result* out,
                 bool wide) {
  const uint32_t ng = job->ngroups;
  const uint32_t* gf = job->group_first;
  const uint32_t t0 = gf[0], nt = gf[ng] - gf[0];
  hipStream_t st = ctx->stream;
  const tracyhip_seqset& sT = job->traces;
  const tracyhip_seqset& sR = job->references;
  DevBuf* const B = ctx->dev;  // indexed by the AB_* roles (capi_internal.h)
  auto ref_of = [&](uint32_t g) { return job->ref_index ? job->ref_index[g] : g; };

  // ---- geometry: the column bound of every group and where its pieces live in the call's own buffers ----
  std::vector<uint64_t> bound(ng), cg(ng + 1, 0), rg(ng + 1, 0), sg(ng + 1, 0);  // columns; prefix sums of columns, row bytes, span pairs
  std::vector<uint32_t> grp(nt);  // trace to group
  uint64_t eT = 0, eR = 0, max_mn = 0, ext_rows = 0, ext_col = 0;
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t r = ref_of(g);
    uint64_t b = sR.length[r];
    eR = std::max<uint64_t>(eR, sR.offset[r] + 6ull * sR.length[r]);
    for (uint32_t i = gf[g]; i < gf[g + 1]; ++i) {
      grp[i - t0] = g;
      b += sT.length[i];
      eT = std::max<uint64_t>(eT, sT.offset[i] + 6ull * sT.length[i]);
    }
    const uint64_t K = gf[g + 1] - gf[g];
    bound[g] = b;
    cg[g + 1] = cg[g] + b;
    rg[g + 1] = rg[g] + (K + 1) * b;
    sg[g + 1] = sg[g] + (K + 1);
    max_mn = std::max(max_mn, b);
    if (K) {
      ext_rows = std::max(ext_rows, out->rows_offset[g] + (K + 1) * b);
      ext_col = std::max(ext_col, out->col_offset[g] + b);
    }
  }
  int rc;
  if ((rc = check_params(prm, max_mn))) return rc;
  if (max_mn > 0xffffffffull) return set_error(TRACYHIP_ERR_RANGE, "a group's column bound exceeds 2^32");
  GroupOut go(ng, *out);
  if (nt == 0) return go.clear_counts(ctx, mem);  // groups without traces: nrows 0 everywhere

  // ---- inputs: traces = [forward | revcomp] in one buffer, references where the caller has them (or staged) ----
  float* d_tr; HIP_TRY(ensure_into(B[AB_TR], 2 * eT, d_tr));
  HIP_TRY(hipMemcpyAsync(d_tr, sT.data, eT * 4, mem == TRACYHIP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  const uint64_t rev_base = eT;
  const void* d_refv = nullptr;
  if ((rc = stage_in(ctx, ctx->dev[DB_IN2], sR.data, eR * 4, mem, &d_refv))) return rc;
  const float* d_ref = static_cast<const float*>(d_refv);
  const uint32_t nref = sR.count;
  std::vector<ProfSeq> hs((size_t)nt + nref, ProfSeq{0, 0, 0});  // (references no group uses keep length 0: nothing of them is read)
  for (uint32_t i = 0; i < nt; ++i) hs[i] = ProfSeq{sT.offset[t0 + i], sT.length[t0 + i], 0};
  for (uint32_t g = 0; g < ng; ++g) hs[(size_t)nt + ref_of(g)] = ProfSeq{sR.offset[ref_of(g)], sR.length[ref_of(g)], 0};
  ProfSeq* d_seqs; HIP_TRY(ensure_into(B[AB_SEQS], hs.size(), d_seqs));
  HIP_TRY(hipMemcpyAsync(d_seqs, hs.data(), sizeof(ProfSeq) * hs.size(), hipMemcpyHostToDevice, st));
  int trc;
  if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 2 * 4ull * eT))) return trc;
  HIP_TRY(launch_prof_revcomp(d_seqs, nt, d_tr, d_tr, rev_base, st));
  uint8_t* d_zero; HIP_TRY(ensure_into(B[AB_CLASS], (size_t)nt + nref, d_zero));
  uint8_t* d_refclass = nullptr;
  const bool screen = !ctx->knobs.no_screen;
  if (screen) HIP_TRY(ensure_into(B[AB_REFCLASS], std::max<uint64_t>(eR, 1), d_refclass));
  HIP_TRY(launch_prof_classify(d_seqs, nt, d_tr, d_zero, nullptr, st));
  HIP_TRY(launch_prof_classify(d_seqs + nt, nref, d_ref, d_zero + nt, d_refclass, st));
  if ((trc = timing_end(ctx))) return trc;
  std::vector<uint8_t> hz((size_t)nt + nref);
  HIP_TRY(hipMemcpyAsync(hz.data(), d_zero, hz.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx_sync(ctx));  // (the classes choose the score bodies)

  uint64_t limit;
  if ((rc = workspace_limit(ctx, ctx->dev[DB_BITS].cap + ctx->dev[DB_SCRATCH].cap, &limit))) return rc;

  // ---- both strand scores of every trace: one launch per run of equal strip height / term count ----
  std::vector<int> KS(nt);
  for (uint32_t i = 0; i < nt; ++i) KS[i] = choose_k(sT.length[t0 + i], MODE_PROF);
  auto row4 = [&](uint32_t i) { return hz[i] && hz[(size_t)nt + ref_of(grp[i])]; };
  std::vector<uint32_t> order(nt);
  for (uint32_t i = 0; i < nt; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
    if (KS[x] != KS[y]) return KS[x] > KS[y];
    return row4(x) > row4(y);
  });
  std::vector<int> k_score(nt);  // strip heights of the score launches, in launch order
  for (uint32_t j = 0; j < nt; ++j) k_score[j] = KS[order[j]];
  const size_t ndesc = std::max<size_t>(2 * (size_t)nt, ng);
  PairDesc *hd, *dd;
  HIP_TRY(ensure_into(ctx->pin[PB_DESC], ndesc, hd));
  HIP_TRY(ensure_into(ctx->dev[DB_DESC], ndesc, dd));
  uint64_t sc_scratch = 0;
  for (uint32_t j = 0; j < nt; ++j) {
    const uint32_t i = order[j], r = ref_of(grp[i]);
    const uint32_t m = sT.length[t0 + i], n = sR.length[r];
    const uint32_t P = num_passes(m, KS[i]);
    PairDesc d = prof_pair_desc(sT.offset[t0 + i], m, sR.offset[r], n, row4(i));
    for (uint32_t s = 0; s < 2; ++s) {
      d.a1_off = sT.offset[t0 + i] + (s ? rev_base : 0);
      d.scratch_off = sc_scratch;
      d.out = 2 * i + s;
      hd[2 * (size_t)j + s] = d;
      if (P > 1) sc_scratch += (uint64_t)n + 2;
    }
  }
  if (sc_scratch * 8 > limit)
    return set_error(TRACYHIP_ERR_OOM, "the strand scores need %llu bytes of boundary rows, workspace limit is %llu", (unsigned long long)(sc_scratch * 8),
                     (unsigned long long)limit);
  HIP_TRY(hipMemcpyAsync(dd, hd, sizeof(PairDesc) * 2 * (size_t)nt, hipMemcpyHostToDevice, st));
  if (sc_scratch) HIP_TRY(ctx->dev[DB_SCRATCH].ensure(sc_scratch * 8));
  int32_t* d_sc2; HIP_TRY(ensure_into(B[AB_SC2], 2 * (size_t)nt, d_sc2));

  DpArgs a = scoring_args(ctx, prm);
  a.a1 = d_tr;
  a.a2 = d_ref;
  a.scratch = static_cast<int32_t*>(ctx->dev[DB_SCRATCH].p);
  a.screen = screen ? 1 : 0;
  a.colcode = d_refclass;
  a.scores = d_sc2;
  std::vector<std::pair<uint32_t, int>> narrow_launches;
  std::vector<int32_t> sc2(2 * (size_t)nt);
  if ((rc = prof_score_stage(ctx, prm, wide, a, hd, dd, k_score.data(), nt, sc2.data(), sc2.size(), max_mn, narrow_launches))) return rc;

  // ---- which traces match, their strands, their order (assemble.h:228-247) ----
  std::vector<int32_t> h_sf(nt), h_sr(nt);
  std::vector<uint8_t> h_fwd(nt);
  std::vector<uint32_t> h_rank(nt, 0xffffffffu), h_nrows(ng, 0), h_ncol(ng, 0);
  std::vector<std::vector<Match>> matched(ng);
  for (uint32_t i = 0; i < nt; ++i) {
    const int32_t gsFwd = sc2[2 * (size_t)i], gsRev = sc2[2 * (size_t)i + 1];
    h_sf[i] = gsFwd; h_sr[i] = gsRev;
    h_fwd[i] = gsFwd >= gsRev ? 1 : 0;
    const double seqsize = (double)sT.length[t0 + i];
    const double thr = seqsize * job->match_fraction * prm->match + seqsize * (1 - job->match_fraction) * prm->mismatch;
    if (gsFwd > thr || gsRev > thr) matched[grp[i]].push_back(Match{std::max(gsFwd, gsRev), i, gsFwd >= gsRev});
  }
  for (uint32_t g = 0; g < ng; ++g) {
    std::vector<Match>& v = matched[g];
    std::sort(v.begin(), v.end(), [](const Match& x, const Match& y) { return x.score > y.score || (x.score == y.score && x.idx < y.idx); });
    for (size_t k = 0; k < v.size(); ++k) h_rank[v[k].idx] = (uint32_t)k;
    h_nrows[g] = v.empty() ? 0u : (uint32_t)v.size() + 1u;
  }

  // ---- chunks of groups: the traceback planes (and boundary rows) of a step of all its groups fit the workspace ----
  ChunkCut cut(limit);
  std::vector<uint32_t> chunk_steps(1, 0);  // per chunk: the most matches of one of its groups
  for (uint32_t g = 0; g < ng; ++g) {
    if (matched[g].empty()) { cut.ride(g); continue; }
    uint64_t words = 0, scr = 0;
    for (const Match& mt : matched[g]) {
      const uint32_t m = sT.length[t0 + mt.idx];
      const uint32_t P = num_passes(m, KS[mt.idx]);
      words = std::max(words, (uint64_t)P * steps_per_pass((uint32_t)bound[g]) * 64);
      if (P > 1) scr = bound[g] + 2;
    }
    if (!cut.add(g, words * 8 + scr * 8, words, scr))
      return set_error(TRACYHIP_ERR_OOM, "group %u needs %llu bytes of traceback planes, workspace limit is %llu", g,
                       (unsigned long long)cut.refused_bytes, (unsigned long long)limit);
    chunk_steps.resize(cut.chunks.size() + 1, 0);
    chunk_steps.back() = std::max<uint32_t>(chunk_steps.back(), (uint32_t)matched[g].size());
  }
  const std::vector<CutChunk>& chunks = cut.finish();
  uint64_t max_words = 0, max_scr = sc_scratch;
  for (const CutChunk& c : chunks) { max_words = std::max(max_words, c.words); max_scr = std::max(max_scr, c.scratch); }
  HIP_TRY(ctx->dev[DB_BITS].ensure(std::max<uint64_t>(max_words * 8, 8)));
  if (max_scr) HIP_TRY(ctx->dev[DB_SCRATCH].ensure(max_scr * 8));

  // ---- the call's own buffers: ops, their offsets / counts, two row blocks, spans, the profile of the rows and its classes ----
  const uint64_t ncols = std::max<uint64_t>(cg[ng], 1), nrowb = std::max<uint64_t>(rg[ng], 1);
  uint8_t *d_ops, *d_w[2], *d_pclass;
  uint32_t* d_len;
  int32_t* d_span;
  float* d_prof;
  HIP_TRY(ensure_into(B[AB_OPS], ncols, d_ops));
  HIP_TRY(B[AB_OFF].ensure(sizeof(uint64_t) * (size_t)ng));
  HIP_TRY(ensure_into(B[AB_LEN], ng, d_len));
  HIP_TRY(ensure_into(B[AB_W0], nrowb, d_w[0]));
  HIP_TRY(ensure_into(B[AB_W1], nrowb, d_w[1]));
  HIP_TRY(ensure_into(B[AB_SPAN], 2 * (size_t)sg[ng], d_span));
  HIP_TRY(ensure_into(B[AB_PROF], 6 * ncols, d_prof));
  HIP_TRY(ensure_into(B[AB_PCLASS], 6 * ncols, d_pclass));
  HIP_TRY(B[AB_STEP].ensure((sizeof(AsmStep) + sizeof(AsmFinal)) * (size_t)ng));
  AsmStep* d_step = static_cast<AsmStep*>(B[AB_STEP].p);
  AsmFinal* d_fin = reinterpret_cast<AsmFinal*>(d_step + ng);
  HIP_TRY(ctx->pin[PB_OFF].ensure(sizeof(uint64_t) * (size_t)ng));
  std::memcpy(ctx->pin[PB_OFF].p, cg.data(), sizeof(uint64_t) * (size_t)ng);
  HIP_TRY(hipMemcpyAsync(B[AB_OFF].p, ctx->pin[PB_OFF].p, sizeof(uint64_t) * (size_t)ng, hipMemcpyHostToDevice, st));
  const uint64_t* d_off = static_cast<const uint64_t*>(B[AB_OFF].p);
  HIP_TRY(hipMemsetAsync(d_len, 0, sizeof(uint32_t) * (size_t)ng, st));
  HIP_TRY(ctx->pin[PB_TMP].ensure((sizeof(AsmStep) + sizeof(AsmFinal)) * (size_t)ng));
  AsmStep* h_step = static_cast<AsmStep*>(ctx->pin[PB_TMP].p);
  AsmFinal* h_fin = reinterpret_cast<AsmFinal*>(h_step + ng);
  uint32_t* h_len; HIP_TRY(ensure_into(ctx->pin[PB_RES], (size_t)ng, h_len));

  if ((rc = go.bind(ctx, mem, ext_rows, ext_col))) return rc;

  a.scores = nullptr;
  const int32_t ignore_last = job->include_reference ? 0 : 1;
  uint32_t total_steps = 0;
  std::vector<uint32_t> act;
  TraceBatch tb{hd, dd, d_ops, d_off, d_len, limit};  // (the planes above hold every step of every chunk: its upload grows nothing)

  for (const CutChunk& c : chunks) {
    for (uint32_t k = 0, steps = chunk_steps[&c - chunks.data()]; k < steps; ++k) {
      // the groups with a trace of rank k, by strip height and term count (one launch per run)
      act.clear();
      for (uint32_t g = c.lo; g < c.hi; ++g)
        if (matched[g].size() > k) act.push_back(g);
      auto flags_of = [&](uint32_t g) { return (k == 0 && row4(matched[g][0].idx)) ? (uint32_t)PAIR_ROW4_ZERO : 0u; };
      std::stable_sort(act.begin(), act.end(), [&](uint32_t x, uint32_t y) {
        const int kx = KS[matched[x][k].idx], ky = KS[matched[y][k].idx];
        if (kx != ky) return kx > ky;
        return flags_of(x) > flags_of(y);
      });
      const uint32_t na = (uint32_t)act.size();
      tb.clear();
      for (uint32_t j = 0; j < na; ++j) {
        const uint32_t g = act[j];
        const Match& mt = matched[g][k];
        const uint32_t r = ref_of(g);
        const uint32_t m = sT.length[t0 + mt.idx];
        const uint32_t n = k == 0 ? sR.length[r] : h_ncol[g];
        const bool last = k + 1 == (uint32_t)matched[g].size();
        const uint64_t a1_off = sT.offset[t0 + mt.idx] + (mt.forward ? 0 : rev_base), a2_off = k == 0 ? sR.offset[r] : 6 * cg[g];
        tb.add(a1_off, m, a2_off, n, flags_of(g) != 0, KS[mt.idx], g);
        AsmStep s{};
        s.left = MsaSide{nullptr, d_tr + a1_off, 1u, m, m};
        if (k == 0) s.right = MsaSide{nullptr, d_ref + a2_off, 1u, n, n};
        else s.right = MsaSide{d_w[(k - 1) & 1] + rg[g], nullptr, k + 1, n, 0u};
        s.ops_off = cg[g];
        s.slot = g;
        s.cap = m + n;
        s.dst = last ? go.d_rows + go.rows_offset[g] : d_w[k & 1] + rg[g];
        s.span = d_span + 2 * sg[g];
        s.prof = last ? nullptr : d_prof + 6 * cg[g];
        s.colclass = d_pclass + 6 * cg[g];
        h_step[j] = s;
      }
      a.a2 = k == 0 ? (const void*)d_ref : (const void*)d_prof;
      a.colcode = !screen ? nullptr : k == 0 ? d_refclass : d_pclass;
      // the op counts: the columns of the next step (and the group's ncol)
      if ((rc = msa_merge_batch(ctx, a, tb, h_step, d_step, h_len, 0, ng))) return rc;
      for (uint32_t j = 0; j < na; ++j) {
        const uint32_t g = act[j];
        if (h_len[g] > h_step[j].cap)
          return set_error(TRACYHIP_ERR_RANGE, "group %u, step %u: the traceback gave %u ops for %u rows and columns", g, k, h_len[g], h_step[j].cap);
        h_ncol[g] = h_len[g];
      }
      ++total_steps;
    }
    // msa_consensus of the chunk's groups
    uint32_t nf = 0;
    for (uint32_t g = c.lo; g < c.hi; ++g) {
      if (matched[g].empty()) continue;
      const uint32_t rows = (uint32_t)matched[g].size() + 1 - ignore_last;
      h_fin[nf++] = go.final_entry(g, d_span + 2 * sg[g], rows, g, (uint32_t)bound[g], job->fraction_called);
    }
    // (h_fin is filled again at the end of the next chunk that has groups to finish: behind the synchronisations of its steps)
    if ((rc = msa_consensus_batch(ctx, h_fin, d_fin, nf, d_len))) return rc;
  }

  // ---- the last synchronisation: error words, results ----
  int32_t herr[kErrWords] = {};
  HIP_TRY(hipMemcpyAsync(herr, ctx->dev[DB_ERR].p, sizeof(herr), hipMemcpyDeviceToHost, st));
  if ((rc = put_result(ctx, mem, out->score_fwd + t0, h_sf.data(), 4 * (size_t)nt)) ||
      (rc = put_result(ctx, mem, out->score_rev + t0, h_sr.data(), 4 * (size_t)nt)) ||
      (rc = put_result(ctx, mem, out->forward + t0, h_fwd.data(), (size_t)nt)) ||
      (rc = put_result(ctx, mem, out->rank + t0, h_rank.data(), 4 * (size_t)nt)) ||
      (rc = go.copy_back(ctx, mem, h_nrows.data(), h_ncol.data())))
    return rc;
  HIP_TRY(ctx_sync(ctx));
  timing_collect(ctx);
  ctx->stats.asm_chunks = (uint32_t)chunks.size();
  ctx->stats.asm_steps = total_steps;
  return range_verdict(prm, herr, narrow_launches, max_mn, kTagShift);
}

}  // namespace

extern "C" {

int tracyhip_assemble_validate(const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem, const tracyhip_assemble_result* out) {
  return assemble_validate(job, prm, mem, out);
}

int tracyhip_assemble_traces(tracyhip_ctx* ctx, const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem,
                             const tracyhip_assemble_result* out) {
  int rc = assemble_validate(job, prm, mem, out);  // (before any device is touched)
  if (rc) return rc;
  if ((rc = ctx_begin(ctx))) return rc;
  ctx->stats = tracyhip_call_stats{};
  ctx->stats.traces = job->ngroups ? job->group_first[job->ngroups] - job->group_first[0] : 0;
  ctx->stats.stream_ordered = 1;
  if (job->ngroups == 0) return check_params(prm, 0);
  rc = assemble_run(ctx, job, prm, mem, out, false);
  if (rc == kWiden) rc = assemble_run(ctx, job, prm, mem, out, true);
  return rc;
}

int tracyhip_assemble_traces_async(tracyhip_ctx* ctx, const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem,
                                   const tracyhip_assemble_result* out) {
  if (!ctx || !job || !prm || !out) return set_error(TRACYHIP_ERR_ARG, "null context / job / params / result");
  const tracyhip_assemble_job j = *job;
  const tracyhip_params q = *prm;
  const tracyhip_assemble_result o = *out;
  return async_submit(ctx, [=]() { return tracyhip_assemble_traces(ctx, &j, &q, mem, &o); });
}

}  // extern "C"
