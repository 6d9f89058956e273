// denovo.hip -- tracyhip_denovo_traces: de novo `tracy assemble` (assemble.h:378-471 -> msa.h) for a batch of groups, the per-group
// host path of tracy_amd/host/msa.hpp / assemble_cli.inc restated as one device pipeline.
//
// Per call: revcomp and classes of every trace (prof_batch.hip); the strand table T[i][j][oi][oj] of every group in ONE family of score
// launches; revSeqBasedOnDist on the host from the table (denovo_plan.h).  Then per chunk of groups: the overlap test in rounds (every
// undecided trace against its next partner, traceback through prof_trace_runs, the 's' ops counted by one wave each, the verdict on
// the host); UPGMA on the host from the table; the merges STEP-BATCHED by tree height -- gotoh(left, right), msa_merge with the left
// rows first, msa_profile of every node below the root (msa_batch.hip) -- and msa_consensus.
//
// Both sides of every dynamic program live in one float buffer: [forward | revcomp] of the inputs, then the node profiles; the column
// classes of the screened score form are indexed like it.  A leaf is its input profile in the DP and its _profileConsChar row in the
// merge.  The columns of a node are the op count of its merge, which only the device knows: the host reads the op counts back once
// per height.  Workspaces are sized from  columns of a node <= the summed lengths of its leaves.
// Host synchronisations: classes, table, one per overlap round and one per tree height of a chunk, one at the end.
// The host code both group calls run around the kernels is msa_batch.hip's, shared with assemble.hip (GroupOut, TraceBatch,
// msa_merge_batch, msa_consensus_batch, prof_score_stage); what stays here is the plan: strands, overlap verdicts, trees, chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "assemble_wave.h"
#include "capi_internal.h"
#include "denovo_plan.h"
#include "dev_wave.h"

using namespace tracyhip;

namespace {

// numAligned of every alignment of an overlap round: one wave per pair, cnt[PairDesc::out]
__global__ __launch_bounds__(64) void denovo_count_kernel(const PairDesc* __restrict__ pairs, const uint8_t* __restrict__ ops, const uint64_t* __restrict__ ops_off,
                                                          const uint32_t* __restrict__ ops_len, uint32_t* __restrict__ cnt) {
  const PairDesc d = pairs[blockIdx.x];
  const uint32_t L = ops_len[d.out];
  if (L > d.m + d.n) return;  // (the walk left the matrix: the host sees the length and reports it)
  MsaDevWave w;
  const uint32_t n = msa_count_aligned_wave(w, ops + ops_off[d.out], L);
  if (threadIdx.x == 0) cnt[d.out] = n;
}

int denovo_validate(const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem, const tracyhip_denovo_result* out) {
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return set_error(TRACYHIP_ERR_ARG, "bad mem kind");
  if (!job || !out) return set_error(TRACYHIP_ERR_ARG, "null job / result");
  if (!prm) return set_error(TRACYHIP_ERR_ARG, "null params");
  if (std::isnan(job->match_fraction)) return set_error(TRACYHIP_ERR_ARG, "match_fraction is not a number");
  if (std::isnan(job->fraction_called)) return set_error(TRACYHIP_ERR_ARG, "fraction_called is not a number");
  const uint32_t ng = job->ngroups;
  if (ng == 0) return TRACYHIP_OK;
  if (!job->group_first) return set_error(TRACYHIP_ERR_ARG, "null group_first");
  if (!check_profile_set(job->traces, "traces")) return TRACYHIP_ERR_ARG;
  if (!out->forward || !out->partner || !out->row || !out->nrows || !out->ncol || !out->rows || !out->gapped || !out->cons || !out->qual ||
      !out->cons_len || !out->rows_offset || !out->col_offset)
    return set_error(TRACYHIP_ERR_ARG, "null result arrays");
  for (uint32_t g = 0; g < ng; ++g) {
    if (job->group_first[g + 1] < job->group_first[g]) return set_error(TRACYHIP_ERR_ARG, "group_first decreases at group %u", g);
    if (job->group_first[g + 1] > job->traces.count)
      return set_error(TRACYHIP_ERR_ARG, "group %u ends at trace %u, the set holds %u", g, job->group_first[g + 1], job->traces.count);
  }
  if (!check_profile_columns(job->traces, "traces", job->group_first[0], job->group_first[ng])) return TRACYHIP_ERR_ARG;
  return TRACYHIP_OK;
}

// a leaf or a node of a group's tree: where its profile and its rows are
struct TreeNode {
  uint32_t n = 0, cap = 0, ncol = 0;  // rows; the bound of its columns; its columns (a node: known after its height)
  uint64_t prof_off = 0;              // floats into DN_PROF (the root of a tree has no profile)
  uint64_t rows_off = 0, span_off = 0, ops_off = 0;  // a node: bytes into DN_ROWS, rows into DN_SPAN, bytes into DN_OPS
  uint32_t slot = 0;                  // a node: its entry of the op offsets / lengths
  bool row4_zero = false;             // a leaf: row 4 of the input profile is zero
};

struct GroupPlan {
  std::vector<uint32_t> keep;  // the traces that passed the overlap test, by index within the group
  DenovoTree tree;
  std::vector<TreeNode> node;
};

int denovo_run(tracyhip_ctx* ctx, const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem, const tracyhip_denovo_result* out, bool wide) {
  const uint32_t ng = job->ngroups;
  const uint32_t* gf = job->group_first;
  const uint32_t t0 = gf[0], nt = gf[ng] - gf[0];
  hipStream_t st = ctx->stream;
  const tracyhip_seqset& sT = job->traces;
  DevBuf* const B = ctx->dev;  // indexed by the DN_* roles (capi_internal.h)
  auto len_of = [&](uint32_t i) { return sT.length[t0 + i]; };  // i: trace index within the call
  // wall time of the stages, each of which ends in a synchronisation (option `verbose`: one line on stderr)
  double stage_ms[5] = {0, 0, 0, 0, 0};  // inputs, table, rounds, tree, consensus + results
  auto clock_now = [] { return std::chrono::steady_clock::now(); };
  auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(clock_now() - t).count(); };
  auto t_stage = clock_now();

  // ---- geometry: per group the summed length S (the column bound of every node), and where its pieces live ----
  std::vector<uint64_t> S(ng), maxlen(ng, 0), tb(ng + 1, 0), ob(ng + 1, 0), pb(ng + 1, 0), sb(ng + 1, 0);
  std::vector<uint32_t> grp(nt);  // trace to group
  uint64_t eT = 0, max_mn = 0, ext_rows = 0, ext_col = 0;
  for (uint32_t g = 0; g < ng; ++g) {
    const uint64_t K = gf[g + 1] - gf[g];
    uint64_t s = 0;
    for (uint32_t i = gf[g]; i < gf[g + 1]; ++i) {
      grp[i - t0] = g;
      s += sT.length[i];
      maxlen[g] = std::max<uint64_t>(maxlen[g], sT.length[i]);
      eT = std::max<uint64_t>(eT, sT.offset[i] + 6ull * sT.length[i]);
    }
    S[g] = s;
    tb[g + 1] = tb[g] + denovo_table_size((uint32_t)K);              // table entries
    ob[g + 1] = ob[g] + std::max(s + K * maxlen[g], K * s);          // op bytes: a round has len_i + maxlen per trace, a tree at most S per node
    pb[g + 1] = pb[g] + (K > 2 ? (K - 2) * s : 0);                   // node profile columns: at most K - 2 nodes below the root
    sb[g + 1] = sb[g] + K * K;                                       // span pairs: the rows of all nodes
    max_mn = std::max(max_mn, s);
    if (K) {
      ext_rows = std::max(ext_rows, out->rows_offset[g] + K * s);
      ext_col = std::max(ext_col, out->col_offset[g] + s);
    }
  }
  int rc;
  if ((rc = check_params(prm, max_mn))) return rc;
  if (max_mn > 0xffffffffull) return set_error(TRACYHIP_ERR_RANGE, "a group's column bound exceeds 2^32");
  GroupOut go(ng, *out);
  if (nt == 0) return go.clear_counts(ctx, mem);  // groups without traces: nrows 0 everywhere

  // ---- inputs: [forward | revcomp | node profiles] in one buffer, the classes of both strands ----
  const uint64_t rev_base = eT, node_base = 2 * eT, nfloat = 2 * eT + 6 * pb[ng];
  float* d_prof; HIP_TRY(ensure_into(B[DN_PROF], nfloat, d_prof));
  uint8_t* d_cls; HIP_TRY(ensure_into(B[DN_COLCLASS], nfloat, d_cls));
  HIP_TRY(hipMemcpyAsync(d_prof, sT.data, eT * 4, mem == TRACYHIP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  std::vector<ProfSeq> hs(2 * (size_t)nt);
  for (uint32_t i = 0; i < nt; ++i) {
    hs[i] = ProfSeq{sT.offset[t0 + i], len_of(i), 0};
    hs[(size_t)nt + i] = ProfSeq{rev_base + sT.offset[t0 + i], len_of(i), 0};
  }
  ProfSeq* d_seqs; HIP_TRY(ensure_into(B[DN_SEQS], hs.size(), d_seqs));
  HIP_TRY(hipMemcpyAsync(d_seqs, hs.data(), sizeof(ProfSeq) * hs.size(), hipMemcpyHostToDevice, st));
  int trc;
  if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 2 * 4ull * eT))) return trc;
  HIP_TRY(launch_prof_revcomp(d_seqs, nt, d_prof, d_prof, rev_base, st));
  uint8_t* d_zero; HIP_TRY(ensure_into(B[DN_CLASS], 2 * (size_t)nt, d_zero));
  const bool screen = !ctx->knobs.no_screen;
  HIP_TRY(launch_prof_classify(d_seqs, 2 * nt, d_prof, d_zero, screen ? d_cls : nullptr, st));
  if ((trc = timing_end(ctx))) return trc;
  std::vector<uint8_t> hz(2 * (size_t)nt);
  HIP_TRY(hipMemcpyAsync(hz.data(), d_zero, hz.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx_sync(ctx));  // (the classes choose the score bodies)
  stage_ms[0] = since(t_stage);
  t_stage = clock_now();

  uint64_t limit;
  if ((rc = workspace_limit(ctx, ctx->dev[DB_BITS].cap + ctx->dev[DB_SCRATCH].cap, &limit))) return rc;

  // ---- the strand table: units (i, oi, j) of two descriptors (oj = 0, 1), one launch per run of equal strip height / term count ----
  std::vector<int> KS(nt);
  for (uint32_t i = 0; i < nt; ++i) KS[i] = choose_k(len_of(i), MODE_PROF);
  auto strand_off = [&](uint32_t i, uint32_t o) { return sT.offset[t0 + i] + (o ? rev_base : 0); };
  struct Unit { uint32_t i, j, oi; };
  std::vector<Unit> units;
  for (uint32_t g = 0; g < ng; ++g)
    for (uint32_t i = gf[g] - t0; i < gf[g + 1] - t0; ++i)
      for (uint32_t oi = 0; oi < 2; ++oi)
        for (uint32_t j = gf[g] - t0; j < gf[g + 1] - t0; ++j)
          if (i != j) units.push_back(Unit{i, j, oi});
  auto row4 = [&](uint32_t i, uint32_t j) { return hz[i] && hz[j]; };
  std::stable_sort(units.begin(), units.end(), [&](const Unit& x, const Unit& y) {
    if (KS[x.i] != KS[y.i]) return KS[x.i] > KS[y.i];
    return row4(x.i, x.j) > row4(y.i, y.j);
  });
  const uint32_t nu = (uint32_t)units.size();
  std::vector<int> k_score(nu);
  const size_t ndesc = std::max<size_t>(2 * (size_t)nu, nt);
  PairDesc *hd, *dd;
  HIP_TRY(ensure_into(ctx->pin[PB_DESC], ndesc, hd));
  HIP_TRY(ensure_into(ctx->dev[DB_DESC], ndesc, dd));
  uint64_t sc_scratch = 0;
  for (uint32_t u = 0; u < nu; ++u) {
    const Unit& x = units[u];
    const uint32_t g = grp[x.i], K = gf[g + 1] - gf[g], base = gf[g] - t0;
    const uint32_t m = len_of(x.i), n = len_of(x.j);
    k_score[u] = KS[x.i];
    PairDesc d = prof_pair_desc(strand_off(x.i, x.oi), m, 0, n, row4(x.i, x.j));
    for (uint32_t oj = 0; oj < 2; ++oj) {
      d.a2_off = strand_off(x.j, oj);
      d.scratch_off = sc_scratch;
      d.out = (uint32_t)(tb[g] + denovo_table_index(K, x.i - base, x.j - base, x.oi, oj));
      hd[2 * (size_t)u + oj] = d;
      if (num_passes(m, KS[x.i]) > 1) sc_scratch += (uint64_t)n + 2;
    }
  }
  if (tb[ng] > 0xffffffffull) return set_error(TRACYHIP_ERR_RANGE, "the strand tables hold more than 2^32 entries");
  if (sc_scratch * 8 > limit)
    return set_error(TRACYHIP_ERR_OOM, "the strand table needs %llu bytes of boundary rows, workspace limit is %llu", (unsigned long long)(sc_scratch * 8),
                     (unsigned long long)limit);
  HIP_TRY(hipMemcpyAsync(dd, hd, sizeof(PairDesc) * 2 * (size_t)nu, hipMemcpyHostToDevice, st));
  if (sc_scratch) HIP_TRY(ctx->dev[DB_SCRATCH].ensure(sc_scratch * 8));
  int32_t* d_table; HIP_TRY(ensure_into(B[DN_TABLE], std::max<uint64_t>(tb[ng], 1), d_table));

  DpArgs a = scoring_args(ctx, prm);
  a.a1 = d_prof;
  a.a2 = d_prof;
  a.scratch = static_cast<int32_t*>(ctx->dev[DB_SCRATCH].p);
  a.screen = screen ? 1 : 0;
  a.colcode = screen ? d_cls : nullptr;
  a.scores = d_table;
  std::vector<std::pair<uint32_t, int>> narrow_launches;
  std::vector<int32_t> table(std::max<uint64_t>(tb[ng], 1), 0);
  if ((rc = prof_score_stage(ctx, prm, wide, a, hd, dd, k_score.data(), nu, table.data(), tb[ng], max_mn, narrow_launches))) return rc;
  stage_ms[1] = since(t_stage);

  // ---- strands (revSeqBasedOnDist) ----
  std::vector<uint8_t> rev(nt, 0), h_fwd(nt);
  {
    std::vector<uint8_t> r;
    std::vector<int32_t> dmat;
    for (uint32_t g = 0; g < ng; ++g) {
      const uint32_t K = gf[g + 1] - gf[g];
      denovo_strands(table.data() + tb[g], K, r, dmat);
      for (uint32_t i = 0; i < K; ++i) rev[gf[g] - t0 + i] = r[i];
    }
    for (uint32_t i = 0; i < nt; ++i) h_fwd[i] = rev[i] ? 0 : 1;
  }
  auto T_of = [&](uint32_t g, uint32_t i, uint32_t j) {  // gotohScore of the chosen strands of traces i and j of group g
    const uint32_t K = gf[g + 1] - gf[g], base = gf[g] - t0;
    return table[tb[g] + denovo_table_index(K, i, j, rev[base + i], rev[base + j])];
  };

  // ---- chunks of groups: the traceback planes (and boundary rows) of an overlap round and of a tree height fit the workspace ----
  // A round aligns every trace of a group with one partner.  The nodes of one height have disjoint leaves, so their sides m_k, n_k
  // sum to at most S; a sweep takes at most m / 256 + 1 passes of (n + 63) x 64 words: the planes of a height are bounded by
  // (S^2 / 1024 + 63 S / 256 + S + 32 K + 2) x 64 words (m n <= S^2 / 4 summed over the nodes), its boundary rows by S + K.
  ChunkCut cut(limit);
  for (uint32_t g = 0; g < ng; ++g) {
    const uint64_t K = gf[g + 1] - gf[g];
    uint64_t round_words = 0, round_scr = 0;
    for (uint32_t i = gf[g] - t0; i < gf[g + 1] - t0; ++i) {
      const uint32_t P = num_passes(len_of(i), KS[i]);
      round_words += (uint64_t)P * steps_per_pass((uint32_t)maxlen[g]) * 64;
      if (P > 1) round_scr += maxlen[g] + 2;
    }
    const uint64_t s = S[g];
    const uint64_t tree_words = (s * s / 1024 + 63 * s / 256 + s + 32 * K + 2) * 64, tree_scr = s + K;
    const uint64_t need = K < 2 ? 0 : std::max(round_words * 8 + round_scr * 8, tree_words * 8 + tree_scr * 8);
    if (!cut.add(g, need))
      return set_error(TRACYHIP_ERR_OOM, "group %u needs %llu bytes of traceback planes, workspace limit is %llu", g, (unsigned long long)need,
                       (unsigned long long)limit);
  }
  const std::vector<CutChunk>& chunks = cut.finish();

  // ---- the call's own buffers ----
  uint8_t* d_ops; HIP_TRY(ensure_into(B[DN_OPS], std::max<uint64_t>(ob[ng], 1), d_ops));
  uint64_t* d_off; HIP_TRY(ensure_into(B[DN_OFF], (size_t)nt, d_off));
  uint32_t* d_len; HIP_TRY(ensure_into(B[DN_LEN], (size_t)nt, d_len));
  uint32_t* d_cnt; HIP_TRY(ensure_into(B[DN_CNT], (size_t)nt, d_cnt));
  int32_t* d_span; HIP_TRY(ensure_into(B[DN_SPAN], 2 * std::max<uint64_t>(sb[ng], 1), d_span));
  // AsmStep: nt for the nodes of a height, ng more for the trees that are one leaf; AsmFinal: ng
  HIP_TRY(B[DN_STEP].ensure(sizeof(AsmStep) * ((size_t)nt + ng) + sizeof(AsmFinal) * (size_t)ng));
  AsmStep* d_step = static_cast<AsmStep*>(B[DN_STEP].p);
  AsmFinal* d_fin = reinterpret_cast<AsmFinal*>(d_step + nt + ng);
  HIP_TRY(ctx->pin[PB_TMP].ensure(sizeof(AsmStep) * ((size_t)nt + ng) + sizeof(AsmFinal) * (size_t)ng));
  AsmStep* h_step = static_cast<AsmStep*>(ctx->pin[PB_TMP].p);
  AsmFinal* h_fin = reinterpret_cast<AsmFinal*>(h_step + nt + ng);
  uint64_t* h_off; HIP_TRY(ensure_into(ctx->pin[PB_OFF], (size_t)nt, h_off));
  uint32_t* h_res; HIP_TRY(ensure_into(ctx->pin[PB_RES], 2 * (size_t)nt, h_res));  // op counts, then 's' counts
  uint32_t* h_len = h_res;
  uint32_t* h_cnt = h_res + nt;
  HIP_TRY(hipMemsetAsync(d_len, 0, sizeof(uint32_t) * (size_t)nt, st));
  HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * (size_t)nt, st));

  if ((rc = go.bind(ctx, mem, ext_rows, ext_col))) return rc;

  a.scores = nullptr;
  std::vector<uint32_t> h_partner(nt, 0xffffffffu), h_row(nt, 0xffffffffu), h_nrows(ng, 0), h_ncol(ng, 0);
  std::vector<uint32_t> next(nt, 0), act;
  std::vector<int8_t> state(nt, 0);  // 0 undecided, 1 kept, -1 excluded
  std::vector<GroupPlan> plan(ng);
  uint32_t total_rounds = 0, total_steps = 0;
  TraceBatch batch{hd, dd, d_ops, d_off, d_len, limit};  // the sweeps of an overlap round or a tree height: upload() sizes the planes for them

  for (const CutChunk& c : chunks) {
    const uint32_t clo = gf[c.lo] - t0, chi = gf[c.hi] - t0;  // the chunk's traces
    // ---- the overlap test (assemble.h:425-456), one partner per undecided trace and round ----
    t_stage = clock_now();
    for (uint32_t g = c.lo; g < c.hi; ++g) {
      uint64_t at = ob[g];
      for (uint32_t i = gf[g] - t0; i < gf[g + 1] - t0; ++i) { h_off[i] = at; at += (uint64_t)len_of(i) + maxlen[g]; }
    }
    if (chi > clo) HIP_TRY(hipMemcpyAsync(d_off + clo, h_off + clo, sizeof(uint64_t) * (chi - clo), hipMemcpyHostToDevice, st));
    for (;;) {
      act.clear();
      for (uint32_t i = clo; i < chi; ++i) {
        if (state[i]) continue;
        const uint32_t g = grp[i], base = gf[g] - t0, K = gf[g + 1] - gf[g];
        if (next[i] == i - base) ++next[i];
        if (next[i] >= K) { state[i] = -1; continue; }
        act.push_back(i);
      }
      if (act.empty()) break;
      auto partner = [&](uint32_t i) { return gf[grp[i]] - t0 + next[i]; };
      std::stable_sort(act.begin(), act.end(), [&](uint32_t x, uint32_t y) {
        if (KS[x] != KS[y]) return KS[x] > KS[y];
        return row4(x, partner(x)) > row4(y, partner(y));
      });
      const uint32_t na = (uint32_t)act.size();
      batch.clear();
      for (uint32_t u = 0; u < na; ++u) {
        const uint32_t i = act[u], j = partner(i);
        batch.add(strand_off(i, rev[i]), len_of(i), strand_off(j, rev[j]), len_of(j), row4(i, j), KS[i], i);
      }
      if ((rc = batch.upload(ctx, a))) return rc;
      if ((rc = prof_trace_runs(ctx, a, hd, dd, batch.k.data(), 0, na, d_ops, d_off, d_len))) return rc;
      if ((trc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, 0))) return trc;
      hipLaunchKernelGGL(denovo_count_kernel, dim3(na), dim3(64), 0, st, (const PairDesc*)dd, (const uint8_t*)d_ops, (const uint64_t*)d_off,
                         (const uint32_t*)d_len, d_cnt);
      HIP_TRY(hipGetLastError());
      if ((trc = timing_end(ctx))) return trc;
      HIP_TRY(hipMemcpyAsync(h_len + clo, d_len + clo, sizeof(uint32_t) * (chi - clo), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(h_cnt + clo, d_cnt + clo, sizeof(uint32_t) * (chi - clo), hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx_sync(ctx));
      for (uint32_t u = 0; u < na; ++u) {
        const uint32_t i = act[u], g = grp[i], base = gf[g] - t0;
        if (h_len[i] > hd[u].m + hd[u].n)
          return set_error(TRACYHIP_ERR_RANGE, "group %u, trace %u: the traceback gave %u ops for %u rows and columns", g, i - base, h_len[i],
                           hd[u].m + hd[u].n);
        if (denovo_overlap_ok((int32_t)h_cnt[i], T_of(g, i - base, next[i]), (int32_t)len_of(i), job->match_fraction, prm->match, prm->mismatch)) {
          state[i] = 1;
          h_partner[i] = next[i];
        } else {
          ++next[i];
        }
      }
      ++total_rounds;
    }

    stage_ms[2] += since(t_stage);
    t_stage = clock_now();

    // ---- the trees (msa.h:326-368): UPGMA on the host, where every node lives ----
    uint64_t rows_need = 0;
    uint32_t maxh = 0, nleafroot = 0;
    for (uint32_t g = c.lo; g < c.hi; ++g) {
      GroupPlan& gp = plan[g];
      const uint32_t base = gf[g] - t0, K = gf[g + 1] - gf[g];
      for (uint32_t i = 0; i < K; ++i)
        if (state[base + i] == 1) gp.keep.push_back(i);
      const uint32_t num = (uint32_t)gp.keep.size();
      if (num < 2) continue;  // "At least 2 traces are required for de novo assembly!"
      std::vector<int32_t> dist((size_t)num * num, 0);
      for (uint32_t x = 0; x < num; ++x)
        for (uint32_t y = x + 1; y < num; ++y) dist[(size_t)x * num + y] = T_of(g, gp.keep[x], gp.keep[y]);
      denovo_tree(dist.data(), (int32_t)num, gp.tree);
      const DenovoTree& t = gp.tree;
      gp.node.assign(2 * (size_t)num + 1, TreeNode());
      for (uint32_t x = 0; x < num; ++x) {
        TreeNode& nd = gp.node[x];
        const uint32_t i = base + gp.keep[x];
        nd.n = 1;
        nd.cap = nd.ncol = len_of(i);
        nd.prof_off = strand_off(i, rev[i]);
        nd.row4_zero = hz[i] != 0;
      }
      uint64_t prof_at = node_base + 6 * pb[g], ops_at = ob[g], span_at = sb[g];
      uint32_t q = 0;
      for (int32_t v = (int32_t)num; v <= t.root; ++v) {  // (children before parents)
        if (!t.below_root[v]) continue;
        TreeNode& nd = gp.node[v];
        const TreeNode &l = gp.node[t.p[v][1]], &r = gp.node[t.p[v][2]];
        nd.n = l.n + r.n;
        nd.cap = l.cap + r.cap;
        nd.ops_off = ops_at; ops_at += nd.cap;
        nd.span_off = span_at; span_at += nd.n;
        nd.slot = base + q++;
        if (v != t.root) {
          nd.prof_off = prof_at; prof_at += 6ull * nd.cap;
          nd.rows_off = rows_need; rows_need += (uint64_t)nd.n * nd.cap;
        }
      }
      // (what the bounds of the geometry promise: K - 1 nodes of at most S columns, K - 2 of them below the root, K^2 rows in all)
      if (ops_at > ob[g + 1] || span_at > sb[g + 1] || prof_at > node_base + 6 * pb[g + 1] || q > K)
        return set_error(TRACYHIP_ERR_RANGE, "group %u: the tree outgrew its workspace", g);
      for (uint32_t r = 0; r < t.order.size(); ++r) h_row[base + gp.keep[t.order[r]]] = r;
      h_nrows[g] = (uint32_t)t.order.size();
      maxh = std::max<uint32_t>(maxh, (uint32_t)t.maxh);
    }
    uint8_t* d_rows; HIP_TRY(ensure_into(B[DN_ROWS], std::max<uint64_t>(rows_need, 1), d_rows));
    // the op offsets of the nodes replace those of the rounds
    for (uint32_t g = c.lo; g < c.hi; ++g) {
      const GroupPlan& gp = plan[g];
      if (gp.keep.size() < 2) continue;
      for (int32_t v = gp.tree.num; v <= gp.tree.root; ++v)
        if (gp.tree.below_root[v]) h_off[gp.node[v].slot] = gp.node[v].ops_off;
    }
    // a tree that is one leaf (UPGMA joined nothing): its row is the leaf's _profileConsChar row -- a merge along len 's' ops with no right side
    for (uint32_t g = c.lo; g < c.hi; ++g) {
      GroupPlan& gp = plan[g];
      if (gp.keep.size() < 2 || gp.tree.root >= gp.tree.num) continue;
      TreeNode& leaf = gp.node[gp.tree.root];
      const uint32_t slot = gf[g] - t0;
      leaf.slot = slot;
      leaf.span_off = sb[g];
      HIP_TRY(hipMemsetAsync(d_ops + ob[g], 's', leaf.ncol, st));
      h_off[slot] = ob[g];
      HIP_TRY(hipMemcpyAsync(d_len + slot, &leaf.ncol, sizeof(uint32_t), hipMemcpyHostToDevice, st));  // (pageable: copied before the call returns)
      AsmStep s{};
      s.left = MsaSide{nullptr, d_prof + leaf.prof_off, 1u, leaf.ncol, leaf.ncol};
      s.right = MsaSide{nullptr, nullptr, 0u, 0u, 0u};
      s.ops_off = ob[g];
      s.slot = slot;
      s.cap = leaf.ncol;
      s.dst = go.d_rows + go.rows_offset[g];
      s.span = d_span + 2 * leaf.span_off;
      h_step[nt + nleafroot++] = s;
      h_ncol[g] = leaf.ncol;
    }
    if (chi > clo) HIP_TRY(hipMemcpyAsync(d_off + clo, h_off + clo, sizeof(uint64_t) * (chi - clo), hipMemcpyHostToDevice, st));
    if (nleafroot) {
      HIP_TRY(hipMemcpyAsync(d_step + nt, h_step + nt, sizeof(AsmStep) * nleafroot, hipMemcpyHostToDevice, st));
      HIP_TRY(launch_msa_merge(d_step + nt, nleafroot, 1, d_ops, d_len, st));
    }

    // ---- the merges, one batch per height ----
    struct Item { uint32_t g; int32_t v; };
    std::vector<Item> items;
    for (uint32_t h = 1; h <= maxh; ++h) {
      items.clear();
      for (uint32_t g = c.lo; g < c.hi; ++g) {
        const GroupPlan& gp = plan[g];
        if (gp.keep.size() < 2) continue;
        for (int32_t v = gp.tree.num; v <= gp.tree.root; ++v)
          if (gp.tree.below_root[v] && gp.tree.height[v] == (int32_t)h) items.push_back(Item{g, v});
      }
      auto left_of = [&](const Item& x) -> const TreeNode& { return plan[x.g].node[plan[x.g].tree.p[x.v][1]]; };
      auto right_of = [&](const Item& x) -> const TreeNode& { return plan[x.g].node[plan[x.g].tree.p[x.v][2]]; };
      auto flags_of = [&](const Item& x) { return (left_of(x).row4_zero && right_of(x).row4_zero) ? (uint32_t)PAIR_ROW4_ZERO : 0u; };  // (leaves only)
      std::stable_sort(items.begin(), items.end(), [&](const Item& x, const Item& y) {
        const int kx = choose_k(left_of(x).ncol, MODE_PROF), ky = choose_k(left_of(y).ncol, MODE_PROF);
        if (kx != ky) return kx > ky;
        return flags_of(x) > flags_of(y);
      });
      const uint32_t na = (uint32_t)items.size();
      batch.clear();
      for (uint32_t u = 0; u < na; ++u) {
        const Item& x = items[u];
        const GroupPlan& gp = plan[x.g];
        const TreeNode &nd = gp.node[x.v], &l = left_of(x), &r = right_of(x);
        const bool root = x.v == gp.tree.root;
        batch.add(l.prof_off, l.ncol, r.prof_off, r.ncol, flags_of(x) != 0, choose_k(l.ncol, MODE_PROF), nd.slot);
        auto side = [&](const TreeNode& s, int32_t idx) {
          return idx < gp.tree.num ? MsaSide{nullptr, d_prof + s.prof_off, 1u, s.ncol, s.ncol} : MsaSide{d_rows + s.rows_off, nullptr, s.n, s.ncol, 0u};
        };
        AsmStep s{};
        s.left = side(l, gp.tree.p[x.v][1]);
        s.right = side(r, gp.tree.p[x.v][2]);
        s.ops_off = nd.ops_off;
        s.slot = nd.slot;
        s.cap = l.ncol + r.ncol;
        s.dst = root ? go.d_rows + go.rows_offset[x.g] : d_rows + nd.rows_off;
        s.span = d_span + 2 * nd.span_off;
        s.prof = root ? nullptr : d_prof + nd.prof_off;
        s.colclass = root ? nullptr : d_cls + nd.prof_off;
        h_step[u] = s;
      }
      // the op counts: the columns of the nodes (and, for a root, the group's ncol)
      if ((rc = msa_merge_batch(ctx, a, batch, h_step, d_step, h_len, clo, chi))) return rc;
      for (uint32_t u = 0; u < na; ++u) {
        const Item& x = items[u];
        GroupPlan& gp = plan[x.g];
        TreeNode& nd = gp.node[x.v];
        if (h_len[nd.slot] > h_step[u].cap)
          return set_error(TRACYHIP_ERR_RANGE, "group %u, height %u: the traceback gave %u ops for %u rows and columns", x.g, h, h_len[nd.slot],
                           h_step[u].cap);
        nd.ncol = h_len[nd.slot];
        if (x.v == gp.tree.root) h_ncol[x.g] = nd.ncol;
      }
      ++total_steps;
    }

    stage_ms[3] += since(t_stage);
    t_stage = clock_now();

    // ---- msa_consensus of the chunk's groups ----
    uint32_t nf = 0;
    for (uint32_t g = c.lo; g < c.hi; ++g) {
      const GroupPlan& gp = plan[g];
      if (!h_nrows[g]) continue;
      const TreeNode& root = gp.node[gp.tree.root];
      h_fin[nf++] = go.final_entry(g, d_span + 2 * root.span_off, root.n, root.slot, root.cap, job->fraction_called);
    }
    if ((rc = msa_consensus_batch(ctx, h_fin, d_fin, nf, d_len))) return rc;
    stage_ms[4] += since(t_stage);
    // (the pinned h_step / h_fin / hd are filled again by the next chunk behind the synchronisations of its rounds; its entries of
    // h_off / h_len are its own traces')
  }

  // ---- the last synchronisation: error words, results ----
  t_stage = clock_now();
  int32_t herr[kErrWords] = {};
  HIP_TRY(hipMemcpyAsync(herr, ctx->dev[DB_ERR].p, sizeof(herr), hipMemcpyDeviceToHost, st));
  if ((rc = put_result(ctx, mem, out->forward + t0, h_fwd.data(), (size_t)nt)) ||
      (rc = put_result(ctx, mem, out->partner + t0, h_partner.data(), 4 * (size_t)nt)) ||
      (rc = put_result(ctx, mem, out->row + t0, h_row.data(), 4 * (size_t)nt)) ||
      (rc = go.copy_back(ctx, mem, h_nrows.data(), h_ncol.data())))
    return rc;
  HIP_TRY(ctx_sync(ctx));
  timing_collect(ctx);
  ctx->stats.denovo_chunks = (uint32_t)chunks.size();
  ctx->stats.denovo_rounds = total_rounds;
  ctx->stats.denovo_steps = total_steps;
  stage_ms[4] += since(t_stage);
  if (ctx->knobs.verbose)
    std::fprintf(stderr, "tracyhip_denovo_traces: groups %u traces %u chunks %zu | inputs_ms %.3f | table_ms %.3f pairs %u | rounds_ms %.3f rounds %u | "
                 "tree_ms %.3f heights %u | consensus_results_ms %.3f\n", ng, nt, chunks.size(), stage_ms[0], stage_ms[1], 2 * nu, stage_ms[2], total_rounds,
                 stage_ms[3], total_steps, stage_ms[4]);
  return range_verdict(prm, herr, narrow_launches, max_mn, kTagShift);
}

}  // namespace

extern "C" {

int tracyhip_denovo_validate(const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem, const tracyhip_denovo_result* out) {
  return denovo_validate(job, prm, mem, out);
}

int tracyhip_denovo_traces(tracyhip_ctx* ctx, const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem, const tracyhip_denovo_result* out) {
  int rc = denovo_validate(job, prm, mem, out);  // (before any device is touched)
  if (rc) return rc;
  if ((rc = ctx_begin(ctx))) return rc;
  ctx->stats = tracyhip_call_stats{};
  ctx->stats.traces = job->ngroups ? job->group_first[job->ngroups] - job->group_first[0] : 0;
  ctx->stats.stream_ordered = 1;
  if (job->ngroups == 0) return check_params(prm, 0);
  rc = denovo_run(ctx, job, prm, mem, out, false);
  if (rc == kWiden) rc = denovo_run(ctx, job, prm, mem, out, true);
  return rc;
}

int tracyhip_denovo_traces_async(tracyhip_ctx* ctx, const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem,
                                 const tracyhip_denovo_result* out) {
  if (!ctx || !job || !prm || !out) return set_error(TRACYHIP_ERR_ARG, "null context / job / params / result");
  const tracyhip_denovo_job j = *job;
  const tracyhip_params q = *prm;
  const tracyhip_denovo_result o = *out;
  return async_submit(ctx, [=]() { return tracyhip_denovo_traces(ctx, &j, &q, mem, &o); });
}

}  // extern "C"
