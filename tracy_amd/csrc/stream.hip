// stream.hip -- tracyhip_align_traces / tracyhip_decompose_traces stream-ordered: the stage orders of sage.h:191-311 and
// indigo.h:190-388 queued on the context's stream from the first kernel to the last, with ONE host synchronisation at the end.
//
// pipeline.hip reads verdicts back after every stage, plans the next launch on the host and uploads its descriptors: ~40
// synchronisations, ~100 copies and 14-20 % idle GPU per `tracy decompose` step, a fixed cost that does not shrink with the batch
// (VERDICT round 3).  Here the host uploads one record of geometry per trace (SGeom: what it knows before anything runs) and small
// kernels do the planning between the DP launches from the results where they lie (stream_plan.h): the class of a trace from its
// k-mer vote, the descriptors of the sweeps and pruned sweeps, the orientation decision, the sub-window and band an alignment's
// score allows, the strip height that sweeps it (lists per strip height by a one-workgroup scan; the band kernels read their
// sizes from the device, Band16Args::count), the certificates.  Lists have fixed slots (PAIR_SKIP for the empty ones) or worst-case
// grids whose surplus waves leave at once: nothing the host has to know before it launches.
//
// Exactness: every shortcut is certified per trace by the rules pipeline.hip calls (stream_plan.h); a trace whose certificate fails, or whose band is
// wider than the band kernels hold, is marked dead (SD_* reasons), skipped by everything after it, and re-done afterwards by the
// host-planned pipeline -- all its tiers -- on the list of dead traces (restoring the basecalls `tracy decompose` rewrites in
// place).  Value-range reports of the 16-bit kernels (un-normalised profiles) send the whole call there.  Results are the
// arrays pipeline.hip writes, bit for bit (tests/test_gpu_stream.py: A/B on ragged batches incl. every failing certificate).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "decompose_launch.h"
#include "launch.h"
#include "pipe_internal.h"
#include "pipe_kernels.h"
#include "stream_fields.h"
#include "stream_plan.h"

using namespace tracyhip;

#define TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)

namespace {

// ---- device memory of one call: one block, carved in order (first pass sizes it, second pass hands out the pointers) ----
struct Arena {
  char* base = nullptr;
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    off = (off + 255u) & ~(size_t)255u;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += sizeof(T) * (count ? count : 1);
    return p;
  }
  template <class T>
  void take_into(T*& p, size_t count) { p = take<T>(count); }
};

// Counters of a planning kernel: summed per workgroup in LDS, one global atomic per counter and workgroup at the end (10^5 threads
// adding to one global word take milliseconds).  body(lc) may return early; lc is the workgroup's block of SC_COUNT words.
__device__ __forceinline__ void s_count(unsigned long long* lc, int which, unsigned long long v = 1ull) { atomicAdd(lc + which, v); }
template <class Body>
__device__ __forceinline__ void with_counters(unsigned long long* cnt, Body body) {
  __shared__ unsigned long long lc[SC_COUNT];
  for (uint32_t i = threadIdx.x; i < (uint32_t)SC_COUNT; i += blockDim.x) lc[i] = 0;
  __syncthreads();
  body(lc);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < (uint32_t)SC_COUNT; i += blockDim.x)
    if (lc[i]) atomicAdd(cnt + i, lc[i]);
}
// the first tier of a pruned sweep (TRACYHIP_TIMER_FRONT: what run_front_once credits for the same tier)
__device__ __forceinline__ void s_count_front(unsigned long long* lc, const FrontDesc& f) {
  const Credit c = front_credit(f.m_rest, f.n, kFrontK1, kFrontHalfW1);
  s_count(lc, SC_FRONT_CELLS, c.cells);
  s_count(lc, SC_FRONT_BYTES, c.bytes);
}

// Wave priority (band16_launch.h wave_prio) of a launch that is being queued: tier 1 -- the tiers of the pruned sweep and the early
// decision -- from option chain_prio = 1 on, tier 2 -- the early tail's stages -- at 2; nonzero only while queue_orientation queues the voted
// strand's chain on its side stream beside the full sweeps (tracyhip_ctx::queue_prio), so the pass behind the decision launches the same
// kernels unraised.
inline int queued_prio(const tracyhip_ctx* ctx, uint32_t tier) { return ctx->queue_prio >= tier ? 1 : 0; }

// ---- geometry -> descriptor lists of the fixed-shape kernels (vote, row maxima, substitution tables) ----
__global__ void s_expand_kernel(const SGeom* __restrict__ geom, uint32_t nt, VoteDesc* __restrict__ vd, RowMaxDesc* __restrict__ rm_rest,
                                RowMaxDesc* __restrict__ rm_trim, RowMaxDesc* __restrict__ rm_full, B16TableDesc* __restrict__ td) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  const SGeom G = geom[t];
  const uint64_t a1 = G.prof_off + G.tl;
  vd[t] = VoteDesc{a1, G.ref_off, G.mf, G.mt, G.rn, 0u};
  rm_rest[t] = RowMaxDesc{a1, G.mf, G.mt, kFrontRows};
  rm_trim[t] = RowMaxDesc{a1, G.mf, G.mt, 0u};
  if (rm_full) rm_full[t] = RowMaxDesc{G.prof_off, G.mf, G.mf, 0u};
  td[t] = B16TableDesc{G.prof_off, G.tab_off, G.mf, G.mf, G.tab_stride, 0u};
}

// the pair a sweep of the trimmed trace against its window in orientation o is (pipeline.hip stage1_desc)
__device__ __forceinline__ PairDesc s_stage1_desc(const SGeom& G, uint32_t t, uint32_t nt, uint32_t o) {
  PairDesc d{};
  d.a1_off = G.prof_off + G.tl;
  d.a1_stride = G.mf;
  d.m = G.mt;
  d.a2_off = G.ref_off;
  d.n = G.rn;
  d.a2_stride = G.rn;
  d.out = o * nt + t;
  d.flags = o ? PAIR_A2_REVCOMP : 0u;
  d.lastrow_off = G.lr_off[o];
  return d;
}

// ---- orientation stage, step 1 (pipeline.hip "o.b"): class of every trace from its vote (s_orient_class); the sweep / prefix / pruned-sweep slots ----
// cls 0: pruned sweep of the voted strand g (prefix with the row kept + band), the other strand swept in full (exact) or bounded by
// its prefix; cls 1: both strands in full; cls 2 (strand by certificate only): g in full, prefix of the other
__global__ void s_orient_plan_kernel(SParams p, const SGeom* __restrict__ geom, const uint32_t* __restrict__ votes, const int32_t* __restrict__ ub,
                                     const int32_t* __restrict__ ub1, PairDesc* __restrict__ full, PairDesc* __restrict__ pre,
                                     FrontDesc* __restrict__ fd, STrace* __restrict__ tr, unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  const SGeom G = geom[t];
  const uint32_t R = kFrontRows;
  const SOrient o = s_orient_class(votes[2 * t], votes[2 * t + 1], G.mt, (G.flags & SG_FRONT_OK) != 0u, p.exact != 0u);
  const uint32_t g = o.g, cls = o.cls;
  PairDesc fa = s_skip_pair(t), fb = s_skip_pair(t), pa = s_skip_pair(t), pb = s_skip_pair(t);
  FrontDesc f{};
  f.flags = PAIR_SKIP;
  f.out = t;
  uint64_t cells = 0, bytes = 0, pcells = 0;
  const Credit full_c = sweep_pair_credit(G.mt, G.rn, true, false), pre_c = prefix_credit(G.mt, G.rn, R);
  const uint64_t full_cells = full_c.cells, pre_cells = pre_c.cells, full_bytes = full_c.bytes;
  if (cls == 0u) {
    pa = s_stage1_desc(G, t, p.nt, g);
    pa.flags |= PAIR_KEEP_ROW;
    pcells += pre_cells;
    if (p.exact) { fa = s_stage1_desc(G, t, p.nt, 1u - g); cells += full_cells; bytes += full_bytes; }
    else { pb = s_stage1_desc(G, t, p.nt, 1u - g); pcells += pre_cells; }
    f.row_off = G.lr_off[g];
    f.a2_off = G.ref_off;
    f.tab_off = G.tab_off + G.tl + R;
    f.tab_stride = G.tab_stride;
    f.m_rest = G.mt - R;
    f.n = G.rn;
    f.flags = g ? PAIR_A2_REVCOMP : 0u;
    f.R = R;
    f.rest = ub[t];
    f.tight = (p.ge <= -2 && ub1[t] <= ub[t]) ? (uint32_t)(ub[t] - ub1[t]) + 1u : 0u;
    s_count_front(lc, f);
  } else if (cls == 1u) {
    fa = s_stage1_desc(G, t, p.nt, g);
    fb = s_stage1_desc(G, t, p.nt, 1u - g);
    cells += 2 * full_cells; bytes += 2 * full_bytes;
  } else {
    fa = s_stage1_desc(G, t, p.nt, g);
    pb = s_stage1_desc(G, t, p.nt, 1u - g);
    cells += full_cells; pcells += pre_cells; bytes += full_bytes;
  }
  // the prefixes: part of the sweep launch, or -- in a launch of their own beside it -- of the pruned sweep they begin
  if (p.split_prefix) { s_count(lc, SC_FRONT_CELLS, pcells); s_count(lc, SC_FRONT_BYTES, pcells ? pre_c.bytes : 0ull); }
  else cells += pcells;
  full[G.full_a] = fa;
  full[G.full_b] = fb;
  pre[t] = pa;
  if (!p.exact) pre[p.nt + t] = pb;
  fd[t] = f;
  STrace S{};
  S.g = (uint8_t)g;
  S.cls = (uint8_t)cls;
  tr[t] = S;
  s_count(lc, SC_SWEEP_CELLS, cells);
  s_count(lc, SC_SWEEP_BYTES, bytes);
  });
}

// what the tiers of a pruned sweep certified for unit t: c_e (window column, 1-based; 0: no tier certified it) and the score
__device__ __forceinline__ uint32_t s_front_result(uint32_t t, const FrontOut* __restrict__ fo1, const int32_t* __restrict__ fs1, const uint32_t* __restrict__ fe1,
                                                   const FrontOut* __restrict__ fo2, const int32_t* __restrict__ fs2, const uint32_t* __restrict__ fe2, int64_t* s_g) {
  if (fo1[t].ok) { *s_g = fs1[t]; return fe1[2 * t + 1] ? fe1[2 * t + 1] + fo1[t].shift : 0u; }
  if (fo2[t].ok) { *s_g = fs2[t]; return fe2[2 * t + 1] ? fe2[2 * t + 1] + fo2[t].shift : 0u; }
  return 0u;
}

// ---- orientation stage, step 2 ahead of time (`tracy align`, on the voted strand's side stream behind its tiers): a trace of class 0
// that a tier certified gets the decision "the voted strand g won" -- S.fwd / rc / sstar / ce as s_orient_decide_kernel will leave them
// if gsFwd > gsRev comes out that way -- and the mark ST_EARLY, so that its preliminary and final alignment can be queued beside the
// other strand's full sweep.  Assumed, not known: S.sc[1 - g] stays open until that sweep has ended, and s_orient_decide_kernel then
// confirms the trace or gives it SD_LOSER_WON, the verdict a clear vote's loser that wins has always had (its sweep kept no row m).
// Only queued when both scores are exact: by certificate there is no full sweep to run beside (no trace is marked, the order before).
// Every other trace is left alone: it is decided, and its alignments are queued, behind the sweeps. ----
__global__ void s_orient_early_kernel(SParams p, const FrontOut* __restrict__ fo1,
                                      const int32_t* __restrict__ fs1, const uint32_t* __restrict__ fe1, const FrontOut* __restrict__ fo2,
                                      const int32_t* __restrict__ fs2, const uint32_t* __restrict__ fe2, STrace* __restrict__ tr, int prio) {
  wave_prio(prio);
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  STrace S = tr[t];
  if (S.cls != 0u || !p.use_votes || !p.exact) return;
  const uint32_t g = S.g;
  int64_t s_g = 0;
  const uint32_t fce = s_front_result(t, fo1, fs1, fe1, fo2, fs2, fe2, &s_g);
  if (fce == 0u) return;
  // (not S.sc[g]: a record indexed by a variable is no longer kept in registers -- the compiler moved all of it to LDS, 52 KB per
  // workgroup, which no CU has free while the sweeps' workgroups fill it: this kernel, 10 us on its own, then waited 0.2-0.6 ms for room)
  if (g == 0u) S.sc[0] = (int32_t)s_g;
  else S.sc[1] = (int32_t)s_g;
  S.fwd = g == 0u ? 1 : 0;
  S.rc = (uint8_t)g;
  S.sstar = (int32_t)s_g;
  S.ce = fce;
  S.mark = ST_EARLY;
  tr[t] = S;
}

// ---- orientation stage, step 2 (pipeline.hip "o.e" .. "o.f"): scores of both strands, the decision gsFwd > gsRev (sage.h:247), the
// winner's c_e from the pruned sweep or (RowEndDesc) from its row m.  For a trace marked ST_EARLY this is the confirmation: the rule is
// the same, and where it names the voted strand every field comes out as s_orient_early_kernel set it (the fields the early stages
// have added since are kept); where it does not, the trace is dead and what its early stages counted is taken back ----
__global__ void s_orient_decide_kernel(SParams p, const SGeom* __restrict__ geom, const uint32_t* __restrict__ votes, const int32_t* __restrict__ ub,
                                       const int32_t* __restrict__ sc2, const FrontOut* __restrict__ fo1, const int32_t* __restrict__ fs1,
                                       const uint32_t* __restrict__ fe1, const FrontOut* __restrict__ fo2, const int32_t* __restrict__ fs2,
                                       const uint32_t* __restrict__ fe2, STrace* __restrict__ tr, RowEndDesc* __restrict__ re,
                                       uint32_t* __restrict__ dead, unsigned long long* __restrict__ cnt, PairDesc* __restrict__ desc_trim) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  const SGeom G = geom[t];
  STrace S = tr[t];
  const uint32_t g = S.g, o = 1u - g, nt = p.nt;
  uint32_t dd = 0;
  int64_t s_g = 0, s_o = 0;
  uint32_t fce = 0;
  auto by_bound = [&]() {  // the other strand holds its prefix maximum: decided by its bound (s_strand_by_bound), or its full sweep is needed
    const SStrand c = s_strand_by_bound(g, sc2[o * nt + t], ub[t], s_g);
    if (c.certified) s_o = c.bound;
    else dd |= SD_STRAND;
  };
  if (S.cls == 0u) {
    s_count(lc, SC_PRUNED);
    fce = s_front_result(t, fo1, fs1, fe1, fo2, fs2, fe2, &s_g);
    if (fce == 0u) { dd |= SD_FRONT; s_count(lc, SC_PRUNED_UNCERT); }
    else if (p.exact) s_o = sc2[o * nt + t];
    else by_bound();
  } else if (S.cls == 1u) {
    s_g = sc2[g * nt + t];
    s_o = sc2[o * nt + t];
  } else {
    s_g = sc2[g * nt + t];
    by_bound();
  }
  S.sc[g] = (int32_t)s_g;
  S.sc[o] = (int32_t)s_o;
  const bool fwd = S.sc[0] > S.sc[1];  // forward iff gsFwd > gsRev (sage.h:247)
  S.fwd = fwd ? 1 : 0;
  S.rc = fwd ? 0 : 1;
  const uint32_t w = S.rc;
  S.sstar = S.sc[w];
  const bool from_front = S.cls == 0u && w == g;
  if (!dd && !from_front) {
    // the winner was swept in full: its row m must be there (the likely loser of a clear vote leaves none: DpArgs::votes)
    const bool swept = S.cls == 1u || (S.cls == 0u && p.exact) || (S.cls == 2u && w == g);
    if (!swept) dd |= SD_STRAND;
    else if (p.use_votes && vote_skips_checkpoints(votes[2 * t], votes[2 * t + 1], w)) dd |= SD_LOSER_WON;
  }
  S.ce = from_front ? fce : 0u;
  re[t] = RowEndDesc{G.lr_off[w], (from_front || dd) ? 0u : G.rn, 0u};
  tr[t] = S;
  if (dd && (S.mark & ST_EARLY)) {  // refuted: today's verdict alone, whatever its early stages found on the wrong strand
    dead[t] = dd;
    if (S.mark & ST_COUNTED_PRELIM) s_count(lc, SC_PRELIM_BANDED, ~0ull);  // (- 1: the counters are sums modulo 2^64)
    if (S.mark & ST_COUNTED_FINAL) s_count(lc, SC_FINAL_BANDED, ~0ull);
  } else if (dd) dead[t] |= dd;
  if (desc_trim) {  // `tracy decompose`: the pair alignment_rows_kernel reads (indigo.h:302)
    PairDesc d{};
    d.a1_off = G.prof_off + G.tl; d.a1_stride = G.mf; d.m = G.mt;
    d.a2_off = G.ref_off; d.n = G.rn; d.a2_stride = G.rn;
    d.out = t;
    d.flags = S.rc ? PAIR_A2_REVCOMP : 0u;
    desc_trim[t] = d;
  }
  });
}

// ---- preliminary alignment (pipeline.hip "o.g"): the sub-window and band its score allows around c_e (s_sub_window), as an origin-tracking sweep
// (mode 0, `tracy align`: only its two ends are read) or a traceback completed with the free end-gap columns (mode 1).
// early: the pass over the traces marked ST_EARLY (1) or over all the others (0); a trace of the other pass is an empty slot ----
__global__ void s_prelim_plan_kernel(SParams p, int mode, int early, const SGeom* __restrict__ geom, STrace* __restrict__ tr, const uint32_t* __restrict__ d_ce,
                                     const int32_t* __restrict__ top, uint32_t* __restrict__ dead, PairDesc* __restrict__ cand,
                                     uint8_t* __restrict__ kc, int prio) {
  wave_prio(prio);
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  kc[t] = 0;
  STrace S = tr[t];
  if (((S.mark & ST_EARLY) != 0u) != (early != 0)) return;
  if (dead[t]) return;
  const SGeom G = geom[t];
  const bool from_front = S.cls == 0 && S.rc == S.g;
  const uint32_t ce = from_front ? S.ce : d_ce[t];
  S.ce = ce;
  uint32_t dd = 0;
  if (ce == 0u) dd = SD_JUNK;  // H(m, c) == E(m, c) in every column: n 'h', then m 'v' (pipeline.hip); the host-planned tiers take it
  else {
    const SubWindow sw = s_sub_window(G.mt, ce, top[t], S.sstar, p.ge);
    S.gap = (uint32_t)(sw.g < 0x7fffffff ? sw.g : 0x7fffffff);
    S.shift = sw.a;
    int K = sw.K;
    if (K && mode == 0 && !b16_origin_ok(p.match, p.mismatch, p.go, p.ge, G.mt, sw.n)) K = 0;
    if (K && !s_fits_lds(sw.n, K)) K = 0;
    if (!K) dd = SD_PRELIM_BAND;
    else if (sw.n > p.ncap) dd = SD_SHAPE;
    else {
      PairDesc q{};
      q.a1_off = G.tab_off + G.tl;
      q.a1_stride = G.tab_stride;
      q.m = G.mt;
      q.n = sw.n;
      q.a2_stride = sw.n;
      q.a2_off = G.ref_off + (S.rc ? (uint64_t)(G.rn - ce) : (uint64_t)sw.a);  // reverse view: column c is byte n - c
      q.flags = S.rc ? PAIR_A2_REVCOMP : 0u;
      q.out = t;
      q.ckpt_off = band_pack(sw.dlo, sw.dhi);
      q.lastrow_off = mode == 0 ? 0ull : ((uint64_t)(G.rn - ce) | ((uint64_t)sw.a << 32));  // 'h' right / left of the sub-window
      cand[t] = q;
      kc[t] = (uint8_t)K;
    }
  }
  tr[t] = S;
  if (dd) dead[t] |= dd;
}

// ---- lists per strip height for a band launch: the candidates (kc[i] = 0 / 4 / 8 / 12) are counted per block of 256 (ballots per
// wave), and every block then sums the totals of the blocks before it and hands its pairs their places in their lists (in unit order)
// and the bytes of their traceback words (KIND 0).  No block waits for another, and neither launch holds more than a few hundred bytes
// of LDS: beside the sweeps they fit wherever a wave slot is free.  A pair whose words do not fit the workspace planned for the launch
// becomes an empty slot and its trace is marked (SD_MEM). ----
constexpr uint32_t kScanBlock = 256, kScanWaves = kScanBlock / 64;
struct ScanPart { uint32_t n[4]; unsigned long long bytes; };
// lists: strip height 12, 8, 4, and the quad form (strip height 4, four lanes per pair) for the narrow bands when the launch has room for it
__device__ __forceinline__ int s_bucket(int K, const PairDesc& d, int quads) {
  const int b = band_bucket(K);  // (kc holds 12, 8 or 4: every other value lands in the lists of height 4, never outside them)
  return (b == 0 || b == 1) ? b : (quads && b16_narrow_ok(band_dmin(d), band_dmax(d))) ? 3 : 2;
}
// sums over the 64 lanes of a wave (every lane gets the sum); the totals of a block's four waves, which lane 0 of each left in LDS
__device__ __forceinline__ uint32_t s_wave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long s_wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ ScanPart s_waves_before(const ScanPart* __restrict__ w, uint32_t upto) {
  ScanPart t{{0, 0, 0, 0}, 0};
  for (uint32_t k = 0; k < upto; ++k) { for (int b = 0; b < 4; ++b) t.n[b] += w[k].n[b]; t.bytes += w[k].bytes; }
  return t;
}
__global__ __launch_bounds__(kScanBlock) void s_scan_count_kernel(const PairDesc* __restrict__ cand, const uint8_t* __restrict__ kc, uint32_t n, int kind,
                                                                  int quads, ScanPart* __restrict__ part, int prio) {
  wave_prio(prio);
  __shared__ ScanPart s_w[kScanWaves];
  const uint32_t tid = threadIdx.x, wv = tid >> 6, L = tid & 63u;
  const uint32_t i = blockIdx.x * kScanBlock + tid;
  const int K = i < n ? kc[i] : 0;
  int bucket = -1;
  unsigned long long mine = 0;
  if (K) {
    const PairDesc d = cand[i];
    bucket = s_bucket(K, d, quads);
    mine = band_word_bytes(d, K, kind);
  }
  ScanPart w;
  for (int b = 0; b < 4; ++b) w.n[b] = (uint32_t)__popcll(__ballot(bucket == b));
  w.bytes = s_wave_sum(mine);
  if (L == 0) s_w[wv] = w;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = s_waves_before(s_w, kScanWaves);
}
// count: the lists' sizes for the launch; stat: added up for the call's statistics -- `tracy align` runs a stage twice, over the early
// traces and over the rest (both written by the last block, whose base plus its own totals they are)
__global__ __launch_bounds__(kScanBlock) void s_scan_place_kernel(PairDesc* __restrict__ cand, uint8_t* __restrict__ kc, uint32_t n, uint32_t unit_mod, int kind,
                                                                  int quads, unsigned long long cap_bytes, const ScanPart* __restrict__ part, uint32_t* __restrict__ idx,
                                                                  uint32_t* __restrict__ dead, uint32_t* __restrict__ count, unsigned long long* __restrict__ stat,
                                                                  int prio) {
  wave_prio(prio);
  __shared__ ScanPart s_base[kScanWaves];  // per wave: its share of the totals of the blocks before this one ...
  __shared__ ScanPart s_w[kScanWaves];     // ... and what its own 64 units add
  __shared__ unsigned long long s_stat[SB_LIST];  // (the lists' sizes are the last block's)
  const uint32_t tid = threadIdx.x, wv = tid >> 6, L = tid & 63u;
  if (tid < SB_LIST) s_stat[tid] = 0;
  ScanPart before{{0, 0, 0, 0}, 0};
  for (uint32_t j = tid; j < blockIdx.x; j += kScanBlock) {
    const ScanPart x = part[j];
    for (int b = 0; b < 4; ++b) before.n[b] += x.n[b];
    before.bytes += x.bytes;
  }
  for (int b = 0; b < 4; ++b) before.n[b] = s_wave_sum(before.n[b]);
  before.bytes = s_wave_sum(before.bytes);
  const uint32_t i = blockIdx.x * kScanBlock + tid;
  const int K = i < n ? kc[i] : 0;
  PairDesc d{};
  unsigned long long mine = 0;
  Credit credit{0, 0};  // (what BandTally::add credits a pair of run_band16; before the word bytes, which then share its divisions)
  if (K) { d = cand[i]; credit = band_credit(d, K, kind); mine = band_word_bytes(d, K, kind); }
  const int bucket = K ? s_bucket(K, d, quads) : -1;
  const unsigned long long below = (1ull << L) - 1ull;
  ScanPart w;
  uint32_t rank = 0;  // pairs of my list in the lanes below me
  for (int b = 0; b < 4; ++b) {
    const unsigned long long bal = __ballot(bucket == b);
    w.n[b] = (uint32_t)__popcll(bal);
    if (bucket == b) rank = (uint32_t)__popcll(bal & below);
  }
  unsigned long long incl = mine;  // inclusive scan of the bytes over the wave
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(incl, o, 64);
    if (L >= (uint32_t)o) incl += y;
  }
  w.bytes = __shfl(incl, 63, 64);
  if (L == 0) { s_base[wv] = before; s_w[wv] = w; }
  __syncthreads();
  const ScanPart base = s_waves_before(s_base, kScanWaves), lower = s_waves_before(s_w, wv);
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    const ScanPart all = s_waves_before(s_w, kScanWaves);
    for (int b = 0; b < 4; ++b) {
      count[b] = base.n[b] + all.n[b];
      stat[SB_LIST + b] += base.n[b] + all.n[b];
    }
  }
  if (K) {
    const int b = bucket;
    uint32_t pos = rank;  // (not base.n[b]: a record indexed by a variable moves to LDS, s_orient_early_kernel)
    for (int k = 0; k < 4; ++k) pos += b == k ? base.n[k] + lower.n[k] : 0u;
    const unsigned long long off = base.bytes + lower.bytes + incl - mine;
    idx[(size_t)b * n + pos] = i;  // (the list stays dense: a dropped pair keeps its slot as an empty one)
    if (off + mine > cap_bytes) {  // (never for kind 1)
      kc[i] = 0;
      cand[i].flags = d.flags | PAIR_SKIP;
      atomicOr(dead + (i % unit_mod), SD_MEM);
    } else {
      cand[i].bits_off = off;
      atomicAdd(&s_stat[SB_CELLS], (unsigned long long)credit.cells);
      atomicAdd(&s_stat[SB_BYTES], (unsigned long long)credit.bytes);
      atomicAdd(&s_stat[2], mine);
      atomicAdd(&s_stat[SB_HIST + s_width_bucket(band_dmin(d), band_dmax(d))], 1ull);
    }
  }
  __syncthreads();
  if (tid < SB_LIST && s_stat[tid]) atomicAdd(stat + tid, s_stat[tid]);
}

// ---- `tracy align`: trimReferenceSlice from the two ends (sage.h:259) and the plan of the final alignment gotoh(full profile,
// trimmed slice) on its certified band (sage.h:311; pipeline.hip step 4; s_final_band, s_final_certified); `early` as above ----
__global__ void s_align_final_plan_kernel(SParams p, int early, const SGeom* __restrict__ geom, STrace* __restrict__ tr, const uint32_t* __restrict__ ends,
                                          uint32_t* __restrict__ dead, PairDesc* __restrict__ cand, uint8_t* __restrict__ kc,
                                          unsigned long long* __restrict__ cnt, int prio) {
  wave_prio(prio);
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  kc[t] = 0;
  STrace S = tr[t];
  if (((S.mark & ST_EARLY) != 0u) != (early != 0)) return;
  if (dead[t]) return;
  const SGeom G = geom[t];
  const uint32_t lead = ends[2 * t] + S.shift, ce = ends[2 * t + 1] + S.shift;
  S.trim = s_trim_finish(lead, ce >= lead ? ce - lead : 0u, G.rn, G.rl, G.rr, S.fwd != 0);
  s_count(lc, SC_PRELIM_BANDED);
  if (early) S.mark |= ST_COUNTED_PRELIM;
  const uint32_t m = G.mf, n = S.trim.len;
  const SFinalBand fb = s_final_band(m, n, s_final_width(S.gap));
  uint32_t dd = 0;
  if (!fb.K) dd = SD_FINAL_BAND;
  else if (n > p.ncap) dd = SD_SHAPE;
  else {
    S.bw = (int32_t)fb.w;
    PairDesc q{};
    q.a1_off = G.tab_off;
    q.a1_stride = G.tab_stride;
    q.m = m;
    q.n = n;
    q.a2_stride = n;
    // oriented slice [ri, ri + len): forward reads it in place, reverse reads [n - ri - len, n - ri) backwards with complemented codes
    q.a2_off = G.ref_off + (S.rc ? G.rn - S.trim.ri - S.trim.len : S.trim.ri);
    q.flags = S.rc ? PAIR_A2_REVCOMP : 0u;
    q.out = t;
    q.ckpt_off = band_pack(fb.dlo, fb.dhi);
    cand[t] = q;
    kc[t] = (uint8_t)fb.K;
    s_count(lc, SC_FINAL_BANDED);
    if (early) S.mark |= ST_COUNTED_FINAL;
  }
  // (not tr[t] = S: the fields this kernel only carries -- sc, sstar, ce -- then stay a 16-byte record per thread that the compiler
  // keeps in LDS, 16 KB per workgroup of a kernel that declares 184 bytes: see s_orient_early_kernel)
  tr[t].bw = S.bw;
  tr[t].mark = S.mark;
  tr[t].trim = S.trim;
  if (dd) dead[t] |= dd;
  });
}

// the band certificate of the final alignment (S_b > top - |ge| (W + 1): no path outside reaches S_b) and the per-trace results
struct AlignOutDev {
  int32_t *score_fwd, *score_rev, *score_prelim, *score_final;
  uint8_t* forward;
  uint32_t *slice_begin, *slice_len, *ref_pos, *ops_len;
};
__global__ void s_align_finish_kernel(SParams p, const STrace* __restrict__ tr, const int32_t* __restrict__ top_full, uint32_t* __restrict__ dead,
                                      AlignOutDev o, unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  if (dead[t]) return;
  const STrace S = tr[t];
  if (!s_final_certified(o.score_final[t], top_full[t], p.ge, S.bw, o.ops_len[t])) {
    dead[t] |= SD_FINAL_CHECK;
    s_count(lc, SC_FINAL_REPEATED);
    return;
  }
  o.score_fwd[t] = S.sc[0];
  o.score_rev[t] = S.sc[1];
  o.forward[t] = S.fwd;
  if (o.score_prelim) o.score_prelim[t] = S.sstar;
  o.slice_begin[t] = S.trim.ri;
  o.slice_len[t] = S.trim.len;
  o.ref_pos[t] = S.trim.pos;
  });
}

// results of the dead traces, computed by the host-planned pipeline into compact arrays, back to their places
struct Frac2 { double a, b; };  // (allelicFraction's two doubles of a trace move as one element)
template <class T>
__global__ void s_scatter_kernel(const uint32_t* __restrict__ list, uint32_t n, const T* __restrict__ src, T* __restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && dst) dst[list[i]] = src[i];
}
template <class T>
int scatter(hipStream_t st, const uint32_t* d_list, uint32_t n, const T* src, T* dst) {
  if (!dst || n == 0) return TRACYHIP_OK;
  hipLaunchKernelGGL(s_scatter_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, st, d_list, n, src, dst);
  HIP_TRY(hipGetLastError());
  return TRACYHIP_OK;
}

// ---- host side shared by the two pipelines ----
struct SweepClass { int K; uint32_t lo, hi; };  // traces [lo, hi) of the sweep order share strip height K

struct StreamCommon {  // device arrays of the orientation stage + preliminary alignment
  SGeom* geom;
  VoteDesc* vd;
  RowMaxDesc *rm_rest, *rm_trim, *rm_full;
  B16TableDesc* td;
  uint32_t* votes;
  int32_t *ub, *ub1, *top_trim, *top_full;
  int32_t* sc2;
  PairDesc *full, *pre, *fpairs0, *fpairs1, *fpairs2, *cand;
  FrontDesc* fd;
  FrontOut *fo0, *fo1, *fo2;
  int32_t *fs0, *fs1, *fs2;
  uint32_t *fe0, *fe1, *fe2;
  STrace* tr;
  RowEndDesc* re;
  uint32_t* ce;
  uint32_t* dead;
  uint8_t* kc;
  uint32_t* idx;
  ScanPart* part;            // the scan's block totals
  uint32_t* count;           // [4] per band stage
  uint32_t* flist;           // pruned sweeps: the units a later tier still has to take (s_front_list_kernel) ...
  uint32_t* fcount;          // ... and how many: [0] for the first wide tier behind the quads, [1] for the last tier; [2]: the allele prefixes' list
  unsigned long long* cnt;   // [SC_COUNT]
  unsigned long long* bstat; // [SB_COUNT] per band stage
  uint32_t* ends;
  uint32_t large_stages = 0; // (host) band stages of the call that took the large form (launch_band16_counted)
  void layout(Arena& a, uint32_t nt, uint32_t nunits, bool exact, bool want_full_top) {
    geom = a.take<SGeom>(nt);
    vd = a.take<VoteDesc>(nt);
    rm_rest = a.take<RowMaxDesc>(nt);
    rm_trim = a.take<RowMaxDesc>(nt);
    rm_full = want_full_top ? a.take<RowMaxDesc>(nt) : nullptr;
    td = a.take<B16TableDesc>(nt);
    votes = a.take<uint32_t>(2 * (size_t)nt);
    ub = a.take<int32_t>(nt);
    ub1 = a.take<int32_t>(nt);
    top_trim = a.take<int32_t>(nt);
    top_full = want_full_top ? a.take<int32_t>(nt) : nullptr;
    sc2 = a.take<int32_t>(2 * (size_t)nt);
    full = a.take<PairDesc>(2 * (size_t)nt);
    pre = a.take<PairDesc>(std::max<size_t>((exact ? 1 : 2) * (size_t)nt, nunits));  // (`tracy decompose` lays the allele prefixes out here later)
    fpairs0 = a.take<PairDesc>(nunits);
    fpairs1 = a.take<PairDesc>(nunits);
    fpairs2 = a.take<PairDesc>(nunits);
    cand = a.take<PairDesc>(nunits);
    fd = a.take<FrontDesc>(nunits);
    fo0 = a.take<FrontOut>(nunits);
    fo1 = a.take<FrontOut>(nunits);
    fo2 = a.take<FrontOut>(nunits);
    fs0 = a.take<int32_t>(nunits);
    fs1 = a.take<int32_t>(nunits);
    fs2 = a.take<int32_t>(nunits);
    fe0 = a.take<uint32_t>(2 * (size_t)nunits);
    fe1 = a.take<uint32_t>(2 * (size_t)nunits);
    fe2 = a.take<uint32_t>(2 * (size_t)nunits);
    tr = a.take<STrace>(nt);
    re = a.take<RowEndDesc>(nt);
    ce = a.take<uint32_t>(nt);
    dead = a.take<uint32_t>(nt);
    kc = a.take<uint8_t>(nunits);
    idx = a.take<uint32_t>(4 * (size_t)nunits);
    part = a.take<ScanPart>((nunits + kScanBlock - 1) / kScanBlock + 1);
    count = a.take<uint32_t>(4 * 8);
    flist = a.take<uint32_t>(nunits);
    fcount = a.take<uint32_t>(4);
    cnt = a.take<unsigned long long>(SC_COUNT);
    bstat = a.take<unsigned long long>(SB_COUNT * 8);
    ends = a.take<uint32_t>(2 * (size_t)nunits);
  }
};

// what the host works out from the job alone
struct StreamHost {
  std::vector<uint32_t> mf, mt, tl, rn, ridx;
  uint32_t nt = 0;
  std::vector<SweepClass> classes;
  uint64_t lr_tot = 0, tab_tot = 0;
  uint32_t maxmt = 0, maxmf = 0, max_rest = 0;
  uint64_t max_mn = 0;
};

// the order of the full sweeps: run_dp's (order_sweeps, dp_plan.h; no flag: profile x code), and like it none when the batch is of a
// size (`similar`: the SizeSpan of the caller's pass over the lengths) -- then the order is the traces' own and `order` stays empty
void sweep_order(StreamHost& h, std::vector<uint32_t>& order, const std::vector<int>& kof, bool similar) {
  const uint32_t nt = h.nt;
  h.classes.clear();
  order.clear();
  if (similar) {
    if (nt) h.classes.push_back(SweepClass{kof[0], 0u, nt});
    return;
  }
  order_sweeps(nt, [&](uint32_t t) { return SweepKey{kof[t], 0u, (uint64_t)h.mt[t] * h.rn[t]}; }, false, order);
  for (uint32_t i = 0; i < nt;) {
    uint32_t e = i;
    while (e < nt && kof[order[e]] == kof[order[i]]) ++e;
    h.classes.push_back(SweepClass{kof[order[i]], i, e});
    i = e;
  }
}

bool stream_options_ok(const CtxKnobs& k) {
  return !k.no_stream && !k.no_narrow && !k.no_band && !k.no_band16 && !k.no_front && !k.no_prefix && !k.no_vote && !k.no_origin &&
         !k.no_subwindow && !k.no_prelim_origin && !k.no_cq && k.band_w < 0;
}

}  // namespace
// workspace one context may plan with (run_dp's rule): the caller's limit, or its share of what is free plus what it holds
int tracyhip::workspace_budget(tracyhip_ctx* ctx, uint64_t held, uint64_t* out, bool* from_cache) {
  if (from_cache) *from_cache = false;
  if (ctx->ws_limit) { *out = ctx->ws_limit; return TRACYHIP_OK; }
  // (hipMemGetInfo is a driver round trip, paid while the device waits for the call to be planned: the answer is kept for as long as
  // the context holds what it held when it asked -- a call of the same shape as the last one.  Free memory can shrink behind the
  // context's back -- another allocator in the process, another process: a plan made from a kept answer whose allocations fail is
  // made again from a fresh one, with_fresh_budget below)
  if (ctx->ws_cache_budget && ctx->ws_cache_held == held && ctx->ws_cache_share == ctx->mem_share) {
    *out = ctx->ws_cache_budget;
    if (from_cache) *from_cache = true;
    return TRACYHIP_OK;
  }
  TRY(workspace_limit(ctx, held, out));
  ctx->ws_cache_budget = *out; ctx->ws_cache_held = held; ctx->ws_cache_share = ctx->mem_share;
  return TRACYHIP_OK;
}
namespace {
// plan(&from_cache) sizes and allocates a call's workspace from workspace_budget's answer: when the answer was a kept one and an
// allocation fails, the kept answer is dropped and the plan is made once more from what the driver says is free now
template <class Plan>
int with_fresh_budget(tracyhip_ctx* ctx, Plan plan) {
  bool from_cache = false;
  int rc = plan(&from_cache);
  if (rc == TRACYHIP_ERR_OOM && from_cache) {
    (void)hipGetLastError();  // (the failed allocation's sticky error)
    ctx->ws_cache_budget = 0;
    rc = plan(&from_cache);
  }
  return rc;
}

DpArgs sweep_args(tracyhip_ctx* ctx, const tracyhip_params& p, const void* d_a1, const void* d_a2, int32_t* d_scores, int32_t* d_lastrow) {
  DpArgs a = scoring_args(ctx, &p);
  a.a1 = d_a1; a.a2 = d_a2; a.scores = d_scores;
  a.ckpt = d_lastrow;  // (never written: row m only)
  a.lastrow = d_lastrow;
  a.ckpt_B = 0x7fffffffu;
  a.ckpt_narrow = 1;
  return a;
}

// LDS of the wide tiers' band launches for the longest rest of the batch: tested by the planners BEFORE anything of a call is queued (a
// tier that finds no room once launches are in flight would hand the call back with the workspace still in use)
bool front_tiers_fit(uint32_t max_rest) { return front_tier_fits(kFrontK1, kFrontHalfW1, max_rest) && front_tier_fits(kFrontK, kFrontHalfW, max_rest); }

// one tier of the pruned sweep over fixed slots: place, band below the kept row, certify (capi.hip run_front_once)
// KB = 0: the quad form (strips of four rows, four lanes per pair) -- the narrow tier ahead of the others
int front_tier(tracyhip_ctx* ctx, const tracyhip_params& p, const FrontDesc* fd, uint32_t n, const int16_t* d_qp, const uint8_t* d_codes, const uint32_t* d_row,
               int KB, int32_t halfw, uint32_t max_rest, PairDesc* pairs, FrontOut* fo, int32_t* fs, uint32_t* fe, const FrontOut* prev,
               const uint32_t* list, const uint32_t* list_count) {
  hipStream_t st = ctx->stream;
  Band16Args a{};
  a.pairs = pairs; a.npairs = n; a.index = list; a.count = list_count; a.qp = d_qp; a.codes = d_codes; a.scores = fs; a.ends = fe;
  a.err = static_cast<int32_t*>(ctx->dev[DB_ERR].p); a.go = p.go; a.ge = p.ge; a.hfree = 1; a.row = d_row;
  const int prio = queued_prio(ctx, 1);
  a.prio = prio;
  a.code_cap = front_code_cap(max_rest, halfw);
  if (KB == 0) {
    if (b16_cont_quad_lds(a.code_cap) > kBandLdsHard) return kStreamNo;  // (front_tiers_run goes on with the wide tiers: nothing was queued for this one)
  } else if (!front_tier_fits(KB, halfw, max_rest)) return set_error(TRACYHIP_ERR_ARG, "pruned-sweep tier without LDS room (front_tiers_fit not consulted)");
  HIP_TRY(launch_front_place(fd, n, d_row, p.go + p.ge, halfw, pairs, fo, st, prev, list, list_count, prio));
  if (KB == 0) HIP_TRY(launch_band16_cont_quad(a, st));
  else HIP_TRY(launch_band16_cont(KB, a, st, !ctx->knobs.no_cont16));
  HIP_TRY(launch_front_certify(fd, n, d_row, p.go, p.ge, halfw, fs, fe, fo, st, prev, list, list_count, prio));
  return TRACYHIP_OK;
}

// the units an earlier tier did not certify as a list for the next tier's three launches: a band launch runs as long as its slowest
// wave and a wave as long as the widest of its four pairs, so units skipped in place leave most waves as they were (one in four
// certified: 0.4 % of the waves empty), whereas a list shortens the launch by what was certified.  The order of the list is whichever
// workgroup adds its part first; results go to the units' own slots, so nothing depends on it.
__device__ __forceinline__ void s_list_append(bool take, uint32_t i, uint32_t* __restrict__ list, uint32_t* __restrict__ count) {  // (blocks of 256 threads, all of them)
  __shared__ uint32_t wave_n[4], base;
  const uint32_t wv = threadIdx.x >> 6, L = threadIdx.x & 63u;
  const unsigned long long bal = __ballot(take);
  if (L == 0) wave_n[wv] = (uint32_t)__popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    base = tot ? atomicAdd(count, tot) : 0u;
  }
  __syncthreads();
  if (!take) return;
  uint32_t at = base + (uint32_t)__popcll(bal & ((1ull << L) - 1ull));
  for (uint32_t k = 0; k < wv; ++k) at += wave_n[k];
  list[at] = i;
}
// (a unit left off the list is not visited by the next tier's place / band / certify launches: its slot of that tier is marked "not
// certified here" explicitly -- consumers read the earlier tier's verdict first, but the slot must not keep a verdict of another call)
__global__ __launch_bounds__(256) void s_front_list_kernel(uint32_t n, const FrontOut* __restrict__ prev, uint32_t* __restrict__ list, uint32_t* __restrict__ count,
                                                           FrontOut* __restrict__ next, int prio) {
  wave_prio(prio);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool take = i < n && !prev[i].ok;
  if (i < n && !take) next[i].ok = 0u;
  s_list_append(take, i, list, count);
}
// ... and the pairs of a launch that take part in it (a prefix launch whose pairs partly share their kept rows: s_allele_plan0_kernel)
__global__ __launch_bounds__(256) void s_pair_list_kernel(uint32_t n, const PairDesc* __restrict__ pairs, uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  s_list_append(i < n && !(pairs[i].flags & PAIR_SKIP), i, list, count);
}
hipError_t front_list(tracyhip_ctx* ctx, uint32_t n, const FrontOut* prev, uint32_t* list, uint32_t* count, FrontOut* next) {
  hipLaunchKernelGGL(s_front_list_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, prev, list, count, next, queued_prio(ctx, 1));
  return hipGetLastError();
}

// what the narrow tier certified goes into the first wide tier's slots (which skipped it): everything after reads two tiers
__global__ void s_front_fold_kernel(uint32_t n, const FrontOut* __restrict__ fo0, const int32_t* __restrict__ fs0, const uint32_t* __restrict__ fe0,
                                    FrontOut* __restrict__ fo1, int32_t* __restrict__ fs1, uint32_t* __restrict__ fe1, int prio) {
  wave_prio(prio);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !fo0[i].ok) return;
  fo1[i] = fo0[i];
  fs1[i] = fs0[i];
  fe1[2 * i] = fe0[2 * i];
  fe1[2 * i + 1] = fe0[2 * i + 1];
}
int front_tiers_run_wide(tracyhip_ctx* ctx, const tracyhip_params& p, StreamCommon& sc, uint32_t n, const int16_t* d_qp, const uint8_t* d_codes,
                         const uint32_t* d_row, uint32_t max_rest, bool after_quads) {
  // (a list costs one more small launch in the chain: worth it from a few waves per SIMD on)
  const bool lists = !ctx->knobs.no_front_lists && n >= ctx->knobs.front_list_min;
  if (lists) HIP_TRY(hipMemsetAsync(sc.fcount, 0, 2 * sizeof(uint32_t), ctx->stream));
  const bool list1 = lists && after_quads;
  if (list1) HIP_TRY(front_list(ctx, n, sc.fo0, sc.flist, sc.fcount, sc.fo1));  // (what the quads certified is folded into fo1 below)
  int rc = front_tier(ctx, p, sc.fd, n, d_qp, d_codes, d_row, kFrontK1, kFrontHalfW1, max_rest, sc.fpairs1, sc.fo1, sc.fs1, sc.fe1, after_quads ? sc.fo0 : nullptr,
                      list1 ? sc.flist : nullptr, list1 ? sc.fcount : nullptr);
  if (rc) return rc;
  if (after_quads) {
    hipLaunchKernelGGL(s_front_fold_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, sc.fo0, sc.fs0, sc.fe0, sc.fo1, sc.fs1, sc.fe1, queued_prio(ctx, 1));
    HIP_TRY(hipGetLastError());
  }
  // (the first list has been read by the tier above: the same array holds the second)
  if (lists) HIP_TRY(front_list(ctx, n, sc.fo1, sc.flist, sc.fcount + 1, sc.fo2));
  return front_tier(ctx, p, sc.fd, n, d_qp, d_codes, d_row, kFrontK, kFrontHalfW, max_rest, sc.fpairs2, sc.fo2, sc.fs2, sc.fe2, sc.fo1,
                    lists ? sc.flist : nullptr, lists ? sc.fcount + 1 : nullptr);
}
constexpr int32_t kQuadHalfW = 5;  // c* +- 5: eleven diagonals, a window of three blocks of strip height 4 (b16_narrow_ok)

// the tiers of a pruned sweep over `n` units: the quad tier (a trace that loses less than |ge| (5 + 1) below the kept row certifies
// there, at a quarter of the lanes), strips of 8 rows on c* +- 60 for the rest, then the widest band one period holds (run_front)
int front_tiers_run(tracyhip_ctx* ctx, const tracyhip_params& p, StreamCommon& sc, uint32_t n, const int16_t* d_qp, const uint8_t* d_codes, const uint32_t* d_row,
                    uint32_t max_rest) {
  // (a tier is three launches of a wave's depth each: worth their latency where the wide tier's launch is long -- 100 000 units
  // -2.5 ms, 12 500 units +0.3 ms measured)
  const bool quads = !ctx->knobs.no_quads && n >= ctx->knobs.quad_tier_min;
  int rc = TRACYHIP_OK;
  if (quads) rc = front_tier(ctx, p, sc.fd, n, d_qp, d_codes, d_row, 0, kQuadHalfW, max_rest, sc.fpairs0, sc.fo0, sc.fs0, sc.fe0, nullptr, nullptr, nullptr);
  if (rc == kStreamNo && quads) return front_tiers_run_wide(ctx, p, sc, n, d_qp, d_codes, d_row, max_rest, false);
  if (rc) return rc;
  return front_tiers_run_wide(ctx, p, sc, n, d_qp, d_codes, d_row, max_rest, quads);
}

// a band launch over the candidates of `n` units: lists per strip height (scan), the three heights (sizes read on the device)
struct BandStageArgs {
  int kind = 0;
  const int16_t* qp = nullptr;
  const uint8_t* codes = nullptr;
  int32_t* scores = nullptr;
  uint32_t* ends = nullptr;
  uint8_t* ops = nullptr;
  const uint64_t* ops_off = nullptr;
  uint32_t* ops_len = nullptr;
  uint32_t code_cap = 0;
  int hfree = 1;
};
int band_stage(tracyhip_ctx* ctx, const tracyhip_params& p, StreamCommon& sc, uint32_t n, uint32_t unit_mod, int stage_no, const BandStageArgs& bl, uint64_t cap_bytes) {
  hipStream_t st = ctx->stream;
  uint32_t* count = sc.count + 4 * stage_no;
  const uint32_t nb = (n + kScanBlock - 1) / kScanBlock;
  const int quads = (!ctx->knobs.no_quads && b16_quad_lds(bl.code_cap) <= kBandLdsHard) ? 1 : 0;  // the narrow bands four lanes to a pair, where sixteen code rows fit
  const int prio = queued_prio(ctx, 2);
  hipLaunchKernelGGL(s_scan_count_kernel, dim3(nb), dim3(kScanBlock), 0, st, sc.cand, sc.kc, n, bl.kind, quads, sc.part, prio);
  hipLaunchKernelGGL(s_scan_place_kernel, dim3(nb), dim3(kScanBlock), 0, st, sc.cand, sc.kc, n, unit_mod, bl.kind, quads, (unsigned long long)cap_bytes, sc.part, sc.idx, sc.dead,
                     count, sc.bstat + SB_COUNT * stage_no, prio);
  HIP_TRY(hipGetLastError());
  Band16Args a{};
  a.prio = prio;
  a.pairs = sc.cand; a.npairs = n; a.qp = bl.qp; a.codes = bl.codes; a.bits = static_cast<uint8_t*>(ctx->dev[DB_BITS].p); a.scores = bl.scores; a.ends = bl.ends;
  a.err = static_cast<int32_t*>(ctx->dev[DB_ERR].p); a.go = p.go; a.ge = p.ge; a.hfree = bl.hfree;
  a.ops = bl.ops; a.ops_off = bl.ops_off; a.ops_len = bl.ops_len; a.code_cap = bl.code_cap;
  Band16Args ak[4] = {a, a, a, a};  // 12, 8, 4, 4 in quads
  for (int b = 0; b < 4; ++b) { ak[b].index = sc.idx + (size_t)b * n; ak[b].count = count + b; }
  if (!quads) ak[3].npairs = 0;
  TRY(timing_begin(ctx, bl.kind == 0 ? TRACYHIP_TIMER_TRACE : TRACYHIP_TIMER_ORIGIN, 0, 0));  // (cells / bytes: the scan's sums, added after the call's synchronisation)
  bool large = false;
  HIP_TRY(launch_band16_counted(bl.kind, ak[0], ak[1], ak[2], ak[3], st, (ctx->b16_fork_ok && !ctx->knobs.no_fork) ? &ctx->b16_fork : nullptr,
                                ctx->knobs.b16_multi_max, &large));
  if (large) ++sc.large_stages;
  TRY(timing_end(ctx));
  return TRACYHIP_OK;
}

// Bytes of traceback words planned for a band launch over `npairs` pairs of `rows` rows in total.  The words of a pair depend on the
// band its score allows -- known on the device only -- so the workspace holds the widest window of every pair (130 bytes per row:
// 12-row strips of 195 steps, 8 bytes each), or half of what the context may still plan with when that is less.  A pair that does
// not fit is dropped by the scan (SD_MEM) and taken by the host-planned tiers, which chunk.
uint64_t band_words_cap(uint64_t rows, uint64_t npairs, uint64_t budget_left) {
  const uint64_t worst = rows * 131 + npairs * 10240;
  return std::max<uint64_t>(std::min(worst, budget_left / 2), 1ull << 20);
}
// orientation stage + c_e of the winner, queued (both pipelines)
struct OrientStage {
  const void* d_prof;
  const int16_t* d_qp;     // tables of the full profiles
  int32_t* d_lastrow;
  bool exact;
  PairDesc* desc_trim;     // `tracy decompose`, or null
  // or work of the call that depends on nothing the orientation stage makes: queued on the call's stream behind the full sweeps, BEFORE
  // the stream waits for the voted strand's chain -- whose band tiers, launches of a few waves' depth, only get going when the sweeps drain
  // (they need 15-20 KB of LDS per workgroup; the sweeps' 7.5 KB workgroups leave no such hole) and leave the device nearly idle for 3-4 ms
  std::function<int()> filler;
  // or stages of the call that need nothing of a trace but its voted strand's certified pruned sweep (`tracy align`: the preliminary and
  // final alignments of the traces s_orient_early_kernel marks): queued on the voted strand's side stream behind its tiers, with the
  // context's stream set to it (and its queue priority: what the hook queues there is tier 2 of queued_prio), BEFORE the call's stream
  // waits for that chain -- so they run beside the end of the full sweeps instead of on a drained device behind them.  Only called with side streams; the caller queues the same stages for the other traces itself,
  // behind the decision.
  std::function<int()> early_tail;
};
int queue_orientation(tracyhip_ctx* ctx, const tracyhip_params& p, const SParams& sp, const StreamHost& h, StreamCommon& sc, const OrientStage& os) {
  hipStream_t st = ctx->stream;
  const uint32_t nt = h.nt;
  const dim3 g256((nt + 255) / 256), b256(256);
  const float* prof = static_cast<const float*>(os.d_prof);
  hipLaunchKernelGGL(s_expand_kernel, g256, b256, 0, st, sc.geom, nt, sc.vd, sc.rm_rest, sc.rm_trim, sc.rm_full, sc.td);
  HIP_TRY(hipGetLastError());
  // the substitution tables and the row maxima need the profiles only, the k-mer vote the profiles and the codes: side by side (the vote
  // holds 22 KB of LDS per workgroup and waits for memory most of the time; the others use none)
  const bool prep_fork = ctx->b16_fork_ok && !ctx->knobs.no_fork;
  hipStream_t sp1 = st;
  if (prep_fork) {
    HIP_TRY(hipEventRecord(ctx->b16_fork.forked, st));
    HIP_TRY(hipStreamWaitEvent(ctx->b16_fork.side[1], ctx->b16_fork.forked, 0));
    sp1 = ctx->b16_fork.side[1];
    ctx->stream = sp1;
  }
  {
    int rc = timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, h.tab_tot * 2);
    hipError_t e = hipSuccess;
    if (!rc) {
      e = launch_b16_tables(sc.td, nt, os.d_prof, false, p.match, p.mismatch, sub_limit(&p), kTagShift, const_cast<int16_t*>(os.d_qp),
                            static_cast<int32_t*>(ctx->dev[DB_ERR].p), sp1);
      rc = timing_end(ctx);
    }
    ctx->stream = st;
    hipLaunchKernelGGL(rowmax_rest_kernel, dim3(nt), dim3(64), 0, sp1, sc.rm_rest, prof, (float)p.match, (float)p.mismatch, sc.ub, sc.ub1);
    hipLaunchKernelGGL(rowmax_rest_kernel, dim3(nt), dim3(64), 0, sp1, sc.rm_trim, prof, (float)p.match, (float)p.mismatch, sc.top_trim, (int32_t*)nullptr);
    if (sc.rm_full) hipLaunchKernelGGL(rowmax_rest_kernel, dim3(nt), dim3(64), 0, sp1, sc.rm_full, prof, (float)p.match, (float)p.mismatch, sc.top_full, (int32_t*)nullptr);
    hipLaunchKernelGGL(kmer_vote_kernel, dim3(nt), dim3(64), 0, st, sc.vd, prof, ctx->codes(), sc.votes);
    if (prep_fork) {  // (joined on every way out)
      HIP_TRY(hipEventRecord(ctx->b16_fork.joined[1], sp1));
      HIP_TRY(hipStreamWaitEvent(st, ctx->b16_fork.joined[1], 0));
    }
    if (rc) return rc;
    HIP_TRY(e);
  }
  hipLaunchKernelGGL(s_orient_plan_kernel, g256, b256, 0, st, sp, sc.geom, sc.votes, sc.ub, sc.ub1, sc.full, sc.pre, sc.fd, sc.tr, sc.cnt);
  HIP_TRY(hipGetLastError());
  // ONE launch per strip height: full sweeps of the class + (with the first) the prefixes of every trace
  DpArgs a = sweep_args(ctx, p, os.d_prof, ctx->codes(), sc.sc2, os.d_lastrow);
  if (!ctx->knobs.no_compact) a.special_blocks = ctx->special_blocks();
  if (sp.use_votes) { a.votes = sc.votes; a.vote_nt = nt; }
  DpArgs ap = a;
  ap.pairs = sc.pre;
  ap.votes = nullptr;
  const uint32_t npre_all = (os.exact ? 1u : 2u) * nt;
  // the pruned sweep of the voted strands: strips of 8 rows on c* +- 60, then the widest band one period holds for what failed (run_front)
  auto front_tiers = [&]() -> int {
    TRY(timing_begin(ctx, TRACYHIP_TIMER_FRONT, 0, 0));
    const int rc = front_tiers_run(ctx, p, sc, nt, os.d_qp, ctx->codes(), reinterpret_cast<const uint32_t*>(os.d_lastrow), h.max_rest);
    const int rc2 = timing_end(ctx);  // (begun: ended whatever the tiers say)
    return rc ? rc : rc2;
  };
  if (ctx->b16_fork_ok && !ctx->knobs.no_fork) {
    // Two strands, two streams.  The voted strand's chain -- its 128-row prefixes, then the band tiers below the kept row: launches
    // of a few waves' depth each, which on their own last as long as their slowest wave -- runs beside the other strand's full
    // sweeps, which fill the device for the whole stage anyway; the decision waits for both.  (The two write different rows of
    // the row-m workspace and different score slots, as they do inside one launch.)
    const B16Fork& fk = ctx->b16_fork;
    HIP_TRY(hipEventRecord(fk.forked, st));
    HIP_TRY(hipStreamWaitEvent(fk.side[0], fk.forked, 0));
    ctx->stream = fk.side[0];  // (timers and front_tier queue on the context's stream)
    // (the prefixes are not timed on their own: they begin with the sweeps and end inside them, and their cells stay credited to the
    // sweep timer, whose interval covers both launches as it covered the one)
    int rc = TRACYHIP_OK;
    {
      DpArgs af = a, apl = ap;
      launch_diag_periods(ctx, &p, h.classes[0].K, 0u, npre_all, true, af, apl);
      // (beside the other strands' full sweeps the device is full whatever this launch's depth: the shape with fewer instructions per cell)
      const uint32_t tall_min = (os.exact && !ctx->knobs.no_prefix_tall_beside) ? 0u : ctx->knobs.prefix_tall_min;
      if (launch_gotoh_ckpt_front(h.classes[0].K, af, 0u, apl, npre_all, fk.side[0], tall_min) != hipSuccess) rc = set_error(TRACYHIP_ERR_HIP, "prefix launch failed");
    }
    // What is queued on the side stream from here on raises its waves' priority as option chain_prio says (queued_prio): the waves of
    // the tiers and of the early tail are the youngest on SIMDs the sweeps keep busy, and a SIMD issues by priority, then by age.  The
    // prefixes above stay at the sweeps' priority, and so does everything queued behind the decision.
    ctx->queue_prio = ctx->knobs.chain_prio;
    if (!rc) rc = front_tiers();
    if (!rc && os.early_tail) {
      hipLaunchKernelGGL(s_orient_early_kernel, g256, b256, 0, fk.side[0], sp, sc.fo1, sc.fs1, sc.fe1, sc.fo2, sc.fs2, sc.fe2, sc.tr, queued_prio(ctx, 1));
      if (hipGetLastError() != hipSuccess) rc = set_error(TRACYHIP_ERR_HIP, "early decision launch failed");
      else rc = os.early_tail();
    }
    ctx->queue_prio = 0;  // (with the stream, on every way out: front_tiers and early_tail hand their status back)
    ctx->stream = st;
    HIP_TRY(hipEventRecord(fk.joined[0], fk.side[0]));
    if (rc) {  // (whoever takes the call from here finds nothing of it running beside the call's stream)
      HIP_TRY(hipStreamWaitEvent(st, fk.joined[0], 0));
      return rc;
    }
    if (ctx->knobs.sweeps_alone) HIP_TRY(hipStreamWaitEvent(st, fk.joined[0], 0));  // (measurement: the full sweeps on a device of their own)
    auto sweeps = [&]() -> int {
      for (const SweepClass& c : h.classes) {
        DpArgs af = a;
        af.pairs = sc.full + 2 * (size_t)c.lo;
        DpArgs apl = ap;
        launch_diag_periods(ctx, &p, c.K, 2 * (c.hi - c.lo), 0u, true, af, apl);
        TRY(timing_begin(ctx, TRACYHIP_TIMER_SCORE, 0, 0));
        const hipError_t e = launch_gotoh_ckpt_front(c.K, af, 2 * (c.hi - c.lo), apl, 0u, st, ctx->knobs.prefix_tall_min);
        TRY(timing_end(ctx));
        HIP_TRY(e);
      }
      return os.filler ? os.filler() : TRACYHIP_OK;
    };
    const int src = sweeps();
    HIP_TRY(hipStreamWaitEvent(st, fk.joined[0], 0));  // (on every way out: nothing of the call runs beside the call's stream afterwards)
    if (src) return src;
  } else {
    bool pre_done = false;
    for (const SweepClass& c : h.classes) {
      DpArgs af = a;
      af.pairs = sc.full + 2 * (size_t)c.lo;
      DpArgs apl = ap;
      launch_diag_periods(ctx, &p, c.K, 2 * (c.hi - c.lo), pre_done ? 0u : npre_all, true, af, apl);
      TRY(timing_begin(ctx, TRACYHIP_TIMER_SCORE, 0, 0));
      HIP_TRY(launch_gotoh_ckpt_front(c.K, af, 2 * (c.hi - c.lo), apl, pre_done ? 0u : npre_all, st, ctx->knobs.prefix_tall_min));
      TRY(timing_end(ctx));
      pre_done = true;
    }
    TRY(front_tiers());
  }
  hipLaunchKernelGGL(s_orient_decide_kernel, g256, b256, 0, st, sp, sc.geom, sc.votes, sc.ub, sc.sc2, sc.fo1, sc.fs1, sc.fe1, sc.fo2, sc.fs2, sc.fe2, sc.tr, sc.re,
                     sc.dead, sc.cnt, os.desc_trim);
  hipLaunchKernelGGL(row_m_end_kernel, dim3(nt), dim3(64), 0, st, static_cast<const RowEndDesc*>(sc.re), static_cast<const int32_t*>(os.d_lastrow), p.go + p.ge, sc.ce);
  HIP_TRY(hipGetLastError());
  return TRACYHIP_OK;
}

// the geometry every trace of a batch has, the sweep order, the workspace offsets; kStreamNo when the batch is not of the stream-ordered shape
// What a caller adds to plan_common's passes over the traces (`tracy decompose`: its own sums and records).  Every pass is a fork and a join
// of the host threads -- 0.3-0.5 ms each on a 100 000-trace batch, whatever it computes, while the device waits -- so the caller's loops
// run INSIDE the two passes there are, slice by slice, instead of in passes of their own.
struct PlanHooks {
  std::function<void(uint32_t lo, uint32_t hi, uint32_t tid)> lengths_slice;  // after the lengths of traces [lo, hi) are known (h.mf / mt / tl / rn)
  std::function<int()> between;                                                 // on the calling thread, before the records are written; an error ends the plan
  std::function<void(uint32_t lo, uint32_t hi, uint32_t tid)> records_slice;  // after the records of traces [lo, hi) are written (trace order)
};
int plan_common(tracyhip_ctx* ctx, const tracyhip_params& p, const tracyhip_seqset& sp, const tracyhip_seqset& sr, const uint32_t* ref_index, uint32_t nt,
                const TrimSrc& trims, StreamHost& h, SGeom* geom, const PlanHooks* hooks = nullptr) {
  h = StreamHost{std::move(h.mf), std::move(h.mt), std::move(h.tl), std::move(h.rn), std::move(h.ridx)};  // (the vectors keep their pages between calls)
  h.nt = nt;
  h.mf.resize(nt); h.mt.resize(nt); h.tl.resize(nt); h.rn.resize(nt); h.ridx.resize(nt);
  static thread_local std::vector<int> kof_tls;  // (kept between calls; the worker threads reach the CALLER's vector through the reference)
  std::vector<int>& kof = kof_tls;
  kof.resize(nt);
  bool odd_shape = false, similar = false;
  uint64_t lr_base[kHostThreads], tab_base[kHostThreads];  // workspace offsets of the slices' first traces (trace order)
  {
    // ONE pass over the job's length arrays (the device waits while the host plans: round 6 measured 2.3 ms per 100 000-trace call in
    // seven passes): lengths, trims, extremes, the strip height of every trace's sweep, whether the batch is of the one-pass shape and
    // whether it is "of a size" (one strip height, cell counts within a quarter of each other: the sweeps then run in the traces' order)
    TRACYHIP_HOST_SCOPE(hs1, "plan_common.lengths");
    struct Part { uint64_t max_mn, lr, tab; uint32_t maxmt, maxmf, bad; bool odd; SizeSpan span; };
    Part part[kHostThreads];
    for (auto& x : part) x = Part{0, 0, 0, 0, 0, ~0u, false, SizeSpan()};
    parallel_for(nt, [&](uint32_t lo, uint32_t hi, uint32_t tid) {
      Part x{0, 0, 0, 0, 0, ~0u, false, SizeSpan()};
      for (uint32_t t = lo; t < hi; ++t) {
        h.ridx[t] = ref_index ? ref_index[t] : t;
        if (h.ridx[t] >= sr.count) { x.bad = std::min(x.bad, t); h.ridx[t] = 0; if (sr.count == 0) continue; }
        h.mf[t] = sp.length[t];
        h.rn[t] = sr.length[h.ridx[t]];
        uint32_t l = trims.left(t), r = trims.right(t);
        if ((uint64_t)l + r >= h.mf[t]) { l = 0; r = 0; }  // createProfile, profile.h:24-27 (per trace: its own pair)
        h.tl[t] = l;
        h.mt[t] = h.mf[t] - (l + r);
        x.max_mn = std::max<uint64_t>(x.max_mn, (uint64_t)h.mf[t] + h.rn[t]);
        x.maxmt = std::max(x.maxmt, h.mt[t]);
        x.maxmf = std::max(x.maxmf, h.mf[t]);
        const int K = choose_k(h.mt[t], MODE_QP);
        kof[t] = K;
        x.odd = x.odd || h.mt[t] == 0 || h.rn[t] == 0 || num_passes(h.mt[t], K) != 1;
        x.span.add(SweepKey{K, 0u, (uint64_t)h.mt[t] * h.rn[t]});
        x.lr += 4ull * ((uint64_t)h.rn[t] + 1);  // (workspace of the slice's traces: row-m words of both strands, substitution tables)
        x.tab += (uint64_t)kB16Codes * b16_table_stride(h.mf[t]);
      }
      part[tid] = x;
      if (hooks && hooks->lengths_slice && x.bad == ~0u) hooks->lengths_slice(lo, hi, tid);
    });
    for (uint32_t i = 0; i < kHostThreads; ++i) { lr_base[i] = h.lr_tot; tab_base[i] = h.tab_tot; h.lr_tot += part[i].lr; h.tab_tot += part[i].tab; }
    uint32_t bad = ~0u;
    SizeSpan span;
    for (const Part& x : part) {
      h.max_mn = std::max(h.max_mn, x.max_mn); h.maxmt = std::max(h.maxmt, x.maxmt); h.maxmf = std::max(h.maxmf, x.maxmf); bad = std::min(bad, x.bad);
      odd_shape = odd_shape || x.odd;
      span.add(x.span);
    }
    similar = span.of_a_size();
    if (bad != ~0u) return set_error(TRACYHIP_ERR_ARG, "ref_index[%u] out of range", bad);
  }
  TRY(check_params(&p, h.max_mn));
  if (!(p.ge < 0 && p.go <= 0 && sub_limit(&p) <= kWideScore)) return kStreamNo;
  if (!narrow_ok(&p, h.maxmt, 16)) return kStreamNo;
  if (odd_shape) return kStreamNo;
  static thread_local std::vector<uint32_t> order_tls;
  std::vector<uint32_t>& order = order_tls;
  { TRACYHIP_HOST_SCOPE(hs3, "plan_common.sweep_order"); sweep_order(h, order, kof, similar); }
  if (hooks && hooks->between) TRY(hooks->between());
  TRACYHIP_HOST_SCOPE(hs4, "plan_common.records_and_offsets");
  uint32_t rest_of[kHostThreads] = {};
  const bool in_trace_order = order.empty();
  parallel_for(nt, [&](uint32_t lo_, uint32_t hi_, uint32_t tid) {
   uint32_t max_rest = 0;
   uint64_t lr = lr_base[tid], tab = tab_base[tid];
   for (uint32_t i = lo_; i < hi_; ++i) {
    const uint32_t t = order.empty() ? i : order[i];
    // class c holds its A slots then its B slots: [2 lo, 2 lo + n_c) and [2 lo + n_c, 2 hi)
    const SweepClass* cls = nullptr;
    for (const SweepClass& c : h.classes) if (i >= c.lo && i < c.hi) { cls = &c; break; }
    SGeom G{};
    G.prof_off = sp.offset[t];
    G.ref_off = sr.offset[h.ridx[t]];
    G.mf = h.mf[t]; G.mt = h.mt[t]; G.tl = h.tl[t]; G.rn = h.rn[t];
    G.rl = trims.left(t); G.rr = trims.right(t);
    G.full_a = 2 * cls->lo + (i - cls->lo);
    G.full_b = 2 * cls->lo + (cls->hi - cls->lo) + (i - cls->lo);
    const bool front_ok = s_front_ok(&p, G.mt, G.rn);
    G.flags = front_ok ? SG_FRONT_OK : 0u;
    if (front_ok) max_rest = std::max(max_rest, G.mt - kFrontRows);
    if (in_trace_order) {  // (the sweeps run in the traces' own order: a slice's workspace offsets are its running sums)
      for (int o = 0; o < 2; ++o) { G.lr_off[o] = lr; lr += 2ull * ((uint64_t)G.rn + 1); }
      G.tab_stride = b16_table_stride(G.mf);
      G.tab_off = tab;
      tab += (uint64_t)kB16Codes * G.tab_stride;
    }
    geom[t] = G;
   }
   rest_of[tid] = max_rest;
   if (in_trace_order && hooks && hooks->records_slice) hooks->records_slice(lo_, hi_, tid);
  });
  for (uint32_t x : rest_of) h.max_rest = std::max(h.max_rest, x);
  if (!in_trace_order) {  // workspace offsets in trace order, every slice from its base (the records above were written in sweep order)
    parallel_for(nt, [&](uint32_t lo, uint32_t hi, uint32_t tid) {
      uint64_t lr = lr_base[tid], tab = tab_base[tid];
      for (uint32_t t = lo; t < hi; ++t) {
        SGeom& G = geom[t];
        for (int o = 0; o < 2; ++o) { G.lr_off[o] = lr; lr += 2ull * ((uint64_t)G.rn + 1); }
        G.tab_stride = b16_table_stride(G.mf);
        G.tab_off = tab;
        tab += (uint64_t)kB16Codes * G.tab_stride;
      }
      if (hooks && hooks->records_slice) hooks->records_slice(lo, hi, tid);
    });
  }
  if (h.max_rest == 0) return kStreamNo;  // no trace takes the pruned sweep
  if (!front_tiers_fit(h.max_rest)) return kStreamNo;  // (rests beyond ~14 k rows: the band launches below the kept row find no LDS)
  return TRACYHIP_OK;
}

// what the launches of the call reported (DpArgs::err): un-normalised profiles send the call to the host-planned pipeline, which
// repeats its stages on the wider kernels or reports the range error
int stream_range_verdict(const tracyhip_params& p, const int32_t* herr, const StreamHost& h) {
  if (herr[0] & 1) return kStreamNo;
  if (herr[1] > sub_limit(&p) || herr[2] || herr[3]) return kStreamNo;
  return TRACYHIP_OK;
}

void stats_from_counters(tracyhip_ctx* ctx, const unsigned long long* c, const unsigned long long* bstat, int nstages, const int* stage_timer,
                         uint32_t large_stages) {
  tracyhip_call_stats& s = ctx->stats;
  s.pruned += (uint32_t)c[SC_PRUNED]; s.pruned_uncertified += (uint32_t)c[SC_PRUNED_UNCERT];
  s.prelim_banded += (uint32_t)c[SC_PRELIM_BANDED]; s.prelim_repeated += (uint32_t)c[SC_PRELIM_REPEATED];
  s.final_banded += (uint32_t)c[SC_FINAL_BANDED]; s.final_repeated += (uint32_t)c[SC_FINAL_REPEATED];
  for (int k = 0; k < 2; ++k) { s.allele_pruned[k] += (uint32_t)c[SC_ALLELE_PRUNED0 + k]; s.allele_uncertified[k] += (uint32_t)c[SC_ALLELE_UNCERT0 + k]; }
  for (int k = 0; k < 3; ++k) { s.allele_banded[k] += (uint32_t)c[SC_ALLELE_BANDED0 + k]; s.allele_repeated[k] += (uint32_t)c[SC_ALLELE_REPEATED0 + k]; }
  s.allele_shared_prefix += (uint32_t)c[SC_ALLELE_SHARED];
  for (int i = 0; i < nstages; ++i)  // (a stage's kind by its timer: tracebacks, origin sweeps)
    for (int b = 0; b < SB_LIST_N; ++b) s.band_list_pairs[stage_timer[i] == TRACYHIP_TIMER_TRACE ? 0 : 1][b] += (uint32_t)bstat[SB_COUNT * i + SB_LIST + b];
  s.band_large_launches += large_stages;
  if (ctx->timing) {
    ctx->acc[TRACYHIP_TIMER_SCORE].cells += c[SC_SWEEP_CELLS];
    ctx->acc[TRACYHIP_TIMER_SCORE].bytes += c[SC_SWEEP_BYTES];
    ctx->acc[TRACYHIP_TIMER_DECOMP].cells += c[SC_DECOMP_CELLS];
    ctx->acc[TRACYHIP_TIMER_DECOMP].bytes += c[SC_DECOMP_BYTES];
    ctx->acc[TRACYHIP_TIMER_FRONT].cells += c[SC_FRONT_CELLS];
    ctx->acc[TRACYHIP_TIMER_FRONT].bytes += c[SC_FRONT_BYTES];
    for (int i = 0; i < nstages; ++i) {
      ctx->acc[stage_timer[i]].cells += bstat[SB_COUNT * i + SB_CELLS];
      ctx->acc[stage_timer[i]].bytes += bstat[SB_COUNT * i + SB_BYTES];
    }
  }
  if (ctx->knobs.verbose)
    for (int i = 0; i < nstages; ++i) {
      const unsigned long long* hst = bstat + SB_COUNT * i + SB_HIST;
      const unsigned long long* lst = bstat + SB_COUNT * i + SB_LIST;
      fprintf(stderr, "tracyhip: band stage %d: pairs by diagonals <=8 %llu <=16 %llu <=24 %llu <=32 %llu <=48 %llu <=64 %llu <=96 %llu more %llu; "
              "by strip height 12: %llu 8: %llu 4: %llu quads: %llu\n", i, hst[0], hst[1], hst[2], hst[3], hst[4], hst[5], hst[6], hst[7], lst[0], lst[1], lst[2], lst[3]);
    }
}

// ---- the frame of a stream-ordered call: what stream_align and stream_decompose do AROUND their stages, written once ----

// a reason a call marks traces dead with (SD_*) and its name in the call's verbose line
struct DeadReason { uint32_t bit; const char* name; };

// The pinned block the call's one read-back lands in: verdict words, counters, band statistics, dead flags, then `extra_bytes` of the
// call's own (align: the slice lengths; decompose: the verdict of the case-sensitive encoders).  The copies are queued in two parts
// because the calls put their own copy at different places of the sequence.
struct ReadBack {
  int32_t* herr = nullptr;
  unsigned long long *hcnt = nullptr, *hbst = nullptr;
  uint32_t* hdead = nullptr;
  void* extra = nullptr;
  int carve(tracyhip_ctx* ctx, uint32_t nt, size_t extra_bytes) {
    HIP_TRY(ctx->pin[PB_RES].ensure(kErrBytes + sizeof(unsigned long long) * (SC_COUNT + SB_COUNT * 8) + sizeof(uint32_t) * (size_t)nt + extra_bytes));
    herr = static_cast<int32_t*>(ctx->pin[PB_RES].p);
    hcnt = reinterpret_cast<unsigned long long*>(herr + kErrWords + 4);
    hbst = hcnt + SC_COUNT;
    hdead = reinterpret_cast<uint32_t*>(hbst + SB_COUNT * 8);
    extra = hdead + nt;
    return TRACYHIP_OK;
  }
  int queue_verdict(tracyhip_ctx* ctx, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(herr, ctx->dev[DB_ERR].p, kErrBytes, hipMemcpyDeviceToHost, st));
    return TRACYHIP_OK;
  }
  int queue_counters(const StreamCommon& sc, uint32_t nt, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(hcnt, sc.cnt, sizeof(unsigned long long) * SC_COUNT, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hbst, sc.bstat, sizeof(unsigned long long) * SB_COUNT * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hdead, sc.dead, sizeof(uint32_t) * (size_t)nt, hipMemcpyDeviceToHost, st));
    return TRACYHIP_OK;
  }
};

// every per-trace result array of the list Fields (stream_fields.h) ...
// ... carved from the arena (in list order; every take is rounded to 256 bytes, so the block's size does not depend on the order)
template <class Fields, class Out>
void carve_all(Arena& a, uint32_t nt, Out& x) {
  Fields::each(x, x, [&](auto& p, auto&, uint32_t per) { a.take_into(p, (size_t)per * nt); });
}
// ... pointed where another struct's is
template <class Fields, class To, class From>
void point_all(To& to, const From& from) {
  Fields::each(to, from, [](auto& t, auto& f, uint32_t) { t = f; });
}
// ... of the dead traces (compact, from the host-planned pipeline) back to their places
template <class Fields, class Out>
int scatter_all(hipStream_t st, const uint32_t* d_list, uint32_t n, Out& compact, Out& o) {
  int rc = TRACYHIP_OK;
  Fields::each(compact, o, [&](auto* src, auto* dst, uint32_t per) {
    if (rc != TRACYHIP_OK) return;
    if constexpr (std::is_same_v<decltype(src), double*>)  // (allelicFraction: the two doubles of a trace move as one element)
      rc = scatter(st, d_list, n, reinterpret_cast<const Frac2*>(src), reinterpret_cast<Frac2*>(dst));
    else
      rc = scatter(st, d_list, n, src, dst);
  });
  return rc;
}
// ... to the caller's host memory
int copy_to_host(hipStream_t st, void* user, const void* dev, size_t bytes) {
  if (user && bytes) HIP_TRY(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, st));
  return TRACYHIP_OK;
}
template <class Fields, class Result, class Out>
int copy_back_all(hipStream_t st, uint32_t nt, const Result& user, Out& o) {
  int rc = TRACYHIP_OK;
  Fields::each(user, o, [&](auto& u, auto& d, uint32_t per) {
    if (rc == TRACYHIP_OK) rc = copy_to_host(st, u, d, sizeof(*d) * per * (size_t)nt);
  });
  return rc;
}

// What both calls keep of a call, and the sections both queue.  The stages themselves -- and everything the calls do differently on
// purpose -- are the derived structs' (AlignStream, DecStream).
struct StreamCall {
  tracyhip_ctx* ctx;
  const tracyhip_params* prm;
  const int mem;
  const CtxKnobs& kn;
  const uint32_t nt;
  const tracyhip_seqset &sp, &sr;
  hipStream_t st;
  tracyhip_params p;
  const TrimSrc trims;  // what the job requests per trace (plan_common writes them into the records: SGeom::rl / rr)
  const bool exact, host;
  StreamHost& h;
  SGeom* geom = nullptr;
  uint32_t ncap = 0;
  uint64_t words_cap = 0;
  SParams spm{};
  dim3 g256, b256;
  const int16_t* d_qp = nullptr;
  int32_t* d_lastrow = nullptr;
  ReadBack rb;
  std::vector<uint32_t> dl;  // the traces the device could not give their tier
  std::vector<uint64_t> sub_poff;  // ... as a sub-job: profile offsets, lengths, reference indices
  std::vector<uint32_t> sub_plen, sub_ridx, sub_tl, sub_tr;  // (sub_tl / sub_tr: each dead trace's own requested pair)

  template <class Job>
  StreamCall(tracyhip_ctx* c, const Job* j, const tracyhip_params* q, int m, StreamHost& h_)
      : ctx(c), prm(q), mem(m), kn(c->knobs), nt(j->ntraces), sp(j->profiles), sr(j->refs), st(c->stream), p(*q), trims(trims_of(j)),
        exact(j->strand_by_certificate == 0), host(m == TRACYHIP_MEM_HOST), h(h_), g256((j->ntraces + 255) / 256), b256(256) {
    p.hfree = 1;  // AlignConfig<true,false> semiglobal (sage.h:165, indigo.h:164)
    p.vfree = 0;
  }

  // columns the band launches stage per pair (the longest trace and its margins): beside the widest substitution table they must fit the LDS
  int size_ncap() {
    ncap = band_code_cap(h.maxmf + 200u);
    return band_lds_fits(ncap, 12, kBandLdsHard) ? TRACYHIP_OK : kStreamNo;
  }

  // verdict words cleared, the reference windows encoded to profile-row codes (with their block map and the validation verdict)
  int encode_references(const uint8_t* refs, uint64_t er) {
    HIP_TRY(ctx->dev[DB_ERR].ensure(kErrBytes));
    HIP_TRY(hipMemsetAsync(ctx->dev[DB_ERR].p, 0, kErrBytes, st));
    int32_t* d_verr = static_cast<int32_t*>(ctx->dev[DB_ERR].p) + kErrVerdictWord;
    HIP_TRY(ctx->ensure_codes(er ? er : 1, st));
    if (er) {
      hipLaunchKernelGGL(encode_codes_kernel, dim3((unsigned)((er + 4095) / 4096)), dim3(256), 0, st, refs, ctx->codes(), er, ctx->special_blocks(), d_verr);
      HIP_TRY(hipGetLastError());
    }
    return TRACYHIP_OK;
  }

  // the records: one pinned block (SGeom per trace, then the call's own array), two copies; the per-call arrays cleared
  int upload_records(StreamCommon& sc, void* d_own, size_t own_bytes) {
    HIP_TRY(hipMemcpyAsync(sc.geom, geom, sizeof(SGeom) * (size_t)nt, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_own, geom + nt, own_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(sc.dead, 0, sizeof(uint32_t) * (size_t)nt, st));
    HIP_TRY(hipMemsetAsync(sc.cnt, 0, sizeof(unsigned long long) * SC_COUNT, st));
    HIP_TRY(hipMemsetAsync(sc.bstat, 0, sizeof(unsigned long long) * SB_COUNT * 8, st));
    sc.large_stages = 0;
    return TRACYHIP_OK;
  }

  // what the planning kernels know of the call, and the buffers every stage reads
  void fill_params() {
    spm.match = p.match; spm.mismatch = p.mismatch; spm.go = p.go; spm.ge = p.ge; spm.nt = nt; spm.exact = exact ? 1u : 0u; spm.ncap = ncap - 8u;
    spm.use_votes = 1u;
    spm.split_prefix = kn.sweeps_alone ? 1u : 0u;
    d_qp = static_cast<const int16_t*>(ctx->dev[DB_B16TAB_PROFILE].p);
    d_lastrow = static_cast<int32_t*>(ctx->dev[DB_LASTROW].p);
  }

  // The call's one synchronisation, then what its launches reported: lower-case reference windows are the caller's error, values
  // outside the 16-bit kernels' range hand the call to the host-planned pipeline.  give_up(rc) is what the call does before it returns
  // a verdict (decompose: DecStream::give_up; align has nothing to put back).
  template <class GiveUp>
  int await_verdict(GiveUp give_up) {
    HIP_TRY(ctx_sync(ctx));
    timing_collect(ctx);
    if (rb.herr[kErrVerdictWord] & 4) {
      (void)give_up(kStreamNo);
      return set_error(TRACYHIP_ERR_ARG, "reference windows must be upper-case [ACGTN] (loadSingleFasta, fasta.h:54-95)");
    }
    return give_up(stream_range_verdict(p, rb.herr, h));
  }

  // the call's statistics from its counters; the traces the device could not give their tier, and (verbose) why
  template <size_t NS, size_t NR>
  void list_dead(const char* what, const StreamCommon& sc, const int (&stage_timer)[NS], const DeadReason (&reasons)[NR]) {
    stats_from_counters(ctx, rb.hcnt, rb.hbst, (int)NS, stage_timer, sc.large_stages);
    ctx->stats.stream_ordered = 1;
    dl.clear();
    for (uint32_t t = 0; t < nt; ++t)
      if (rb.hdead[t]) dl.push_back(t);
    ctx->stats.fallback_traces += (uint32_t)dl.size();
    if (kn.verbose) {
      std::string why;
      for (const DeadReason& r : reasons) {
        uint32_t n = 0;
        for (uint32_t t : dl) n += (rb.hdead[t] & r.bit) != 0u;
        why += (why.empty() ? "" : ", ") + std::string(r.name) + " " + std::to_string(n);
      }
      fprintf(stderr, "stream-ordered %s: %u traces, %zu to the host-planned tiers (%s)\n", what, nt, dl.size(), why.c_str());
    }
  }

  // the dead traces as a job of their own for the host-planned pipeline: payloads where they lie on the device, offsets by the list
  template <class Job>
  void sub_job(Job& j, const void* d_prof, const void* d_ref) {
    const uint32_t nd = (uint32_t)dl.size();
    sub_poff.resize(nd); sub_plen.resize(nd); sub_ridx.resize(nd); sub_tl.resize(nd); sub_tr.resize(nd);
    for (uint32_t i = 0; i < nd; ++i) {
      const uint32_t t = dl[i];
      sub_poff[i] = sp.offset[t]; sub_plen[i] = sp.length[t]; sub_ridx[i] = h.ridx[t];
      sub_tl[i] = trims.left(t); sub_tr[i] = trims.right(t);
    }
    j.ntraces = nd;
    j.profiles.data = d_prof; j.profiles.offset = sub_poff.data(); j.profiles.length = sub_plen.data(); j.profiles.count = nd;
    j.refs.data = d_ref;
    j.ref_index = sub_ridx.data();
    j.trim_left_each = sub_tl.data(); j.trim_right_each = sub_tr.data();
  }

  // run() is the host-planned pipeline on the sub-job: the call's statistics stay the stream-ordered call's, only its synchronisations count
  template <class Run>
  int host_planned(Run run) {
    const tracyhip_call_stats keep = ctx->stats;
    TRY(run());
    const uint32_t syncs = ctx->stats.host_syncs;
    ctx->stats = keep;
    ctx->stats.host_syncs = syncs;
    return TRACYHIP_OK;
  }
};

}  // namespace

// =====================================================================================================================
// tracyhip_align_traces, stream-ordered (sage.h:191-311)
// =====================================================================================================================
namespace {
struct AlignArena {
  StreamCommon sc;
  uint64_t* ops_off;
  // results where the caller's arrays are host memory (TRACYHIP_MEM_HOST)
  AlignOutDev o;
  uint8_t* ops;
  // compact results of the dead traces (host-planned pipeline), scattered back
  AlignOutDev f;
  uint32_t* dead_list;
  void layout(Arena& a, uint32_t nt, bool exact, bool host_results, uint64_t ops_bound) {
    sc.layout(a, nt, nt, exact, true);
    ops_off = a.take<uint64_t>(nt);
    o = AlignOutDev{};
    ops = nullptr;
    if (host_results) { carve_all<AlignFields>(a, nt, o); ops = a.take<uint8_t>(ops_bound); }
    carve_all<AlignFields>(a, nt, f);
    dead_list = a.take<uint32_t>(nt);
  }
};

// One stream-ordered tracyhip_align_traces call: one method per section (queued in this order), as DecStream below
struct AlignStream : StreamCall {
  const tracyhip_align_job* job;
  const tracyhip_align_result* out;
  uint64_t ops_bound = 1;
  AlignArena A;
  const void *d_prof = nullptr, *d_ref = nullptr;
  AlignOutDev o{};
  uint8_t* d_ops = nullptr;
  uint32_t* hlen = nullptr;  // the slice lengths (host-memory results: they size the copy of the ops)

  AlignStream(tracyhip_ctx* c, const tracyhip_align_job* j, const tracyhip_params* q, int m, const tracyhip_align_result* o_, StreamHost& h_)
      : StreamCall(c, j, q, m, h_), job(j), out(o_) {}

  // geometry and the ops offsets are laid out in the pinned block they travel from: one copy, no staging
  int pin_records() {
    HIP_TRY(ctx->pin[PB_DESC].ensure(sizeof(SGeom) * (size_t)nt + sizeof(uint64_t) * (size_t)nt));
    geom = static_cast<SGeom*>(ctx->pin[PB_DESC].p);
    return TRACYHIP_OK;
  }
  int plan_geometry() { return plan_common(ctx, p, sp, sr, job->ref_index, nt, trims, h, geom); }

  // what the host knows before anything runs, beside the geometry: where the ops go, the workspace
  int plan() {
    for (uint32_t t = 0; t < nt; ++t) {
      geom[t].ops_off = out->ops_offset[t];
      ops_bound = std::max<uint64_t>(ops_bound, out->ops_offset[t] + h.mf[t] + h.rn[t]);
    }
    TRY(size_ncap());

    // ---- workspace ----
    uint64_t rows_total = 0;
    for (uint32_t t = 0; t < nt; ++t) rows_total += h.mf[t];
    Arena sizing;
    A.layout(sizing, nt, exact, host, ops_bound);
    TRY(with_fresh_budget(ctx, [&](bool* from_cache) -> int {
      uint64_t budget = 0;
      TRY(workspace_budget(ctx, ctx->dev[DB_LASTROW].cap + ctx->dev[DB_BITS].cap + ctx->dev[DB_STREAM].cap + ctx->dev[DB_B16TAB_PROFILE].cap, &budget, from_cache));
      const uint64_t fixed = h.lr_tot * 4 + 64 + h.tab_tot * 2 + 64 + sizing.off;
      if (fixed > budget) return kStreamNo;
      words_cap = band_words_cap(rows_total, nt, budget - fixed);
      HIP_TRY(ctx->dev[DB_LASTROW].ensure(h.lr_tot * 4 + 64));
      HIP_TRY(ctx->dev[DB_B16TAB_PROFILE].ensure(h.tab_tot * sizeof(int16_t) + 64));
      HIP_TRY(ctx->dev[DB_BITS].ensure(words_cap + 64));
      HIP_TRY(ctx->dev[DB_STREAM].ensure(sizing.off + 256));
      return TRACYHIP_OK;
    }));
    Arena arena;
    arena.base = static_cast<char*>(ctx->dev[DB_STREAM].p);
    A.layout(arena, nt, exact, host, ops_bound);
    return TRACYHIP_OK;
  }

  // payloads and result arrays: the caller's (device memory) or staged; references encoded once; records uploaded
  int bind() {
    const uint64_t ep = seqset_extent(sp), er = seqset_extent(sr);
    TRY(stage_in(ctx, ctx->dev[DB_IN1], sp.data, ep * 4, mem, &d_prof));
    TRY(stage_in(ctx, ctx->dev[DB_IN2], sr.data, er, mem, &d_ref));
    TRY(encode_references(static_cast<const uint8_t*>(d_ref), er));
    std::memcpy(geom + nt, out->ops_offset, sizeof(uint64_t) * (size_t)nt);
    TRY(upload_records(A.sc, A.ops_off, sizeof(uint64_t) * (size_t)nt));
    fill_params();
    o = A.o;
    d_ops = A.ops;
    if (!host) { point_all<AlignFields>(o, *out); d_ops = out->ops; }
    return TRACYHIP_OK;
  }

  // stages 2 - 4 on the context's stream for the traces marked ST_EARLY (early = 1) or for all the others (0)
  int queue_alignments(int early) {
    StreamCommon& sc = A.sc;
    hipStream_t s = ctx->stream;
    // ---- 2. preliminary alignment (sage.h:258) by its two ends, 3. trimReferenceSlice (sage.h:259) ----
    hipLaunchKernelGGL(s_prelim_plan_kernel, g256, b256, 0, s, spm, 0, early, sc.geom, sc.tr, sc.ce, sc.top_trim, sc.dead, sc.cand, sc.kc, queued_prio(ctx, 2));
    HIP_TRY(hipGetLastError());
    BandStageArgs b1;
    b1.kind = 1; b1.qp = d_qp; b1.codes = ctx->codes(); b1.ends = sc.ends; b1.code_cap = ncap; b1.hfree = 1;
    TRY(band_stage(ctx, p, sc, nt, nt, 0, b1, ~0ull));
    // ---- 4. final alignment gotoh(full profile, trimmed slice) (sage.h:311) on its certified band ----
    hipLaunchKernelGGL(s_align_final_plan_kernel, g256, b256, 0, s, spm, early, sc.geom, sc.tr, sc.ends, sc.dead, sc.cand, sc.kc, sc.cnt, queued_prio(ctx, 2));
    HIP_TRY(hipGetLastError());
    BandStageArgs b2;
    b2.kind = 0; b2.qp = d_qp; b2.codes = ctx->codes(); b2.scores = o.score_final; b2.ops = d_ops; b2.ops_off = A.ops_off; b2.ops_len = o.ops_len; b2.code_cap = ncap;
    b2.hfree = 1;
    return band_stage(ctx, p, sc, nt, nt, 1, b2, words_cap);
  }

  // The order of the call.  Side stream: the voted strands' prefixes and tiers, the early decision, stages 2 - 4 of the early traces.
  // Call's stream: the other strands' full sweeps; then, behind both, the decision with both exact scores (which confirms or kills an
  // early trace), stages 2 - 4 once more over the traces that were not early (the same kernels and the same lists, workspace and
  // counters, which the first pass has finished with: the two passes' counters add up), and the certificates of all of them.
  int queue_stages() {
    StreamCommon& sc = A.sc;
    // ---- 1. orientation (sage.h:239-247) ----
    OrientStage os{d_prof, d_qp, d_lastrow, exact, nullptr};
    if (!kn.no_early_tail && exact) os.early_tail = [this]() { return queue_alignments(1); };
    TRY(queue_orientation(ctx, p, spm, h, sc, os));
    TRY(queue_alignments(0));
    hipLaunchKernelGGL(s_align_finish_kernel, g256, b256, 0, st, spm, sc.tr, sc.top_full, sc.dead, o, sc.cnt);
    HIP_TRY(hipGetLastError());
    return TRACYHIP_OK;
  }

  // the one read-back: verdict words, counters, dead flags (+ the slice lengths when the ops go to host memory)
  int read_back() {
    TRY(rb.carve(ctx, nt, host ? sizeof(uint32_t) * (size_t)nt : 0));
    hlen = static_cast<uint32_t*>(rb.extra);
    TRY(rb.queue_verdict(ctx, st));
    TRY(rb.queue_counters(A.sc, nt, st));
    if (host) HIP_TRY(hipMemcpyAsync(hlen, o.slice_len, sizeof(uint32_t) * (size_t)nt, hipMemcpyDeviceToHost, st));
    TRY(await_verdict([](int rc) { return rc; }));
    static const int stage_timer[2] = {TRACYHIP_TIMER_ORIGIN, TRACYHIP_TIMER_TRACE};
    static const DeadReason reasons[] = {{SD_FRONT, "front"}, {SD_STRAND, "strand"}, {SD_LOSER_WON, "loser won"}, {SD_JUNK, "junk"}, {SD_PRELIM_BAND, "prelim band"},
                                         {SD_FINAL_BAND, "final band"}, {SD_FINAL_CHECK, "final check"}, {SD_MEM, "mem"}, {SD_SHAPE, "shape"}};
    list_dead("align", A.sc, stage_timer, reasons);
    return TRACYHIP_OK;
  }

  // traces the device could not give their tier: the host-planned pipeline, every tier of it, on the list
  int redo_dead_traces() {
    if (dl.empty()) return TRACYHIP_OK;
    const uint32_t nd = (uint32_t)dl.size();
    std::vector<uint64_t> ooff(nd);
    for (uint32_t i = 0; i < nd; ++i) ooff[i] = out->ops_offset[dl[i]];
    tracyhip_align_job j = *job;
    sub_job(j, d_prof, d_ref);
    tracyhip_align_result r{};
    point_all<AlignFields>(r, A.f);
    r.ops = d_ops; r.ops_offset = ooff.data();
    TRY(host_planned([&]() { return align_traces_legacy(ctx, &j, prm, TRACYHIP_MEM_DEVICE, &r); }));
    HIP_TRY(hipMemcpyAsync(A.dead_list, dl.data(), sizeof(uint32_t) * nd, hipMemcpyHostToDevice, st));
    TRY(scatter_all<AlignFields>(st, A.dead_list, nd, A.f, o));
    if (host) {  // (the host-planned pipeline may have re-allocated the pinned blocks: a fresh one for the lengths)
      HIP_TRY(ensure_into(ctx->pin[PB_RES], nt, hlen));
      HIP_TRY(hipMemcpyAsync(hlen, o.slice_len, sizeof(uint32_t) * (size_t)nt, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx_sync(ctx));  // (dl is pageable)
    return TRACYHIP_OK;
  }

  // results to the caller's host arrays
  int copy_back() {
    if (!host) return TRACYHIP_OK;
    uint64_t ops_total = 0;
    for (uint32_t t = 0; t < nt; ++t) ops_total = std::max<uint64_t>(ops_total, out->ops_offset[t] + h.mf[t] + hlen[t]);
    TRY(copy_back_all<AlignFields>(st, nt, *out, o));
    TRY(copy_to_host(st, out->ops, d_ops, ops_total));
    HIP_TRY(ctx_sync(ctx));
    return TRACYHIP_OK;
  }
};
}  // namespace

int tracyhip::stream_align(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm, int mem, const tracyhip_align_result* out) {
  if (!stream_options_ok(ctx->knobs) || job->oriented) return kStreamNo;
  static thread_local StreamHost h;
  AlignStream s(ctx, job, prm, mem, out, h);
  TRY(s.pin_records());
  { TRACYHIP_HOST_SCOPE(hsa, "stream_align.plan_common"); TRY(s.plan_geometry()); }
  TRACYHIP_HOST_SCOPE(hsb, "stream_align.rest_of_call");
  TRY(s.plan());
  TRY(s.bind());
  TRY(s.queue_stages());  // 1. .. 4. (sage.h:239-311)
  TRY(s.read_back());     // the call's one synchronisation
  TRY(s.redo_dead_traces());
  return s.copy_back();
}

// =====================================================================================================================
// tracyhip_decompose_traces, stream-ordered (indigo.h:190-388)
// =====================================================================================================================
namespace {

struct SParamsD {        // what the allele stages need beside SParams
  uint64_t bext;         // extent of the basecall arrays: allele k of trace t is the string at k bext + bc_off + soff of the two-allele buffer
  int32_t best;          // max(match, mismatch, 0): the most a row of a string scores
};

// off1 / aops_off / ops2_off: where the band launches of the four traceback stages put their strings -- plain offset arrays
// (Band16Args::ops_off) filled here from the records instead of travelling beside them (3.2 MB per 100 000 traces and a host loop);
// base1: alleles 1 and 2 reach their buffers through offsets relative to allele 0's, modulo 2^64 (band16_body adds an offset to ONE pointer)
__global__ void s_expand_d_kernel(const SGeom* __restrict__ geom, const SGeomD* __restrict__ geomd, uint32_t nt, uint64_t bext, BpDesc* __restrict__ bp,
                                  RowsDesc* __restrict__ rows, DecompDesc* __restrict__ dd, BcDesc* __restrict__ bc, B16TableDesc* __restrict__ atd,
                                  uint64_t* __restrict__ off1, uint64_t* __restrict__ aops_off, uint64_t* __restrict__ ops2_off, uint64_t base1) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  const SGeom G = geom[t];
  const SGeomD D = geomd[t];
  off1[t] = G.ops_off;
  aops_off[t] = D.opsk_off[0];
  aops_off[nt + t] = base1 + D.opsk_off[1];
  ops2_off[t] = D.opsk_off[2];
  bp[t] = BpDesc{G.prof_off + G.tl, G.mf, G.mt};
  rows[t] = RowsDesc{G.ops_off, 0u, 0u};
  dd[t] = DecompDesc{G.ops_off, D.bc_off, D.dcp_off, 0u, G.mf, G.rn, 0u, G.rl, G.rr};
  bc[t] = BcDesc{D.sig_off, D.bc_off, D.nsamples, G.mf, G.rl, G.rr};
  for (uint32_t k = 0; k < 2; ++k) atd[k * nt + t] = B16TableDesc{k * bext + D.bc_off + D.soff, D.atab_off[k], 0u, D.sl, D.atab_stride, 0u};
}

// the band traceback of the trimmed trace (indigo.h:302) must reproduce the sweep's score; its string completes the alignment rows
__global__ void s_prelim_check_kernel(SParams p, const STrace* __restrict__ tr, const int32_t* __restrict__ sb, uint32_t* __restrict__ len1, const uint8_t* __restrict__ kc,
                                      int32_t* __restrict__ strim, uint32_t* __restrict__ dead, unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  if (!dead[t] && kc[t]) {
    s_count(lc, SC_PRELIM_BANDED);
    if (!s_exact_certified(sb[t], tr[t].sstar, len1[t])) { dead[t] |= SD_PRELIM_CHECK; s_count(lc, SC_PRELIM_REPEATED); }
  }
  if (dead[t]) { len1[t] = 0u; return; }  // (nothing downstream walks its rows)
  strim[t] = tr[t].sstar;
  });
}

// indigo.h:303-309 (the score gate) and 314-317 (findHomozygousBreakpoint's verdict) as tracyhip_decompose_result::status; what the
// decomposeAlleles launch worked on, for the kernel timers
__global__ void s_status_kernel(SParams p, const SGeom* __restrict__ geom, const int32_t* __restrict__ strim, const int32_t* __restrict__ hst,
                                const uint32_t* __restrict__ len1, const uint32_t* __restrict__ dead, int32_t* __restrict__ status,
                                unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt || dead[t]) return;
  const double seqsize = (double)geom[t].mt;
  const double thr = seqsize * 0.35 * p.match + seqsize * (1 - 0.35) * p.mismatch;
  int32_t st = 0;
  if ((double)strim[t] <= thr) st = -1;
  else if (hst[t] != 1) st = hst[t] == 0 ? -2 : -3;
  status[t] = st;
  s_count(lc, SC_DECOMP_CELLS, len1[t]);
  s_count(lc, SC_DECOMP_BYTES, 2ull * len1[t] + 4ull * geom[t].mf);
  });
}

// gotoh(allele, rs.refslice) (indigo.h:359) by the pruned sweep: prefix rows with row R kept + the band below them (pipeline.hip 6.b)
__global__ void s_allele_plan0_kernel(SParams p, SParamsD pd, const SGeom* __restrict__ geom, const SGeomD* __restrict__ geomd, const STrace* __restrict__ tr,
                                      uint32_t* __restrict__ dead, PairDesc* __restrict__ pre, FrontDesc* __restrict__ fd, const uint8_t* __restrict__ seqs,
                                      int share, unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 2u * p.nt) return;
  const uint32_t k = q / p.nt, t = q % p.nt;
  pre[q] = s_skip_pair(q);
  FrontDesc f{};
  f.flags = PAIR_SKIP;
  f.out = q;
  fd[q] = f;
  if (dead[t]) return;
  const SGeom G = geom[t];
  const SGeomD D = geomd[t];
  if (!(D.flags[k] & SG_FRONT_OK) || D.sl == 0u || G.rn == 0u) { atomicOr(dead + t, SD_ALLELE_FRONT); return; }
  const uint32_t R = kFrontRows, rcf = tr[t].rc ? PAIR_A2_REVCOMP : 0u;
  PairDesc d{};
  d.a1_off = k * pd.bext + D.bc_off + D.soff;
  d.m = D.sl; d.a1_stride = D.sl;
  d.a2_off = G.ref_off;
  d.n = G.rn; d.a2_stride = G.rn;
  d.flags = rcf | PAIR_KEEP_ROW;
  d.out = q;
  d.lastrow_off = D.alr_off[k];
  // The two alleles of a trace differ from the breakpoint on and at heterozygous positions before it: where their first R
  // characters are the same string, rows 1..R against the same window are the same rows, and allele 2 reads the row allele 1 keeps
  // (two thirds of the traces of the decompose bench).  Byte equality of the inputs, nothing else.
  uint32_t kept = k;
  if (share && k == 1u && (D.flags[0] & SG_FRONT_OK)) {
    const uint8_t *x = seqs + D.bc_off + D.soff, *y = x + pd.bext;
    uint32_t i = 0;
    while (i < R && x[i] == y[i]) ++i;
    if (i == R) kept = 0u;
  }
  if (kept != k) {
    d = s_skip_pair(q);
    s_count(lc, SC_ALLELE_SHARED);
  }
  pre[q] = d;
  f.row_off = D.alr_off[kept];
  f.a2_off = G.ref_off;
  f.tab_off = D.atab_off[k] + R;
  f.tab_stride = D.atab_stride;
  f.m_rest = D.sl - R;
  f.n = G.rn;
  f.flags = rcf;
  f.R = R;
  f.rest = (int32_t)((int64_t)pd.best * (int64_t)(D.sl - R));  // a row of a string scores `match` at most
  fd[q] = f;
  s_count(lc, SC_ALLELE_PRUNED0 + (int)k);
  s_count_front(lc, f);
  if (kept == k) {
    const Credit c = prefix_credit(D.sl, G.rn, R);
    s_count(lc, SC_SWEEP_CELLS, c.cells);
    s_count(lc, SC_SWEEP_BYTES, c.bytes);
  }
  });
}

// the verdict of the pruned sweep; S*, c_e bound the alignment: the origin-tracking sweep over its sub-window, on its band (pipeline.hip 6.c, 6.d;
// s_sub_window)
__global__ void s_allele_plan1_kernel(SParams p, SParamsD pd, const SGeom* __restrict__ geom, const SGeomD* __restrict__ geomd, const STrace* __restrict__ tr,
                                      const FrontOut* __restrict__ fo1, const int32_t* __restrict__ fs1, const uint32_t* __restrict__ fe1,
                                      const FrontOut* __restrict__ fo2, const int32_t* __restrict__ fs2, const uint32_t* __restrict__ fe2,
                                      SAllele* __restrict__ al, uint32_t* __restrict__ dead, PairDesc* __restrict__ cand, uint8_t* __restrict__ kc,
                                      unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 2u * p.nt) return;
  const uint32_t k = q / p.nt, t = q % p.nt;
  kc[q] = 0;
  if (dead[t]) return;
  const SGeom G = geom[t];
  const SGeomD D = geomd[t];
  int32_t sstar = 0;
  uint32_t ce = 0;
  if (fo1[q].ok) { sstar = fs1[q]; ce = fe1[2 * q + 1] ? fe1[2 * q + 1] + fo1[q].shift : 0u; }
  else if (fo2[q].ok) { sstar = fs2[q]; ce = fe2[2 * q + 1] ? fe2[2 * q + 1] + fo2[q].shift : 0u; }
  if (ce == 0u) { atomicOr(dead + t, SD_ALLELE_FRONT); s_count(lc, SC_ALLELE_UNCERT0 + (int)k); return; }
  const uint32_t m = D.sl;
  const SubWindow sw = s_sub_window(m, ce, (int64_t)pd.best * m, sstar, p.ge);
  SAllele A{};
  A.sstar = sstar; A.ce = ce; A.gap = sw.g; A.shift = sw.a;
  al[q] = A;
  int K = sw.K;
  if (K && !b16_origin_ok(p.match, p.mismatch, p.go, p.ge, m, sw.n)) K = 0;
  if (K && !s_fits_lds(sw.n, K)) K = 0;
  if (!K) { atomicOr(dead + t, SD_ALLELE_ORIGIN); return; }
  if (sw.n > p.ncap) { atomicOr(dead + t, SD_SHAPE); return; }
  const bool rc = tr[t].rc != 0;
  PairDesc d{};
  d.a1_off = D.atab_off[k]; d.a1_stride = D.atab_stride;
  d.m = m;
  d.n = sw.n; d.a2_stride = sw.n;
  d.a2_off = G.ref_off + (rc ? (uint64_t)(G.rn - ce) : (uint64_t)sw.a);  // reverse view: column c is byte n - c
  d.flags = rc ? PAIR_A2_REVCOMP : 0u;
  d.out = q;
  d.ckpt_off = band_pack(sw.dlo, sw.dhi);
  cand[q] = d;
  kc[q] = (uint8_t)K;
  });
}

// trimReferenceSlice (indigo.h:360) from the two ends; gotoh(allele, trimmed slice) (indigo.h:365) on the band around its known end (pipeline.hip 6.f;
// s_slice_band, narrowed to the walked path unless option no_origin_band)
__global__ void s_allele_plan2_kernel(SParams p, const SGeom* __restrict__ geom, const SGeomD* __restrict__ geomd, const STrace* __restrict__ tr,
                                      const uint32_t* __restrict__ ends, SAllele* __restrict__ al, uint32_t* __restrict__ dead, PairDesc* __restrict__ cand,
                                      uint8_t* __restrict__ kc, int narrow_by_origin, unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 2u * p.nt) return;
  const uint32_t k = q / p.nt, t = q % p.nt;
  kc[q] = 0;
  if (dead[t]) return;
  const SGeom G = geom[t];
  const SGeomD D = geomd[t];
  SAllele A = al[q];
  const STrace S = tr[t];
  const uint32_t lead = ends[2 * q] + A.shift, cend = ends[2 * q + 1] + A.shift;
  A.trim = s_trim_finish(lead, cend >= lead ? cend - lead : 0u, G.rn, G.rl, G.rr, S.fwd != 0);
  al[q] = A;
  const uint32_t m = D.sl, n = A.trim.len;
  const int64_t ce = (int64_t)cend - (int64_t)A.trim.ri;  // last column of the alignment, in the slice
  const SBand b = s_slice_band(m, n, ce, A.gap, narrow_by_origin != 0, lead, A.trim.ri);
  int K = b.K;
  if (K && !s_fits_lds(n, K)) K = 0;
  if (!K) { atomicOr(dead + t, SD_ALLELE_BAND); return; }
  if (n > p.ncap) { atomicOr(dead + t, SD_SHAPE); return; }
  PairDesc d{};
  d.a1_off = D.atab_off[k]; d.a1_stride = D.atab_stride;
  d.m = m;
  d.n = n; d.a2_stride = n;
  d.a2_off = G.ref_off + (S.rc ? G.rn - A.trim.ri - A.trim.len : A.trim.ri);
  d.flags = S.rc ? PAIR_A2_REVCOMP : 0u;
  d.out = q;
  d.ckpt_off = band_pack(b.dlo, b.dhi);
  cand[q] = d;
  kc[q] = (uint8_t)K;
  s_count(lc, SC_ALLELE_BANDED0 + (int)k);
  });
}

__global__ void s_allele_check_kernel(SParams p, const SAllele* __restrict__ al, const int32_t* __restrict__ score, const uint32_t* __restrict__ len,
                                      uint32_t* __restrict__ dead, unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 2u * p.nt) return;
  const uint32_t k = q / p.nt, t = q % p.nt;
  if (dead[t]) return;
  if (!s_exact_certified(score[q], al[q].sstar, len[q])) { atomicOr(dead + t, SD_ALLELE_CHECK); s_count(lc, SC_ALLELE_REPEATED0 + (int)k); }
  });
}

// allele 1 vs allele 2, global (indigo.h:379-387): the band guessed from what the two alleles lost against the reference, the bound
// its score has to beat (pipeline.hip 6.i; s_a12_band)
__global__ void s_a12_plan_kernel(SParams p, SParamsD pd, const SGeomD* __restrict__ geomd, const int32_t* __restrict__ ascore, uint32_t* __restrict__ dead,
                                  PairDesc* __restrict__ cand, uint8_t* __restrict__ kc, long long* __restrict__ bound, unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt) return;
  kc[t] = 0;
  if (dead[t]) return;
  const SGeomD D = geomd[t];
  const uint32_t m = D.sl;
  const SA12Band b = s_a12_band(m, pd.best, p.go, p.ge, ascore[t], ascore[p.nt + t]);
  if (m) bound[t] = b.bound;
  int K = b.K;
  if (K && !s_fits_lds(m, K)) K = 0;
  if (!K) { dead[t] |= SD_A12_BAND; return; }
  PairDesc d{};
  d.a1_off = D.atab_off[0]; d.a1_stride = D.atab_stride;
  d.m = m; d.n = m; d.a2_stride = m;
  d.a2_off = D.bc_off + D.soff;
  d.out = t;
  d.ckpt_off = band_pack(b.dlo, b.dhi);
  cand[t] = d;
  kc[t] = (uint8_t)K;
  s_count(lc, SC_ALLELE_BANDED2);
  });
}

struct DecompOutDev {
  int32_t *status, *score_fwd, *score_rev, *score_trim;
  uint8_t* forward;
  uint32_t *slice_begin[2], *slice_len[2], *ref_pos[2];
  int32_t* score[3];
  uint32_t* ops_len[3];
};
// ... with the per-trace results the decompose kernels write themselves (host side only: DecompFields walks all of them)
struct DecompResDev : DecompOutDev {
  tracyhip_breakpoint* bp;
  tracyhip_decomp_status* dstatus;
  double* fractions;
};
// the certificate of the allele 1 vs allele 2 band, and the per-trace results
__global__ void s_decompose_finish_kernel(SParams p, const STrace* __restrict__ tr, const SAllele* __restrict__ al, const int32_t* __restrict__ ascore,
                                          const uint32_t* __restrict__ alen, const long long* __restrict__ bound, uint32_t* __restrict__ dead, DecompOutDev o,
                                          unsigned long long* __restrict__ cnt) {
  with_counters(cnt, [&](unsigned long long* lc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.nt || dead[t]) return;
  if (!s_a12_certified(o.score[2][t], bound[t], o.ops_len[2][t])) { dead[t] |= SD_A12_CHECK; s_count(lc, SC_ALLELE_REPEATED2); return; }
  const STrace S = tr[t];
  o.score_fwd[t] = S.sc[0];
  o.score_rev[t] = S.sc[1];
  o.forward[t] = S.fwd;
  for (uint32_t k = 0; k < 2; ++k) {
    const SAllele A = al[k * p.nt + t];
    o.slice_begin[k][t] = A.trim.ri;
    o.slice_len[k][t] = A.trim.len;
    o.ref_pos[k][t] = A.trim.pos;
    o.score[k][t] = ascore[k * p.nt + t];
    o.ops_len[k][t] = alen[k * p.nt + t];
  }
  });
}

// the basecalls of the dead traces as they were before decomposeAlleles rewrote them (the host-planned pipeline starts from them)
__global__ __launch_bounds__(64) void s_restore_kernel(const uint32_t* __restrict__ list, const SGeom* __restrict__ geom, const SGeomD* __restrict__ geomd,
                                                       const uint8_t* __restrict__ pri_bak, const uint8_t* __restrict__ sec_bak, uint8_t* __restrict__ pri,
                                                       uint8_t* __restrict__ sec) {
  const uint32_t t = list[blockIdx.x];
  const uint64_t off = geomd[t].bc_off;
  for (uint32_t i = threadIdx.x; i < geom[t].mf; i += 64) { pri[off + i] = pri_bak[off + i]; sec[off + i] = sec_bak[off + i]; }
}

struct DecompArena {
  StreamCommon sc;
  SGeomD* geomd;
  BpDesc* bpd; RowsDesc* rowsd; DecompDesc* dd; BcDesc* bcd; B16TableDesc* atd;
  PairDesc* desc_trim;
  uint64_t* off1;          // ops / rows of the trimmed trace, per trace
  uint64_t* aops_off;      // ops of allele k of trace t, relative to the ops of allele 0 (2 nt)
  uint64_t* ops2_off;      // ops of allele 1 vs allele 2
  uint8_t *ops1, *rows0, *rows1;
  uint32_t* len1;
  int32_t *sb, *hst;
  uint8_t *seqs2, *cq_ref, *cq_sd, *cq_special, *pri_bak, *sec_bak;
  int32_t* cq_flag;
  SAllele* al;
  int32_t* ascore; uint32_t* alen;
  long long* bound;
  // staged payloads / results where the caller's arrays are host memory
  float* in_prof; uint8_t* in_ref; int32_t *in_sig, *in_pos;
  int32_t* peaks;          // the peak table of the batch (decompose_kernels.hip): built from the chromatograms, or the caller's staged here (host memory)
  uint8_t *pri, *sec, *secdecomp;
  int32_t *dcp_indel, *dcp_err;
  DecompResDev o;
  uint8_t* ops[3];
  // compact results of the dead traces
  DecompResDev f;
  uint32_t* dead_list;
  struct Sizes { uint32_t nt; bool exact, host, own_peaks; uint64_t tot1, bext, er, ep, sext, dext, opscap[3]; };  // own_peaks: no table from the caller, or one in host memory
  void layout(Arena& a, const Sizes& z) {
    const uint32_t nt = z.nt;
    sc.layout(a, nt, 2 * nt, z.exact, false);
    geomd = a.take<SGeomD>(nt);
    bpd = a.take<BpDesc>(nt); rowsd = a.take<RowsDesc>(nt); dd = a.take<DecompDesc>(nt); bcd = a.take<BcDesc>(nt); atd = a.take<B16TableDesc>(2 * (size_t)nt);
    desc_trim = a.take<PairDesc>(nt);
    off1 = a.take<uint64_t>(nt); aops_off = a.take<uint64_t>(2 * (size_t)nt); ops2_off = a.take<uint64_t>(nt);
    ops1 = a.take<uint8_t>(z.tot1); rows0 = a.take<uint8_t>(z.tot1); rows1 = a.take<uint8_t>(z.tot1);
    len1 = a.take<uint32_t>(nt);
    sb = a.take<int32_t>(nt); hst = a.take<int32_t>(nt);
    seqs2 = a.take<uint8_t>(2 * z.bext + 16);
    cq_ref = a.take<uint8_t>(z.er + 2 * kCodePad); cq_sd = a.take<uint8_t>(z.bext + 2 * kCodePad); cq_special = a.take<uint8_t>((z.er >> 8) + 2);
    pri_bak = a.take<uint8_t>(z.bext); sec_bak = a.take<uint8_t>(z.bext);
    cq_flag = a.take<int32_t>(4);
    al = a.take<SAllele>(2 * (size_t)nt);
    ascore = a.take<int32_t>(2 * (size_t)nt); alen = a.take<uint32_t>(2 * (size_t)nt);
    bound = a.take<long long>(nt);
    peaks = z.own_peaks ? a.take<int32_t>(4 * z.bext + 4) : nullptr;
    o = DecompResDev{};
    if (z.host) {
      in_prof = a.take<float>(z.ep); in_ref = a.take<uint8_t>(z.er); in_sig = a.take<int32_t>(z.sext); in_pos = a.take<int32_t>(z.sext ? z.bext : 0);  // (sext = 0: the caller passed the peak table)
      pri = a.take<uint8_t>(z.bext); sec = a.take<uint8_t>(z.bext); secdecomp = a.take<uint8_t>(z.bext);
      dcp_indel = a.take<int32_t>(z.dext); dcp_err = a.take<int32_t>(z.dext);
      carve_all<DecompFields>(a, nt, o);
      // (the three ops buffers back to back: the offsets of alleles 1 and 2 are taken relative to the first)
      for (int k = 0; k < 3; ++k) ops[k] = a.take<uint8_t>(z.opscap[k]);
    }
    carve_all<DecompFields>(a, nt, f);
    dead_list = a.take<uint32_t>(nt);
  }
};

static_assert(sizeof(tracyhip_breakpoint) == sizeof(BreakpointOut) && sizeof(tracyhip_decomp_status) == sizeof(DecompOut), "result records of the C ABI are the kernels'");

}  // namespace

namespace {
// One stream-ordered tracyhip_decompose_traces call: what its sections share, one method per section (queued in this order)
struct DecStream : StreamCall {
  const tracyhip_decompose_job* job;
  const tracyhip_decompose_result* out;
  const tracyhip_basecalls& bc;
  const tracyhip_decomp_params& dp;
  tracyhip_params pglobal;
  SGeomD* geomd = nullptr;
  DecompArena::Sizes z{};
  uint32_t maxbc = 0, maxsl = 0, max_arest = 0;
  uint64_t atab_tot = 0, alr_tot = 0, rows_alleles = 0;
  DecompArena A;
  const float* d_prof = nullptr;
  const uint8_t* d_ref = nullptr;
  const int32_t *d_sig = nullptr, *d_pos = nullptr, *d_peaks = nullptr;
  bool build_peaks = false;   // no table from the caller: peaks_kernel fills A.peaks (beside the sweeps when the context has side streams)
  bool peaks_forked = false;  // ... on side[3]; the call's stream waits for ready[1] before generateSecondaryDecomposed
  uint8_t *d_pri = nullptr, *d_sec = nullptr, *d_sd = nullptr;
  int32_t *d_di = nullptr, *d_de = nullptr;
  DecompResDev o{};
  uint8_t* d_opsK[3] = {nullptr, nullptr, nullptr};
  SParamsD spd{};
  dim3 g256x2;
  const int16_t* d_aqp = nullptr;
  uint8_t *d_cq_ref = nullptr, *d_cq_sd = nullptr;
  int32_t* hcq = nullptr;  // the verdict of the case-sensitive encoders
  bool af_forked = false;    // allelicFraction is on a side stream (joined before the read-back)
  bool af_pending = false;   // ... not queued yet (queue_allelic_fraction)
  bool bp_early = false;     // findBreakpoint and the windows' case-sensitive codes were queued behind the full sweeps (OrientStage::filler)
  bool cq_ref_done = false;
  bool encoded_early = false;

  DecStream(tracyhip_ctx* c, const tracyhip_decompose_job* j, const tracyhip_params* q, int m, const tracyhip_decompose_result* o_, StreamHost& h_)
      : StreamCall(c, j, q, m, h_), job(j), out(o_), bc(j->bc), dp(j->dprm), pglobal(*q),
        g256x2((2 * j->ntraces + 255) / 256) {
    pglobal.hfree = 0;  // AlignConfig<false,false> (indigo.h:381)
    pglobal.vfree = 0;
  }
  // whatever happens once the stages are queued, the caller's basecalls in device memory are put back before the host-planned pipeline takes the call
  int give_up(int rc) {
    if (rc != TRACYHIP_OK) af_pending = false;  // (the host-planned pipeline redoes the call)
    if (rc != TRACYHIP_OK && peaks_forked) { (void)hipStreamWaitEvent(st, ctx->b16_fork.ready[1], 0); peaks_forked = false; }
    if (rc != TRACYHIP_OK && af_forked) {  // (nothing of this call may still run when the caller -- or the host-planned pipeline -- takes the buffers back)
      (void)hipStreamWaitEvent(st, ctx->b16_fork.joined[3], 0);
      af_forked = false;
      if (rc != kStreamNo || host) (void)ctx_sync(ctx);
    }
    if (rc == kStreamNo && !host) {
      (void)hipMemcpyAsync(d_pri, A.pri_bak, z.bext, hipMemcpyDeviceToDevice, st);
      (void)hipMemcpyAsync(d_sec, A.sec_bak, z.bext, hipMemcpyDeviceToDevice, st);
      (void)ctx_sync(ctx);
    }
    return rc;
  }

  // payloads in device memory: the encoder needs nothing the planner makes -- it runs while the host lays out the geometry records
  // (2 ms for 100 000 traces during which the device had nothing to do).  Harmless should the planner hand the call back.
  int encode_early() {
    if (host) return TRACYHIP_OK;
    TRY(encode_references(static_cast<const uint8_t*>(sr.data), seqset_extent(sr)));
    encoded_early = true;
    return TRACYHIP_OK;
  }

  // what the host knows before anything runs: geometry of every trace (laid out in the pinned block it travels from), workspace
  int plan() {
    // geometry and offsets are laid out in the pinned block they travel from
    HIP_TRY(ctx->pin[PB_DESC].ensure((sizeof(SGeom) + sizeof(SGeomD)) * (size_t)nt));
    geom = static_cast<SGeom*>(ctx->pin[PB_DESC].p);
    geomd = reinterpret_cast<SGeomD*>(geom + nt);
    // ---- geometry of the decompose stages (decompose_traces_legacy's, trace by trace): sums, extents and checks per slice of the batch, then
    // the records with their running offsets from the slices' bases -- inside plan_common's two passes (PlanHooks) ----
    z.nt = nt; z.exact = exact; z.host = host;
    if (!bc.peaks && (!bc.signal || !bc.signal_offset || !bc.nsamples || !bc.bcpos)) return set_error(TRACYHIP_ERR_ARG, "null basecall arrays: neither a peak table nor signal + bcpos");
    z.own_peaks = !bc.peaks || host;
    struct Part {
      uint64_t atab = 0, alr = 0, tot1 = 0, sext = 0, bext = 0, dext = 0, opscap[3] = {0, 0, 0}, rows_alleles = 0, rows_traces = 0;
      uint32_t maxbc = 0, maxsl = 0, max_arest = 0, bad_len = ~0u, bad_range = ~0u;
    };
    Part part[kHostThreads];
    auto trimmed = [&](uint32_t t, uint32_t& soff, uint32_t& sl) {  // trimmedSeq, abif.h:68-75
      const uint32_t l = trims.left(t), r = trims.right(t);
      if ((uint64_t)(uint32_t)(l + r + 1) >= (uint64_t)h.mf[t]) { soff = 0; sl = h.mf[t]; }
      else { soff = l; sl = h.mf[t] - l - r; }
    };
    auto front_ok = [&](uint32_t t, uint32_t sl) { return s_front_ok(&p, sl, h.rn[t]); };
    uint64_t base_atab[kHostThreads], base_alr[kHostThreads], base_tot1[kHostThreads];
    uint64_t rows_traces = 0;
    PlanHooks hooks;
    hooks.lengths_slice = [&](uint32_t lo, uint32_t hi, uint32_t tid) {
      Part x;
      for (uint32_t t = lo; t < hi; ++t) {
        if (bc.bc_len[t] != h.mf[t]) x.bad_len = std::min(x.bad_len, t);
        if (bc.bc_len[t] >= 2u * kMaxIndelGlobal) x.bad_range = std::min(x.bad_range, t);
        uint32_t soff, sl;
        trimmed(t, soff, sl);
        x.atab += 2ull * kB16Codes * b16_table_stride(sl);
        x.alr += 2ull * ((uint64_t)h.rn[t] + 2);
        x.tot1 += (uint64_t)h.mt[t] + h.rn[t];
        if (front_ok(t, sl)) x.max_arest = std::max(x.max_arest, sl - kFrontRows);
        if (!bc.peaks) x.sext = std::max<uint64_t>(x.sext, bc.signal_offset[t] + 4ull * bc.nsamples[t]);
        x.bext = std::max<uint64_t>(x.bext, bc.bc_offset[t] + bc.bc_len[t]);
        x.dext = std::max<uint64_t>(x.dext, out->dcp_offset[t] + 2ull * dp.maxindel + 2);
        for (int k = 0; k < 3; ++k) x.opscap[k] = std::max<uint64_t>(x.opscap[k], out->ops_offset[k][t] + (uint64_t)sl + (k < 2 ? h.rn[t] : sl));
        x.maxbc = std::max(x.maxbc, h.mf[t]);
        x.maxsl = std::max(x.maxsl, sl);
        x.rows_alleles += 2ull * sl;
        x.rows_traces += h.mt[t];
      }
      part[tid] = x;
    };
    hooks.between = [&]() -> int {
      uint32_t bad_len = ~0u, bad_range = ~0u;
      for (const Part& x : part) { bad_len = std::min(bad_len, x.bad_len); bad_range = std::min(bad_range, x.bad_range); }
      const uint32_t first_bad = std::min(bad_len, bad_range);  // (the first offending trace, as a loop over the traces would report it)
      if (first_bad != ~0u) {
        if (bc.bc_len[first_bad] != h.mf[first_bad])
          return set_error(TRACYHIP_ERR_ARG, "trace %u: profile has %u columns but %u basecalls", first_bad, h.mf[first_bad], bc.bc_len[first_bad]);
        return set_error(TRACYHIP_ERR_RANGE, "trace %u has %u basecalls; the scan tables hold < %d", first_bad, bc.bc_len[first_bad], 2 * kMaxIndelGlobal);
      }
      for (uint32_t i = 0; i < kHostThreads; ++i) {
        const Part& x = part[i];
        base_atab[i] = atab_tot; base_alr[i] = alr_tot; base_tot1[i] = z.tot1;
        atab_tot += x.atab; alr_tot += x.alr; z.tot1 += x.tot1;
        z.sext = std::max(z.sext, x.sext); z.bext = std::max(z.bext, x.bext); z.dext = std::max(z.dext, x.dext);
        for (int k = 0; k < 3; ++k) z.opscap[k] = std::max(z.opscap[k], x.opscap[k]);
        maxbc = std::max(maxbc, x.maxbc); maxsl = std::max(maxsl, x.maxsl); max_arest = std::max(max_arest, x.max_arest);
        rows_alleles += x.rows_alleles;
        rows_traces += x.rows_traces;
      }
      return TRACYHIP_OK;
    };
    hooks.records_slice = [&](uint32_t lo, uint32_t hi, uint32_t tid) {
      uint64_t atab = base_atab[tid], alr = base_alr[tid], tot1 = base_tot1[tid];
      for (uint32_t t = lo; t < hi; ++t) {
        SGeomD& D = geomd[t];
        D = SGeomD{};
        trimmed(t, D.soff, D.sl);
        D.bc_off = bc.bc_offset[t];
        D.sig_off = bc.peaks ? 0ull : bc.signal_offset[t];
        D.nsamples = bc.peaks ? 0u : bc.nsamples[t];
        D.dcp_off = out->dcp_offset[t];
        for (int k = 0; k < 3; ++k) D.opsk_off[k] = out->ops_offset[k][t];
        D.atab_stride = b16_table_stride(D.sl);
        const bool ok = front_ok(t, D.sl);
        for (int k = 0; k < 2; ++k) {
          D.atab_off[k] = atab; atab += (uint64_t)kB16Codes * D.atab_stride;
          D.alr_off[k] = alr; alr += (uint64_t)h.rn[t] + 2;
          D.flags[k] = ok ? SG_FRONT_OK : 0u;
        }
        geom[t].ops_off = tot1;
        tot1 += (uint64_t)h.mt[t] + h.rn[t];
      }
    };
    TRY(plan_common(ctx, p, sp, sr, job->ref_index, nt, trims, h, geom, &hooks));
    if (max_arest == 0 || !front_tiers_fit(max_arest)) return kStreamNo;
    TRY(decompose_limits(dp.maxindel, maxbc));
    z.ep = seqset_extent(sp); z.er = seqset_extent(sr);
    TRY(size_ncap());

    // ---- workspace ----
    TRACYHIP_HOST_SCOPE(hs6, "plan.workspace");
    Arena sizing;
    A.layout(sizing, z);
    TRY(with_fresh_budget(ctx, [&](bool* from_cache) -> int {
      uint64_t budget = 0;
      TRY(workspace_budget(ctx, ctx->dev[DB_LASTROW].cap + ctx->dev[DB_BITS].cap + ctx->dev[DB_STREAM].cap + ctx->dev[DB_B16TAB_PROFILE].cap + ctx->dev[DB_B16TAB_ALLELE0].cap, &budget, from_cache));
      const uint64_t lr_words = std::max(h.lr_tot, alr_tot);
      const uint64_t fixed = lr_words * 4 + 64 + h.tab_tot * 2 + atab_tot * 2 + 128 + sizing.off;
      if (fixed > budget) return kStreamNo;
      words_cap = band_words_cap(std::max(rows_traces, rows_alleles), 2ull * nt, budget - fixed);
      HIP_TRY(ctx->dev[DB_LASTROW].ensure(lr_words * 4 + 64));
      HIP_TRY(ctx->dev[DB_B16TAB_PROFILE].ensure(h.tab_tot * sizeof(int16_t) + 64));
      HIP_TRY(ctx->dev[DB_B16TAB_ALLELE0].ensure(atab_tot * sizeof(int16_t) + 64));
      HIP_TRY(ctx->dev[DB_BITS].ensure(words_cap + 64));
      HIP_TRY(ctx->dev[DB_STREAM].ensure(sizing.off + 256));
      return TRACYHIP_OK;
    }));
    Arena arena;
    arena.base = static_cast<char*>(ctx->dev[DB_STREAM].p);
    A.layout(arena, z);

    return TRACYHIP_OK;
  }

  // payloads and result arrays: the caller's (device memory) or staged; references encoded; geometry uploaded
  int bind() {
    StreamCommon& sc = A.sc;
    // ---- payloads and result arrays: the caller's (device memory) or staged ----
    d_prof = static_cast<const float*>(sp.data);
    d_ref = static_cast<const uint8_t*>(sr.data);
    d_sig = bc.signal; d_pos = bc.bcpos;
    d_peaks = bc.peaks ? bc.peaks : A.peaks;
    build_peaks = !bc.peaks;
    d_pri = bc.primary; d_sec = bc.secondary; d_sd = out->secdecomp;
    d_di = out->dcp_indel; d_de = out->dcp_err;
    o = A.o;
    for (int k = 0; k < 3; ++k) d_opsK[k] = out->ops[k];
    if (host) {
      auto up = [&](void* dev, const void* src, size_t bytes) -> int {
        if (bytes) HIP_TRY(hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, st));
        return TRACYHIP_OK;
      };
      TRY(up(A.in_prof, sp.data, z.ep * 4)); TRY(up(A.in_ref, sr.data, z.er));
      if (bc.peaks) { TRY(up(A.peaks, bc.peaks, z.bext * 16)); d_peaks = A.peaks; }  // (16 bytes per basecall instead of the chromatogram)
      else { TRY(up(A.in_sig, bc.signal, z.sext * 4)); TRY(up(A.in_pos, bc.bcpos, z.bext * 4)); }
      TRY(up(A.pri, bc.primary, z.bext)); TRY(up(A.sec, bc.secondary, z.bext));
      d_prof = A.in_prof; d_ref = A.in_ref; d_sig = A.in_sig; d_pos = A.in_pos; d_pri = A.pri; d_sec = A.sec; d_sd = A.secdecomp;
      d_di = A.dcp_indel; d_de = A.dcp_err;
      // a table holds dcp_n entries of its 2 maxindel + 2 and the whole region goes back to the caller: the rest is zero, not what the arena held
      HIP_TRY(hipMemsetAsync(d_di, 0, z.dext * 4, st)); HIP_TRY(hipMemsetAsync(d_de, 0, z.dext * 4, st));
      for (int k = 0; k < 3; ++k) d_opsK[k] = A.ops[k];
    } else {
      point_all<DecompFields>(o, *out);
    }
    HIP_TRY(hipMemcpyAsync(A.pri_bak, d_pri, z.bext, hipMemcpyDeviceToDevice, st));  // decomposeAlleles rewrites the basecalls in place
    HIP_TRY(hipMemcpyAsync(A.sec_bak, d_sec, z.bext, hipMemcpyDeviceToDevice, st));

    // ---- references encoded once (unless encode_early did it while the host planned); the records: one pinned block, two copies ----
    if (!encoded_early) TRY(encode_references(d_ref, z.er));
    // (the offset arrays of the band launches are filled from these records on the device: s_expand_d_kernel)
    TRY(upload_records(sc, A.geomd, sizeof(SGeomD) * (size_t)nt));

    fill_params();
    spd.bext = z.bext;
    spd.best = (int32_t)std::max<int64_t>(std::max<int64_t>(p.match, p.mismatch), 0);

    return TRACYHIP_OK;
  }

  int queue_trace_stages() {
    StreamCommon& sc = A.sc;
    // ---- 2. orientation (indigo.h:235-247), 3. gotoh(trimmed trace, window) (indigo.h:302) by traceback on its band ----
    OrientStage os{d_prof, d_qp, d_lastrow, exact, A.desc_trim};
    // the descriptors of the decompose stages need nothing but the geometry records; findBreakpoint (indigo.h:196) nothing but the profiles:
    // it runs on a side stream beside the sweeps and is waited for where its result is first read (findHomozygousBreakpoint)
    hipLaunchKernelGGL(s_expand_d_kernel, g256, b256, 0, st, sc.geom, A.geomd, nt, z.bext, A.bpd, A.rowsd, A.dd, A.bcd, A.atd, A.off1, A.aops_off, A.ops2_off,
                       (uint64_t)(reinterpret_cast<uintptr_t>(d_opsK[1]) - reinterpret_cast<uintptr_t>(d_opsK[0])));
    HIP_TRY(hipGetLastError());
    // findBreakpoint (indigo.h:196) needs nothing but the profiles, the case-sensitive codes of the windows (the allele stages' columns)
    // nothing but the references: both fill the hole behind the full sweeps (OrientStage::filler)
    // the peak table (no table from the caller): one pass over the chromatograms -- HBM work that needs no LDS and few registers, on the
    // lowest-priority side stream beside the sweeps, which leave the memory system idle; joined before generateSecondaryDecomposed
    if (build_peaks && ctx->b16_fork_ok && !ctx->knobs.no_fork) {
      const B16Fork& fk = ctx->b16_fork;
      HIP_TRY(hipEventRecord(fk.forked, st));
      HIP_TRY(hipStreamWaitEvent(fk.side[3], fk.forked, 0));
      ctx->stream = fk.side[3];
      const int rcp = launch_peaks(ctx, A.bcd, nt, maxbc, d_sig, d_pos, A.peaks);
      ctx->stream = st;
      HIP_TRY(hipEventRecord(fk.ready[1], fk.side[3]));
      peaks_forked = true;
      if (rcp) return rcp;
      build_peaks = false;
    }
    bp_early = ctx->b16_fork_ok && !ctx->knobs.no_fork;
    if (bp_early)
      os.filler = [&]() -> int {
        TRY(launch_breakpoint(ctx, A.bpd, nt, h.maxmt, d_prof, reinterpret_cast<BreakpointOut*>(o.bp)));
        return encode_windows_cq();
      };
    TRY(give_up(queue_orientation(ctx, p, spm, h, sc, os)));
    hipLaunchKernelGGL(s_prelim_plan_kernel, g256, b256, 0, st, spm, 1, 0, sc.geom, sc.tr, sc.ce, sc.top_trim, sc.dead, sc.cand, sc.kc, 0);
    HIP_TRY(hipGetLastError());
    BandStageArgs b0;
    b0.kind = 0; b0.qp = d_qp; b0.codes = ctx->codes(); b0.scores = A.sb; b0.ops = A.ops1; b0.ops_off = A.off1; b0.ops_len = A.len1; b0.code_cap = ncap; b0.hfree = 1;
    TRY(band_stage(ctx, p, sc, nt, nt, 0, b0, words_cap));
    hipLaunchKernelGGL(s_prelim_check_kernel, g256, b256, 0, st, spm, sc.tr, A.sb, A.len1, sc.kc, o.score_trim, sc.dead, sc.cnt);
    HIP_TRY(hipGetLastError());
    // ---- 1. findBreakpoint (indigo.h:196), unless it already ran behind the full sweeps ----
    BreakpointOut* bpo = reinterpret_cast<BreakpointOut*>(o.bp);
    if (!bp_early) TRY(launch_breakpoint(ctx, A.bpd, nt, h.maxmt, d_prof, bpo));
    {
      RowsArgs ra{};
      ra.pairs = A.desc_trim;
      ra.a1 = d_prof; ra.a2 = d_ref;
      ra.a1_profile = 1; ra.a2_profile = 0; ra.a2_revcomp_flag = 1; ra.a2_onehot = 1;
      ra.ops = A.ops1; ra.ops_off = A.off1; ra.ops_len = A.len1;
      ra.rows0 = A.rows0; ra.rows1 = A.rows1;
      ra.npairs = nt;
      // a trace with a shift (findBreakpoint) skips findHomozygousBreakpoint, and decomposeAlleles only asks where row 0 has gaps: the
      // consensus characters of its profile columns -- six reads per column -- are left out for it
      static_assert(offsetof(BreakpointOut, indelshift) == 0 && sizeof(BreakpointOut) == 16, "layout");
      ra.row0_gaps_only = reinterpret_cast<const int32_t*>(bpo);
      ra.row0_gaps_only_stride = 4;
      HIP_TRY(launch_alignment_rows(ra, st));
    }
    // ---- 4. findHomozygousBreakpoint (indigo.h:314-317), 5. decomposeAlleles, generateSecondaryDecomposed, allelicFraction (indigo.h:340-350) ----
    TRY(launch_homozygous(ctx, A.rowsd, A.rows0, A.rows1, nt, bpo, A.hst, A.len1));
    {
      DecompArgs a{};
      a.desc = A.dd;
      a.rows0 = A.rows0; a.rows1 = A.rows1;
      a.primary = d_pri; a.secondary = d_sec;
      a.dcp_indel = d_di; a.dcp_err = d_de;
      a.out = reinterpret_cast<DecompOut*>(o.dstatus);
      a.prm = DecompParams{dp.trim_left, dp.trim_right, dp.maxindel, dp.madc};
      a.ntraces = nt;
      a.lens = A.len1;
      a.skip = sc.dead;
      TRY(launch_decompose(ctx, a, bpo, maxbc, 0, 0));
      if (build_peaks) { TRY(launch_peaks(ctx, A.bcd, nt, maxbc, d_sig, d_pos, A.peaks)); build_peaks = false; }
      if (peaks_forked) { HIP_TRY(hipStreamWaitEvent(st, ctx->b16_fork.ready[1], 0)); peaks_forked = false; }
      TRY(launch_secdecomp(ctx, A.bcd, nt, maxbc, d_peaks, d_pri, d_sec, d_sd));
      // allelicFraction feeds nothing but its own result (indigo.h:350): it runs beside the allele stages, which read the same
      // decomposed basecalls and write elsewhere; the read-back waits for it.  It is QUEUED once the allele stages' first long launch is
      // (queue_allelic_fraction): beside the encoders' fills and copies it would only make those wait for its hundred thousand waves.
      af_pending = ctx->b16_fork_ok && !ctx->knobs.no_fork;
      if (!af_pending) TRY(queue_allelic_fraction());
    }
    hipLaunchKernelGGL(s_status_kernel, g256, b256, 0, st, spm, sc.geom, o.score_trim, A.hst, A.len1, sc.dead, o.status, sc.cnt);
    HIP_TRY(hipGetLastError());

    return TRACYHIP_OK;
  }

  // allelicFraction (indigo.h:350) on the low-priority side stream, behind the point of the call's stream at which the decomposed basecalls
  // were complete (ready[0]); on the call's stream itself without side streams
  // case-sensitive codes of the reference windows (MODE_CQ columns of the allele stages), their block map and the verdict words: once
  int encode_windows_cq() {
    if (cq_ref_done) return TRACYHIP_OK;
    cq_ref_done = true;
    d_cq_ref = A.cq_ref + kCodePad;
    HIP_TRY(hipMemsetAsync(A.cq_ref, 5, kCodePad, st));
    HIP_TRY(hipMemsetAsync(A.cq_ref + kCodePad + z.er, 5, kCodePad, st));
    HIP_TRY(hipMemsetAsync(A.cq_special, 0, (z.er >> 8) + 2, st));
    HIP_TRY(hipMemsetAsync(A.cq_flag, 0, sizeof(int32_t) * 4, st));
    if (z.er) hipLaunchKernelGGL(encode_cq_kernel, dim3((unsigned)((z.er + 4095) / 4096)), dim3(256), 0, st, d_ref, d_cq_ref, z.er, A.cq_flag, A.cq_special);
    HIP_TRY(hipGetLastError());
    return TRACYHIP_OK;
  }

  int queue_allelic_fraction() {
    const bool fork = af_pending;
    af_pending = false;
    if (fork) {
      HIP_TRY(hipStreamWaitEvent(ctx->b16_fork.side[3], ctx->b16_fork.ready[0], 0));
      ctx->stream = ctx->b16_fork.side[3];
    }
    const int rc = launch_allelic_fraction(ctx, A.bcd, nt, maxbc, d_peaks, d_pri, d_sd, o.fractions, 18ull * std::accumulate(h.mf.begin(), h.mf.end(), 0ull), z.bext);
    ctx->stream = st;
    if (fork) {
      HIP_TRY(hipEventRecord(ctx->b16_fork.joined[3], ctx->b16_fork.side[3]));
      af_forked = true;
    }
    return rc;
  }

  int queue_allele_stages() {
    StreamCommon& sc = A.sc;
    // ---- 6. allele-specific alignments (indigo.h:355-387), both alleles of every trace in the same launches ----
    // strings scored through the query-profile table (MODE_CQ): the two allele strings side by side, case-sensitive codes of the windows
    // and of allele 2, the test that the rows hold A C G T N only (read with the call's verdict words)
    d_cq_sd = A.cq_sd + kCodePad;
    HIP_TRY(hipMemcpyAsync(A.seqs2, d_pri, z.bext, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(A.seqs2 + z.bext, d_sd, z.bext, hipMemcpyDeviceToDevice, st));
    TRY(encode_windows_cq());
    // (the encoders write every code byte: only the spare bytes on both sides are filled)
    HIP_TRY(hipMemsetAsync(A.cq_sd, 5, kCodePad, st));
    HIP_TRY(hipMemsetAsync(A.cq_sd + kCodePad + z.bext, 5, kCodePad, st));
    if (z.bext) {
      hipLaunchKernelGGL(encode_cq_kernel, dim3((unsigned)((z.bext + 4095) / 4096)), dim3(256), 0, st, static_cast<const uint8_t*>(d_sd), d_cq_sd, z.bext, A.cq_flag, (uint8_t*)nullptr);
      hipLaunchKernelGGL(cq_rows_kernel, dim3((unsigned)((2 * z.bext + 4095) / 4096)), dim3(256), 0, st, static_cast<const uint8_t*>(A.seqs2), 2 * z.bext, A.cq_flag);
    }
    HIP_TRY(hipGetLastError());
    d_aqp = static_cast<const int16_t*>(ctx->dev[DB_B16TAB_ALLELE0].p);
    TRY(timing_begin(ctx, TRACYHIP_TIMER_MISC, 0, atab_tot * 2));
    HIP_TRY(launch_b16_tables(A.atd, 2 * nt, A.seqs2, true, p.match, p.mismatch, sub_limit(&p), kTagShift, const_cast<int16_t*>(d_aqp), static_cast<int32_t*>(ctx->dev[DB_ERR].p), st));
    TRY(timing_end(ctx));
    // (shared kept rows leave holes in the prefix launch: its pairs as a list, as for the later tiers)
    const bool share = !kn.no_front_lists && 2 * nt >= kn.front_list_min;
    hipLaunchKernelGGL(s_allele_plan0_kernel, g256x2, b256, 0, st, spm, spd, sc.geom, A.geomd, sc.tr, sc.dead, sc.pre, sc.fd, static_cast<const uint8_t*>(A.seqs2),
                       share ? 1 : 0, sc.cnt);
    HIP_TRY(hipGetLastError());
    if (share) {
      HIP_TRY(hipMemsetAsync(sc.fcount + 2, 0, sizeof(uint32_t), st));
      hipLaunchKernelGGL(s_pair_list_kernel, g256x2, b256, 0, st, 2 * nt, sc.pre, sc.flist, sc.fcount + 2);
      HIP_TRY(hipGetLastError());
    }
    {
      DpArgs a = scoring_args(ctx, &p);
      a.pairs = sc.pre;
      if (share) { a.index = sc.flist; a.count = sc.fcount + 2; }
      a.a1 = A.seqs2; a.a2 = d_cq_ref;
      a.special_blocks = kn.no_compact ? nullptr : A.cq_special;
      a.lastrow = d_lastrow;
      // (the side stream starts where the call's stream is NOW: allelicFraction begins with the prefixes, not with the fills and copies)
      if (af_pending) HIP_TRY(hipEventRecord(ctx->b16_fork.ready[0], st));
      TRY(timing_begin(ctx, TRACYHIP_TIMER_SCORE, 0, 0));
      HIP_TRY(launch_gotoh_front_prefix_cq(a, 2 * nt, st, ctx->knobs.prefix_tall_min));
      TRY(timing_end(ctx));
    }
    if (af_pending) TRY(give_up(queue_allelic_fraction()));
    TRY(timing_begin(ctx, TRACYHIP_TIMER_FRONT, 0, 0));
    {
      int rc = front_tiers_run(ctx, p, sc, 2 * nt, d_aqp, d_cq_ref, reinterpret_cast<const uint32_t*>(d_lastrow), max_arest);
      if (rc) return give_up(rc);
    }
    TRY(timing_end(ctx));
    hipLaunchKernelGGL(s_allele_plan1_kernel, g256x2, b256, 0, st, spm, spd, sc.geom, A.geomd, sc.tr, sc.fo1, sc.fs1, sc.fe1, sc.fo2, sc.fs2, sc.fe2, A.al, sc.dead, sc.cand,
                       sc.kc, sc.cnt);
    HIP_TRY(hipGetLastError());
    BandStageArgs b1;
    b1.kind = 1; b1.qp = d_aqp; b1.codes = d_cq_ref; b1.ends = sc.ends; b1.code_cap = ncap; b1.hfree = 1;
    TRY(band_stage(ctx, p, sc, 2 * nt, nt, 1, b1, ~0ull));
    hipLaunchKernelGGL(s_allele_plan2_kernel, g256x2, b256, 0, st, spm, sc.geom, A.geomd, sc.tr, sc.ends, A.al, sc.dead, sc.cand, sc.kc, kn.no_origin_band ? 0 : 1, sc.cnt);
    HIP_TRY(hipGetLastError());
    BandStageArgs b2;
    b2.kind = 0; b2.qp = d_aqp; b2.codes = d_cq_ref; b2.scores = A.ascore; b2.ops = d_opsK[0]; b2.ops_off = A.aops_off; b2.ops_len = A.alen; b2.code_cap = ncap; b2.hfree = 1;
    TRY(band_stage(ctx, p, sc, 2 * nt, nt, 2, b2, words_cap));
    hipLaunchKernelGGL(s_allele_check_kernel, g256x2, b256, 0, st, spm, A.al, A.ascore, A.alen, sc.dead, sc.cnt);
    hipLaunchKernelGGL(s_a12_plan_kernel, g256, b256, 0, st, spm, spd, A.geomd, A.ascore, sc.dead, sc.cand, sc.kc, A.bound, sc.cnt);
    HIP_TRY(hipGetLastError());
    BandStageArgs b3;
    b3.kind = 0; b3.qp = d_aqp; b3.codes = d_cq_sd; b3.scores = o.score[2]; b3.ops = d_opsK[2]; b3.ops_off = A.ops2_off; b3.ops_len = o.ops_len[2]; b3.code_cap = ncap; b3.hfree = 0;
    TRY(band_stage(ctx, pglobal, sc, nt, nt, 3, b3, words_cap));
    const DecompOutDev& ko = o;  // (the kernels' part of o: bp / dstatus / fractions are written by the decompose kernels through their own arguments)
    hipLaunchKernelGGL(s_decompose_finish_kernel, g256, b256, 0, st, spm, sc.tr, A.al, A.ascore, A.alen, A.bound, sc.dead, ko, sc.cnt);
    HIP_TRY(hipGetLastError());

    return TRACYHIP_OK;
  }

  // the one read-back: verdict words, counters, dead flags
  int read_back() {
    if (af_pending) TRY(queue_allelic_fraction());
    if (af_forked) HIP_TRY(hipStreamWaitEvent(st, ctx->b16_fork.joined[3], 0));
    // ---- the one read-back ----
    TRY(rb.carve(ctx, nt, sizeof(int32_t) * 4));
    hcq = static_cast<int32_t*>(rb.extra);
    TRY(rb.queue_verdict(ctx, st));
    HIP_TRY(hipMemcpyAsync(hcq, A.cq_flag, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, st));
    TRY(rb.queue_counters(A.sc, nt, st));
    TRY(await_verdict([this](int rc) { return give_up(rc); }));
    if (hcq[0] & 1) return give_up(kStreamNo);  // a basecall string holds something else than A C G T N: the byte-compare kernels (pipeline.hip)
    static const int stage_timer[4] = {TRACYHIP_TIMER_TRACE, TRACYHIP_TIMER_ORIGIN, TRACYHIP_TIMER_TRACE, TRACYHIP_TIMER_TRACE};
    static const DeadReason reasons[] = {{SD_FRONT, "front"}, {SD_STRAND, "strand"}, {SD_LOSER_WON, "loser won"}, {SD_JUNK, "junk"}, {SD_PRELIM_BAND, "prelim band"},
                                         {SD_PRELIM_CHECK, "prelim check"}, {SD_MEM, "mem"}, {SD_ALLELE_FRONT, "allele front"}, {SD_ALLELE_ORIGIN, "allele origin"},
                                         {SD_ALLELE_BAND, "allele band"}, {SD_ALLELE_CHECK, "allele check"}, {SD_A12_BAND, "a12 band"}, {SD_A12_CHECK, "a12 check"},
                                         {SD_SHAPE, "shape"}};
    list_dead("decompose", A.sc, stage_timer, reasons);
    return TRACYHIP_OK;
  }

  // the traces the device could not give their tier: the host-planned pipeline on the list, from the basecalls as they were
  int redo_dead_traces() {
    if (dl.empty()) return TRACYHIP_OK;
    const uint32_t nd = (uint32_t)dl.size();
    HIP_TRY(hipMemcpyAsync(A.dead_list, dl.data(), sizeof(uint32_t) * nd, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(s_restore_kernel, dim3(nd), dim3(64), 0, st, A.dead_list, A.sc.geom, A.geomd, A.pri_bak, A.sec_bak, d_pri, d_sec);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ctx_sync(ctx));
    std::vector<uint64_t> bcoff(nd), dcpoff(nd), ooff[3];
    std::vector<uint32_t> bclen(nd);
    for (int k = 0; k < 3; ++k) ooff[k].resize(nd);
    for (uint32_t i = 0; i < nd; ++i) {
      const uint32_t t = dl[i];
      bcoff[i] = bc.bc_offset[t]; bclen[i] = bc.bc_len[t];
      dcpoff[i] = out->dcp_offset[t];
      for (int k = 0; k < 3; ++k) ooff[k][i] = out->ops_offset[k][t];
    }
    tracyhip_decompose_job j = *job;
    sub_job(j, d_prof, d_ref);
    j.bc.ntraces = nd;
    // (the peak table of the batch is on the device by now, the caller's or the one built from the chromatograms: the sub-job reads it)
    j.bc.signal = nullptr; j.bc.signal_offset = nullptr; j.bc.nsamples = nullptr; j.bc.bcpos = nullptr; j.bc.peaks = d_peaks;
    j.bc.primary = d_pri; j.bc.secondary = d_sec; j.bc.bc_offset = bcoff.data(); j.bc.bc_len = bclen.data();
    tracyhip_decompose_result r{};
    point_all<DecompFields>(r, A.f);
    r.dcp_indel = d_di; r.dcp_err = d_de; r.dcp_offset = dcpoff.data();
    r.secdecomp = d_sd;
    for (int k = 0; k < 3; ++k) { r.ops[k] = d_opsK[k]; r.ops_offset[k] = ooff[k].data(); }
    TRY(host_planned([&]() { return decompose_traces_legacy(ctx, &j, prm, TRACYHIP_MEM_DEVICE, &r); }));
    TRY(scatter_all<DecompFields>(st, A.dead_list, nd, A.f, o));
    HIP_TRY(ctx_sync(ctx));
    return TRACYHIP_OK;
  }

  // Results to the caller's host arrays.  The per-trace arrays go in the order of DecompFields -- the order of the scatters -- between the
  // arrays laid out by offsets: one list cannot give both the order the scatters had and the order these copies had (bp, fractions, the
  // tables, dstatus, ..., ops[k] behind score[k] / ops_len[k]).  The copies are independent, on one stream, and end in the one
  // synchronisation below: what arrives, and host_syncs, do not depend on their order.
  int copy_back() {
    if (!host) return TRACYHIP_OK;
    TRY(copy_to_host(st, bc.primary, d_pri, z.bext)); TRY(copy_to_host(st, bc.secondary, d_sec, z.bext)); TRY(copy_to_host(st, out->secdecomp, d_sd, z.bext));
    TRY(copy_to_host(st, out->dcp_indel, d_di, z.dext * 4)); TRY(copy_to_host(st, out->dcp_err, d_de, z.dext * 4));
    TRY(copy_back_all<DecompFields>(st, nt, *out, o));
    for (int k = 0; k < 3; ++k) TRY(copy_to_host(st, out->ops[k], d_opsK[k], z.opscap[k]));
    HIP_TRY(ctx_sync(ctx));
    return TRACYHIP_OK;
  }
};
}  // namespace

int tracyhip::stream_decompose(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_params* prm, int mem,
                               const tracyhip_decompose_result* out) {
  if (!stream_options_ok(ctx->knobs) || job->oriented || job->ref_profiles.data) return kStreamNo;
  static thread_local StreamHost h;
  DecStream s(ctx, job, prm, mem, out, h);
  TRY(s.encode_early());
  { TRACYHIP_HOST_SCOPE(hs, "stream_decompose.plan"); TRY(s.plan()); }
  { TRACYHIP_HOST_SCOPE(hs, "stream_decompose.bind"); TRY(s.bind()); }
  { TRACYHIP_HOST_SCOPE(hs, "stream_decompose.queue_trace_stages"); if (int rc = s.queue_trace_stages()) return s.give_up(rc); }    // 2., 3., then 1., 4., 5. (indigo.h:196-350)
  { TRACYHIP_HOST_SCOPE(hs, "stream_decompose.queue_allele_stages"); if (int rc = s.queue_allele_stages()) return s.give_up(rc); }  // 6. (indigo.h:355-387)
  TRACYHIP_HOST_SCOPE(hs_rb, "stream_decompose.read_back_and_after");
  if (int rc = s.read_back()) return s.give_up(rc);            // the call's one synchronisation
  TRY(s.redo_dead_traces());
  return s.copy_back();
}
