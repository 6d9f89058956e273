// stream_plan.h -- what the stream-ordered pipelines (stream.hip) keep on the device between two launches, and the per-trace planning
// rules of both pipelines: which strand the k-mers vote for (R10, in dp_lane.h, where the sweep kernels see it too), which strand to
// prune (R1, R2), whether a strand's bound decides it (R11), which band an alignment's score allows (R3, R5, R7, R8), whether a band
// fits the band kernels (R4), whether a certificate held (R6, R12, R13), trimReferenceSlice's last step (R9).  Each rule is written once, as a
// TR_HD function: the planning kernels of stream.hip (one thread per trace) and the host-planned tiers of pipeline.hip call the same
// ones, so that a trace takes the same tier on either path -- and a trace whose tier the device cannot give it (a failed
// certificate, a band wider than the band kernels hold) is marked `dead` and handed to the host-planned tiers afterwards.  Where the
// two planners differ on purpose, the difference is an argument.  The header compiles for the host alone (tests/cpp/plan_rules.cpp).
#ifndef TRACY_AMD_STREAM_PLAN_H
#define TRACY_AMD_STREAM_PLAN_H

#include "../../include/tracy_hip.h"
#include "band16.h"
#include "front.h"
#include "launch_rules.h"

namespace tracyhip {

// why a trace left the stream-ordered pass (bit set of SDead; tracyhip_call_stats::fallback_traces counts traces with any)
enum : uint32_t {
  SD_FRONT = 1u,          // pruned sweep of the voted strand not certified in either tier (pipeline.hip: swept in full)
  SD_STRAND = 2u,         // strand by certificate: the loser's bound does not decide (its full sweep is needed)
  SD_LOSER_WON = 4u,      // the strand the vote marked as the likely loser won: its row m was not kept
  SD_JUNK = 8u,           // c_e = 0: the all-gap path is optimal (or an empty pair)
  SD_PRELIM_BAND = 16u,   // preliminary alignment: its score allows a band wider than the band kernels hold
  SD_PRELIM_CHECK = 32u,  // ... or the banded result is not the sweep's (score differs, walk left the band)
  SD_FINAL_BAND = 64u,    // `tracy align`: final alignment outside the band kernels' shapes
  SD_FINAL_CHECK = 128u,  // ... or its band certificate failed
  SD_MEM = 256u,          // traceback words beyond the workspace planned for the launch
  SD_ALLELE_FRONT = 512u, // gotoh(allele, window): pruned sweep not eligible / not certified
  SD_ALLELE_ORIGIN = 1024u,  // its origin band too wide
  SD_ALLELE_BAND = 2048u,    // gotoh(allele, slice): band too wide / ends outside the slice
  SD_ALLELE_CHECK = 4096u,   // ... or the banded result is not S*
  SD_A12_BAND = 8192u,       // allele 1 vs allele 2: no band
  SD_A12_CHECK = 16384u,     // ... or its bound not beaten
  SD_SHAPE = 32768u,         // a sub-window longer than the launch's LDS staging was sized for
};

// counters the planning kernels keep (tracyhip_call_stats, kernel timers): one block of 64-bit words per call
enum : int {
  SC_PRUNED = 0, SC_PRUNED_UNCERT, SC_PRELIM_BANDED, SC_PRELIM_REPEATED, SC_FINAL_BANDED, SC_FINAL_REPEATED,
  SC_ALLELE_PRUNED0, SC_ALLELE_PRUNED1, SC_ALLELE_UNCERT0, SC_ALLELE_UNCERT1,
  SC_ALLELE_BANDED0, SC_ALLELE_BANDED1, SC_ALLELE_BANDED2, SC_ALLELE_REPEATED0, SC_ALLELE_REPEATED1, SC_ALLELE_REPEATED2,
  SC_SWEEP_CELLS, SC_SWEEP_BYTES,  // the combined sweep / prefix launches (TRACYHIP_TIMER_SCORE)
  SC_DECOMP_CELLS, SC_DECOMP_BYTES,
  SC_FRONT_CELLS, SC_FRONT_BYTES,  // the first tier of the pruned sweeps (TRACYHIP_TIMER_FRONT: strips of 8 rows on c* +- 60)
  SC_ALLELE_SHARED,                // allele 2 reading the prefix row allele 1 keeps (s_allele_plan0_kernel)
  SC_COUNT
};
// per band stage (bucket scan): cells and algorithmic bytes of the launch (kernel timers), bytes of its traceback words
// ... and how wide its bands were: pairs by diagonals (dmax - dmin + 1) <= 8, 16, 24, 32, 48, 64, 96, more (option `verbose` prints them)
// ... and the sizes of its four lists: strip height 12, 8, 4, the quad form (tracyhip_call_stats::band_list_pairs)
enum : int { SB_CELLS = 0, SB_BYTES = 1, SB_WORDS = 2, SB_HIST = 4, SB_HIST_N = 8, SB_LIST = 12, SB_LIST_N = 4, SB_COUNT = 16 };
TR_HD int s_width_bucket(int32_t dmin, int32_t dmax) {
  const int32_t w = dmax - dmin + 1;
  return w <= 8 ? 0 : w <= 16 ? 1 : w <= 24 ? 2 : w <= 32 ? 3 : w <= 48 ? 4 : w <= 64 ? 5 : w <= 96 ? 6 : 7;
}

enum : uint32_t { SG_FRONT_OK = 1u };

struct SGeom {          // one trace: what the host knows before anything runs
  uint64_t prof_off;    // full profile &P[0][0] (floats)
  uint64_t ref_off;     // reference window (bytes of the payload = codes of the code buffer)
  uint64_t lr_off[2];   // row m / kept row of the forward / reverse-complement sweep (int32 units)
  uint64_t tab_off;     // substitution table of the full profile (int16 units)
  uint64_t ops_off;     // `tracy align`: the final alignment's ops (tracyhip_align_result::ops_offset); `tracy decompose`: ops and rows of the trimmed trace
  uint32_t mf, mt, tl, rn;
  uint32_t tab_stride;
  uint32_t full_a, full_b;  // its two slots in the list of full sweeps (sorted by strip height, then size)
  uint32_t flags;       // SG_FRONT_OK
  uint32_t rl, rr;      // the trims the job REQUESTS for this trace (its per-trace arrays, else the scalar pair): what trimReferenceSlice
                        // (R9), trimmedSeq and the decompose stages take -- tl / mt above are createProfile's clamped view of them
};
struct SGeomD {         // `tracy decompose`: the rest
  uint64_t bc_off;      // basecalls (primary / secondary / secDecompose / bcPos)
  uint64_t sig_off;
  uint64_t dcp_off;
  uint64_t opsk_off[3];  // allele alignments (tracyhip_decompose_result::ops_offset[k])
  uint64_t atab_off[2];  // substitution tables of the allele strings (int16 units)
  uint64_t alr_off[2];   // kept rows of their prefix sweeps (int32 units)
  uint32_t nsamples, sl, soff, atab_stride;
  uint32_t flags[2];     // SG_FRONT_OK per allele
};

struct TrimRec {        // trimReferenceSlice's three numbers
  uint32_t ri;          // offset of the trimmed slice in the oriented reference
  uint32_t len;         // its length after std::string::substr clamping
  uint32_t pos;         // rs.pos after the update (rs.pos starts at 0)
  uint32_t pad;
};

struct STrace {         // one trace: what the stages leave for each other
  int32_t sc[2];        // gsFwd, gsRev (the loser's may be its certified bound)
  int32_t sstar;        // the winner's: score of the preliminary alignment
  uint32_t ce;          // where that alignment ends on row m (window column, 1-based)
  uint32_t gap;         // gap columns its score allows
  uint32_t shift;       // columns of the window left of the sub-window
  int32_t bw;           // `tracy align`: half width of the final alignment's band
  uint8_t g, cls, rc, fwd;
  uint32_t mark;        // ST_* (`tracy align`: the early tail)
  TrimRec trim;
};
// STrace::mark.  A trace is EARLY when its stages behind the orientation decision were queued for the voted strand before the other
// strand's exact score was there (s_orient_early_kernel); the decision then confirms it, or gives it the verdict SD_LOSER_WON.  The
// two COUNTED bits say which of the call's counters its early stages added to: a refuted trace takes them back.
enum : uint32_t { ST_EARLY = 1u, ST_COUNTED_PRELIM = 2u, ST_COUNTED_FINAL = 4u };
struct SAllele {        // one allele of one trace (`tracy decompose`)
  int32_t sstar;
  uint32_t ce;
  int64_t gap;
  uint32_t shift;
  uint32_t pad;
  TrimRec trim;
};

struct SParams {        // scoring + switches every planning kernel sees
  int32_t match, mismatch, go, ge;
  uint32_t nt;
  uint32_t exact;       // both orientation scores exact (no strand by certificate)
  uint32_t ncap;        // longest sub-window the band launches staged LDS for
  uint32_t use_votes;   // the full sweeps skip row m of the likely loser (DpArgs::votes)
  uint32_t split_prefix;  // the voted strands' prefixes run in a launch of their own beside the full sweeps (timed and credited with the pruned sweep)
};

TR_HD int64_t s_abs64(int32_t x) { return x < 0 ? -(int64_t)x : (int64_t)x; }
TR_HD int64_t s_best(const SParams& p) { const int64_t b = p.match > p.mismatch ? p.match : p.mismatch; return b > 0 ? b : 0; }

// R9. the widening / clamping / rs.pos part of trimReferenceSlice (fmindex.h:443-461)
TR_HD TrimRec s_trim_finish(uint32_t ri, uint32_t risize, uint32_t n, uint32_t trim_left, uint32_t trim_right, bool forward) {
  if (ri >= trim_left) { ri -= trim_left; risize += trim_left; }
  if ((uint32_t)(ri + risize + trim_right) < n) risize += trim_right;
  TrimRec r;
  r.ri = ri;
  r.len = (ri <= n) ? ((risize < n - ri) ? risize : n - ri) : 0;  // substr(ri, risize)
  r.pos = 0;
  if (forward) r.pos = ri;
  else {
    const int32_t offset = (int32_t)n - (int32_t)ri - (int32_t)risize;
    if (offset >= 0) r.pos = (uint32_t)offset;  // negative: the reference only warns (fmindex.h:457-459)
  }
  r.pad = 0;
  return r;
}

// value ranges of the origin-tracking sweep on the band kernels (b16_origin_ok) for m rows / n columns, in the domain they take
// (AlignConfig<true,false>)
TR_HD bool origin16_ok(const tracyhip_params* prm, uint32_t maxm, uint32_t maxn) {
  if (!prm->hfree || prm->vfree) return false;
  return b16_origin_ok(prm->match, prm->mismatch, prm->go, prm->ge, maxm, maxn);
}

// R2. a pruned sweep (front.h) of m rows against n columns is eligible: two strips of kFrontK rows below the prefix's kFrontRows, a
// column, and the value ranges of the origin-tracking sweep over the widest sub-window the placement can give it
TR_HD bool s_front_ok(const tracyhip_params* prm, uint32_t m, uint32_t n) {
  return m > kFrontRows + 2u * (uint32_t)kFrontK && n >= 1 && origin16_ok(prm, m, m - kFrontRows + 2u * (uint32_t)kFrontHalfW + 16u);
}

// R1. class of a trace from its k-mer votes vf / vr for the two strands.  g: the voted strand.  both: no clear majority of shared k-mers
// (or no rows below the prefix), both strands are swept.  cls 0: pruned sweep of g (front_ok: R2); 1: both strands in full (`exact`:
// both scores are needed exactly); 2: g in full + the prefix of the other (strand by certificate: R11).  The vote itself is R10
// (s_clear_vote, dp_lane.h).  What makes a trace eligible beside it differs on purpose and stays with the caller: here rows below the
// pruned sweep's prefix (m > kFrontRows); in pipeline.hip's orient_vote rows below the prefix of the batch's strip height (its elig[t]).
struct SOrient { uint32_t g, both, cls; };
TR_HD SOrient s_orient_class(uint32_t vf, uint32_t vr, uint32_t m, bool front_ok, bool exact) {
  const ClearVote v = s_clear_vote(vf, vr);
  SOrient o;
  o.g = v.g;
  o.both = (m > kFrontRows && v.clear) ? 0u : 1u;
  o.cls = (!o.both && front_ok) ? 0u : (exact || o.both) ? 1u : 2u;
  return o;
}

// R11. strand by certificate.  The voted strand g has its exact score S_g; the other strand has only the maximum of its prefix rows,
// and the rows below them add at most ub: its score is at most bound = prefix + ub.  The reference decides forward iff gsFwd > gsRev
// (sage.h:247), so a voted forward strand needs bound < S_g and a voted reverse strand bound <= S_g: the tie goes to reverse either way.
// A certified loser's score array holds the bound (at most INT32_MAX); without the certificate its full sweep is needed.
struct SStrand { bool certified; int32_t bound; };
TR_HD SStrand s_strand_by_bound(uint32_t g, int32_t prefix, int32_t ub, int64_t s_g) {
  const int64_t b = (int64_t)prefix + ub;
  return SStrand{g == 0u ? b < s_g : b <= s_g, (int32_t)(b < 0x7fffffffLL ? b : 0x7fffffffLL)};
}

// diagonals [dlo, dhi] of a band and the strip height that sweeps it (b16_pick_k; 0: too wide)
struct SBand { int32_t dlo, dhi; int K; };
// the band around an alignment that ends in column ce of row m with at most g gap steps: diagonals (ce - m) +- (g + 1)
TR_HD SBand s_end_band(uint32_t m, int64_t ce, int64_t g) {
  const int64_t gg = g < (1 << 20) ? g : (1 << 20);
  const int32_t d1 = (int32_t)ce - (int32_t)m;
  SBand b;
  b.dlo = d1 - (int32_t)gg - 1;
  b.dhi = d1 + (int32_t)gg + 1;
  b.K = b16_pick_k(b.dlo, b.dhi);
  return b;
}

// R3. A path that ends at (m, c_e) with score S* and can collect at most `top` on its diagonal steps has at most g = (top - S*) / |ge|
// gap columns: it lies in the columns (a, c_e], a = c_e - m - g - 2, on the band s_end_band(m, n', g) of that sub-window of
// n' = c_e - a columns (preliminary alignment of `tracy align`, gotoh(allele, window) of `tracy decompose`).
struct SubWindow { int64_t g; uint32_t a, n; int32_t dlo, dhi; int K; };
TR_HD SubWindow s_sub_window(uint32_t m, uint32_t ce, int64_t top, int64_t sstar, int32_t ge) {
  SubWindow s;
  const int64_t age = -(int64_t)ge, loss = top - sstar;
  s.g = loss > 0 ? loss / age : 0;
  int64_t a = (int64_t)ce - (int64_t)m - s.g - 2;
  if (a < 0) a = 0;
  s.a = (uint32_t)a;
  s.n = (uint32_t)((int64_t)ce - a);
  const SBand b = s_end_band(m, s.n, s.g);
  s.dlo = b.dlo;
  s.dhi = b.dhi;
  s.K = b.K;
  return s;
}
// R4. LDS of a band launch, asked of one pair of n columns: the launches' rule (launch_rules.h) at the planners' limit
TR_HD bool s_fits_lds(uint32_t n, int K) { return band_lds_fits(band_code_cap(n), K, kBandLdsPlan); }

// R5. `tracy align`, final alignment gotoh(full profile, trimmed slice) of m x n on a band of half width w: the gap columns the
// preliminary alignment's score allowed + 48 for what the trimmed ends add, within [32, 96] ...
TR_HD int64_t s_final_width(uint32_t gap) {
  const int64_t w = (int64_t)gap + 48;
  return w < 32 ? 32 : w > 96 ? 96 : w;
}
// ... or the width the caller wants (host planner: option band_w), narrowed to what one period of the K = 12 strips holds when that
// leaves at least 24; diagonals [-w - (m-n)+, w + (n-m)+].  K = 0: no band (an empty pair, a slice past the LDS limit, too wide)
struct SFinalBand { int64_t w; int32_t dlo, dhi; int K; };
TR_HD SFinalBand s_final_band(uint32_t m, uint32_t n, int64_t want) {
  SFinalBand f{0, 0, 0, 0};
  if (!(m && n && s_fits_lds(n, 12))) return f;
  const int64_t over = (int64_t)n - (int64_t)m, aover = over < 0 ? -over : over;
  const int64_t fit = ((int64_t)b16_max_window(12) - 12 - aover) / 2;  // the widest band the kernels sweep
  f.w = want > fit && fit >= 24 ? fit : want;
  f.dlo = (int32_t)(-f.w - (over < 0 ? -over : 0));
  f.dhi = (int32_t)(f.w + (over > 0 ? over : 0));
  f.K = b16_pick_k(f.dlo, f.dhi);
  return f;
}
// R6. its certificate: a path that leaves the band makes more than w interior gap steps and scores at most top - |ge| (w + 1); a banded
// score S_b above that (and a walk that stayed inside: ops_len != 0) is the optimum
TR_HD bool s_final_certified(int32_t sb, int32_t top, int32_t ge, int64_t w, uint32_t ops_len) {
  return (int64_t)sb > (int64_t)top - (-(int64_t)ge) * (w + 1) && ops_len != 0u;
}

// R7. gotoh(allele, trimmed slice) of m x n: the alignment ends in slice column ce of row m with at most g gap steps (g < 0: not
// known), on the diagonals s_end_band(m, ce, g).  narrow (stream.hip, unless option no_origin_band): the origin sweep followed the
// very path the traceback will walk (the same predecessor at every maximum); it starts at row 0 in column `lead` of the window, i.e.
// on diagonal d0 = lead - ri of the slice (ri: where the slice begins; lead < ri: unknown), and ends on d1.  With v vertical and h
// horizontal gap steps, h - v = d1 - d0 and h + v <= g, so the path stays on [min(d0, d1) - s, max(d0, d1) + s], s = (g - |d1 - d0|) / 2
// -- and a band that holds THIS path reproduces its walk: every cell of the path keeps its value (its own prefix is inside), every
// other value is a lower bound, so whatever lost a comparison in the full matrix loses it in the band, and what won or tied with
// preference is on the path.  (The other co-optimal paths, which d1 +- g would hold as well, are never walked.)  g + 3 diagonals
// instead of 2 g + 3.  The host planner does not narrow.
TR_HD SBand s_slice_band(uint32_t m, uint32_t n, int64_t ce, int64_t g, bool narrow, uint32_t lead, uint32_t ri) {
  SBand b{0, 0, 0};
  if (!(g >= 0 && m && n && ce >= 1 && ce <= (int64_t)n)) return b;
  b = s_end_band(m, ce, g);
  if (narrow && lead >= ri) {
    const int64_t gg = g < (1 << 20) ? g : (1 << 20);
    const int32_t d0 = (int32_t)(lead - ri), d1 = (int32_t)ce - (int32_t)m;
    const int64_t delta = d1 > d0 ? (int64_t)d1 - d0 : (int64_t)d0 - d1;
    if (delta <= gg) {
      const int32_t sdev = (int32_t)((gg - delta) / 2);
      b.dlo = (d0 < d1 ? d0 : d1) - sdev - 1;
      b.dhi = (d0 < d1 ? d1 : d0) + sdev + 1;
      b.K = b16_pick_k(b.dlo, b.dhi);
    }
  }
  return b;
}

// R8. allele 1 vs allele 2, global (indigo.h:379-387), both of `len` bases (the trimmed trace).  W is guessed from what the two alleles
// lost against the reference (scores sc1, sc2; they differ from each other by about as much as both differ from it), at most 90.  Both
// ends are fixed: a path that leaves the diagonals [-W, W] makes at least W + 1 vertical and W + 1 horizontal gap steps in two runs,
// so it scores at most `bound` = best (len - W - 1) - |ge| 2 (W + 1) - 2 |go|; a banded score above that is the optimum.  (For
// alleles of different lengths the band and the bound would widen by (m - n)+ / (n - m)+; here they are always the same length.)
struct SA12Band { int32_t dlo, dhi; int K; int64_t bound; };
TR_HD SA12Band s_a12_band(uint32_t len, int64_t best, int32_t go, int32_t ge, int32_t sc1, int32_t sc2) {
  SA12Band r{0, 0, 0, 0};
  if (len == 0) return r;
  const int64_t age = -(int64_t)ge, ago = -(int64_t)go;
  const int64_t l0 = best * len - sc1, l1 = best * len - sc2;
  const int64_t lost = (l0 > 0 ? l0 : 0) + (l1 > 0 ? l1 : 0);
  const int64_t per = best + 2 * age;
  int64_t W = (5 * lost / 2 + 40) / (per > 0 ? per : 1) + 2;
  if (W > 90) W = 90;
  r.dlo = (int32_t)-W;
  r.dhi = (int32_t)W;
  r.K = b16_pick_k(r.dlo, r.dhi);
  r.bound = best * ((int64_t)len - (W + 1)) - age * 2 * (W + 1) - 2 * ago;
  return r;
}

// R12. certificate of a banded traceback whose exact score S* is known beforehand: the sub-window (preliminary alignment) or the
// trimmed slice (gotoh(allele, slice)) holds the alignment just located, so its score is S* again -- a banded score is never above
// the optimum, and one that reaches it is it.  A banded walk that left its band reports no ops.
TR_HD bool s_exact_certified(int32_t sb, int32_t sstar, uint32_t ops_len) { return sb == sstar && ops_len != 0u; }
// R13. certificate of allele 1 vs allele 2: the banded score beats the bound of s_a12_band (R8) -- what any path that leaves the band
// scores at most -- and the walk stayed inside (ops_len != 0)
TR_HD bool s_a12_certified(int64_t sb, int64_t bound, uint32_t ops_len) { return sb > bound && ops_len != 0u; }

TR_HD PairDesc s_skip_pair(uint32_t out) {
  PairDesc d{};
  d.flags = PAIR_SKIP;
  d.out = out;
  return d;
}

}  // namespace tracyhip
#endif
