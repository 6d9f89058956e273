// seed.hip -- tracyhip_genome_upload / tracyhip_seed_traces: k-mer seeding of a batch of traces in an indexed genome on the device
// (getReferenceSlice, fmindex.h:236-326), bit-identical to the host's one-pass form (tracy_amd/host/seed.hpp scanBothStrands +
// getReferenceSlice) for every trace it answers; the rest is DEFERRED to the host.  tracyhip_genome_build: the same handle with the
// table built on the device from the text (index_build.hip).
//
// One workgroup of 256 threads per trace.  A look-up is two dependent random reads into a gigabyte of directory + table; the
// look-ups of a trace are independent, so every lane takes four windows at once: their keys, then their four directory loads,
// then their four first table lines -- ~1000 look-ups of a trace in flight at the same time instead of a core's ~20.  Votes go
// to two lists in LDS (one per strand, appended by an LDS atomic); findMaxFreq sorts each list (bitonic, both lists in the
// same steps) and finds the longest run by bisection from every run start.  The window is copied (and complemented) byte by
// byte by the whole workgroup.
//
// Option seed_spill: a trace with more votes than the lists hold (a read inside a gene family or repeat, a read of more than
// ~2 100 windows) is not deferred but reports the pass it overflowed in and the exact vote counts of everything it can still need;
// seed_spill_kernel, launched over those traces after the chunk's synchronisation, repeats the sweep from that pass with every vote
// counted in a per-strand hash table in device memory (seed.h) and ends like the first kernel.  One copy of the sweep (seed_sweep,
// parameterised by what happens to a vote), of the fold over the workgroup, of the anchoring rule and of the end (seed_finish).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/tracy_hip.h"
#include "capi_internal.h"
#include "index_build.h"
#include "seed.h"

using namespace tracyhip;

struct tracyhip_genome {
  int device = 0;
  uint32_t k = 0, bucket_bits = 0, nc = 0;
  uint64_t ntab = 0, text_len = 0, bytes = 0;
  std::vector<void*> mem;
  SeedGenome g{};
};

namespace {

struct SeedArgs {
  SeedGenome g;
  const uint8_t* cons;   // consensus bytes; trace i at cons + off[i], len[i] bytes
  const uint64_t* off;
  const uint32_t* len;
  SeedOut* out;          // [n]
  uint8_t* slices;       // trace i's window at slices + i * slice_cap
  uint64_t slice_cap;
  uint32_t n, P, cap;    // P: LDS list capacity per strand (power of two >= cap)
  const uint32_t* trims;  // [n] each trace's own trims, left in the low and right in the high 16 bits (a scalar call: its pair n times)
  uint32_t kmer, min_support, maxindel;  // (16-bit values)
  uint32_t spill;        // option seed_spill: a trace with more votes than the lists hold reports kSeedSpill instead of DEFERRED
};

// one trace of a spill launch: what the first kernel reported of it, and where its two tables lie
struct SeedSpillDesc {
  uint32_t trace;        // its index in the chunk
  uint32_t pass;         // the pass to start at
  uint32_t votes[2][2];  // [pass][strand]: a pass's table takes seed_table_capacity(votes) slots
  uint64_t tab[2];       // first slot of the strand's table in SeedSpillArgs::slots (room for the larger of its passes)
};
struct SeedSpillArgs {
  const SeedSpillDesc* desc;  // one per workgroup
  SeedSlot* slots;
};

__device__ __forceinline__ void write_status(const SeedArgs& a, uint32_t t, int32_t st) {
  a.out[t].status = st;
  a.out[t].slice_len = 0;
}

// a trace's windows: consensus, lengths and the strand rules of scanBothStrands
struct SeedTrace {
  const uint8_t* c;
  uint32_t S, k, p_lo, p_hi, nwin, fwd_from, rev_until;
  uint64_t mask, bmask;
};
// The domain of scanBothStrands (seed.hpp:614-619) for trace t: -1 and `tr` filled, or the status of a trace without a sweep --
// DEFERRED outside the domain (the host runs its two scans), UNANCHORED without a window.
__device__ __forceinline__ int32_t seed_trace(const SeedArgs& a, uint32_t t, SeedTrace& tr) {
  const uint32_t S = a.len[t];
  const uint32_t trims = a.trims[t];  // (indexed by the block: a scalar load)
  const uint32_t k = a.kmer, TL = trims & 0xffffu, TR = trims >> 16;
  if (k != a.g.k || k < 1 || k > 32 || (uint64_t)S + k >= 65536u || TL + 1 < k || TR + 1 < k || S < TL || S < TR) return TRACYHIP_SEED_DEFERRED;
  if (S <= TL + TR) return TRACYHIP_SEED_UNANCHORED;  // no window on either strand: zero votes in both passes
  tr.c = a.cons + a.off[t];
  tr.S = S;
  tr.k = k;
  tr.p_lo = TL + 1 - k;
  tr.p_hi = S - TR;
  tr.nwin = tr.p_hi - tr.p_lo;
  tr.fwd_from = k - 1;
  tr.rev_until = tr.nwin >= k ? tr.nwin - k + 1 : 0;
  tr.mask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
  tr.bmask = (1ull << a.g.bucket_bits) - 1ull;
  return -1;
}

// What happens to the votes of one window and strand -- the `occs` table entries from qlo on, each voting its position - at:
// appended to the strand's list in LDS and counted past its end (n[] is then the exact size of the pass);
struct SeedListSink {
  int64_t* l[2];
  uint32_t* n;
  uint32_t P;
  __device__ __forceinline__ void votes(int strand, const uint64_t* tab, uint64_t qlo, uint64_t occs, int64_t at) const {
    const uint32_t slot = atomicAdd(&n[strand], (uint32_t)occs);
    for (uint64_t q = 0; q < occs; ++q)
      if (slot + q < P) l[strand][slot + q] = (int64_t)(tab[2 * (qlo + q) + 1] & ~kSeedFlipped) - at;
  }
};
// counted only, which is a list of capacity 0; or inserted into the strand's counting table in device memory (seed.h) through the
// device's atomics: relaxed, device scope, so every access of a slot is served by the L2 and none by a CU's cache
struct SeedMemDevice {
  template <class T>
  static __device__ __forceinline__ T load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  template <class T>
  static __device__ __forceinline__ void store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ int64_t claim(int64_t* p, int64_t expected, int64_t v) {
    return (int64_t)atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expected, (unsigned long long)v);
  }
  static __device__ __forceinline__ void add(uint32_t* p, uint32_t n) { atomicAdd(p, n); }
};
struct SeedTableSink {
  SeedSlot* tab[2];
  uint64_t cap[2];
  uint32_t* lost;  // set where a vote found no slot (a table smaller than its votes: the trace is then DEFERRED, not answered wrongly)
  __device__ __forceinline__ void votes(int strand, const uint64_t* tab_, uint64_t qlo, uint64_t occs, int64_t at) const {
    SeedSlot* const mine = strand == 0 ? tab[0] : tab[1];  // (selected, not indexed: the sink stays in registers)
    const uint64_t slots = strand == 0 ? cap[0] : cap[1];
    for (uint64_t q = 0; q < occs; ++q)
      if (!seed_table_insert<SeedMemDevice>(mine, slots, (int64_t)(tab_[2 * (qlo + q) + 1] & ~kSeedFlipped) - at)) *lost = 1u;
  }
};

// The look-up sweep of one pass over a trace's windows by the whole workgroup: every window's key, its run in the table, and per
// strand the votes the pass's rule admits (unique: k-mers with one occurrence; else: with fewer than 1000), handed to `sink`.
template <class Sink>
__device__ __forceinline__ void seed_sweep(const SeedGenome& g, const SeedTrace& tr, bool unique, const Sink& sink) {
  const uint32_t tid = threadIdx.x;
  const uint8_t* c = tr.c;
  const uint32_t S = tr.S, k = tr.k, p_lo = tr.p_lo, nwin = tr.nwin, fwd_from = tr.fwd_from, rev_until = tr.rev_until;
  const uint64_t mask = tr.mask, bmask = tr.bmask;
  for (uint32_t base = 0; base < nwin; base += kSeedThreads * kSeedWin) {
    uint64_t key[kSeedWin];
    uint32_t info[kSeedWin];  // bit 0: a look-up (no N), bit 1: the forward k-mer is the run's flipped part, bit 2: palindrome
    uint64_t lo[kSeedWin], hi[kSeedWin];
#pragma unroll
    for (uint32_t j = 0; j < kSeedWin; ++j) {
      const uint32_t w = base + j * kSeedThreads + tid;
      info[j] = 0;
      key[j] = 0;
      if (w < nwin) {
        uint64_t fw = 0;
        bool ok = true;
        for (uint32_t q = 0; q < k; ++q) {
          const uint32_t b = seed_letter(c[p_lo + w + q]);
          ok = ok && b < 4;
          fw = ((fw << 2) | (b & 3u)) & mask;
        }
        if (ok) {
          const uint64_t rc = seed_revcomp(fw, k);
          key[j] = rc < fw ? rc : fw;
          info[j] = 1u | (rc < fw ? 2u : 0u) | (rc == fw ? 4u : 0u);
        }
      }
    }
    // the directory slots of all four windows, then their buckets (every index clamped to the table)
#pragma unroll
    for (uint32_t j = 0; j < kSeedWin; ++j) {
      lo[j] = hi[j] = 0;
      if (info[j]) {
        const uint64_t b = key[j] & bmask;
        lo[j] = g.dir[b];
        hi[j] = g.dir[b + 1];
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < kSeedWin; ++j) {
      if (!info[j]) continue;
      const uint64_t e = hi[j] < g.ntab ? hi[j] : g.ntab;
      uint64_t i = lo[j] < e ? lo[j] : e;
      const uint64_t kk = key[j];
      while (i < e && g.tab[2 * i] < kk) ++i;
      const uint64_t own = i;  // [own, mid): the run's own code, [mid, end): its reverse complement's
      while (i < e && g.tab[2 * i] == kk && !(g.tab[2 * i + 1] & kSeedFlipped)) ++i;
      const uint64_t mid = i;
      while (i < e && g.tab[2 * i] == kk) ++i;
      const uint64_t end = i;
      const bool flipped = (info[j] & 2u) != 0, pal = (info[j] & 4u) != 0;
      const uint64_t f_lo = flipped ? mid : own, f_hi = flipped ? end : mid;
      const uint64_t r_lo = pal ? f_lo : (flipped ? own : mid), r_hi = pal ? f_hi : (flipped ? mid : end);
      const uint32_t w = base + j * kSeedThreads + tid;
      const int64_t p = (int64_t)(p_lo + w);
      for (int strand = 0; strand < 2; ++strand) {
        if (strand == 0 ? w < fwd_from : w >= rev_until) continue;
        const uint64_t qlo = strand == 0 ? f_lo : r_lo, qhi = strand == 0 ? f_hi : r_hi;
        const uint64_t occs = qhi - qlo;
        if (!(unique ? occs == 1 : (occs > 0 && occs < 1000))) continue;
        const int64_t at = strand == 0 ? p : (int64_t)S - p - (int64_t)k;
        sink.votes(strand, g.tab, qlo, occs, at);
      }
    }
  }
}

// every lane's best (length, value) per strand folded over the workgroup: all lanes leave with the same freq[] / best[]
__device__ __forceinline__ void seed_fold_best(uint32_t bl[2], int64_t bv[2], uint32_t freq[2], int64_t best[2]) {
  __shared__ uint32_t s_len[2][kSeedThreads / 64];
  __shared__ int64_t s_val[2][kSeedThreads / 64];
  const uint32_t tid = threadIdx.x;
  for (int s = 0; s < 2; ++s)
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t ol = __shfl_xor(bl[s], d);
      const int64_t ov = __shfl_xor(bv[s], d);
      seed_better(bl[s], bv[s], ol, ov);
    }
  if ((tid & 63) == 0) {
    for (int s = 0; s < 2; ++s) { s_len[s][tid >> 6] = bl[s]; s_val[s][tid >> 6] = bv[s]; }
  }
  __syncthreads();
  for (int s = 0; s < 2; ++s) {
    freq[s] = 0;
    best[s] = 0;
    for (uint32_t w = 0; w < kSeedThreads / 64; ++w) seed_better(freq[s], best[s], s_len[s][w], s_val[s][w]);
  }
  __syncthreads();  // (the next pass rewrites s_len / s_val, and what the votes were counted in)
}

// the anchoring rule of getReferenceSlice over the two strands' best counts ([0] forward, [1] reverse)
__device__ __forceinline__ bool seed_anchors(const uint32_t freq[2], uint32_t min_support, bool& fwd) {
  if (freq[0] >= min_support && freq[0] > 2 * freq[1]) { fwd = true; return true; }
  if (freq[1] >= min_support && freq[1] > 2 * freq[0]) { fwd = false; return true; }
  return false;
}

// The end of a trace whose passes are done, by the whole workgroup: UNANCHORED, or the result record and the oriented window.
__device__ __forceinline__ void seed_finish(const SeedArgs& a, uint32_t t, uint32_t S, bool anchored, bool fwd, uint32_t support, int64_t bestPos) {
  __shared__ uint64_t s_src, s_wlen;
  const uint32_t tid = threadIdx.x;
  if (!anchored) {
    if (tid == 0) write_status(a, t, TRACYHIP_SEED_UNANCHORED);
    return;
  }
  if (tid == 0) {
    const SeedWindow win = seed_window(a.g.cum, a.g.starts, a.g.lengths, a.g.nc, a.g.text_len, bestPos, S, (uint16_t)a.maxindel);
    const uint64_t n = win.len < a.slice_cap ? win.len : a.slice_cap;
    s_src = win.src;
    s_wlen = win.len;
    SeedOut o;
    o.status = TRACYHIP_SEED_ANCHORED;
    o.forward = fwd ? 1u : 0u;
    o.kmersupport = support;
    o.pos = win.pos;
    o.contig = a.g.contig_id[win.ref];
    o.slice_len = (uint32_t)n;
    a.out[t] = o;
  }
  __syncthreads();
  // the oriented window: reverseComplement of the whole slice (a letter outside ACGTNacgtn keeps the output position's ORIGINAL
  // byte), of which the first slice_cap bytes are kept
  const uint64_t L = s_wlen, n = L < a.slice_cap ? L : a.slice_cap;
  const uint8_t* src = a.g.text + s_src;
  uint8_t* dst = a.slices + (uint64_t)t * a.slice_cap;
  if (fwd) {
    for (uint64_t i = tid; i < n; i += kSeedThreads) dst[i] = src[i];
  } else {
    for (uint64_t i = tid; i < n; i += kSeedThreads) {
      const uint8_t cc = seed_complement(src[L - 1 - i]);
      dst[i] = cc ? cc : src[i];
    }
  }
}

__global__ __launch_bounds__(kSeedThreads) void seed_traces_kernel(SeedArgs a) {
  extern __shared__ int64_t lists[];  // [2][P]: forward votes, reverse votes
  __shared__ uint32_t s_n[2];
  __shared__ uint32_t s_bad;
  const uint32_t t = blockIdx.x, tid = threadIdx.x;
  SeedTrace tr;
  const int32_t early = seed_trace(a, t, tr);
  if (early >= 0) {
    if (tid == 0) write_status(a, t, early);
    return;
  }
  if (tid == 0) s_bad = 0;
  __syncthreads();
  // letters among the windows: A C G T N only (anything else: the host's two scans, seed.hpp:636)
  {
    uint32_t bad = 0;
    for (uint32_t q = tr.p_lo + tid; q < tr.p_hi - 1 + tr.k; q += kSeedThreads) bad |= seed_letter(tr.c[q]) == 5 ? 1u : 0u;
    if (bad) atomicOr(&s_bad, 1u);
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) write_status(a, t, TRACYHIP_SEED_DEFERRED);
    return;
  }
  int64_t* const lf = lists;
  int64_t* const lr = lists + a.P;
  SeedListSink sink{{lf, lr}, s_n, a.P};
  uint32_t freq[2] = {0, 0};
  int64_t best[2] = {0, 0};
  bool anchored = false, fwd = false;
  // seed_spill, an overflow in the unique pass: that pass's votes, kept while the second pass's are counted
  bool counting = false;
  uint32_t n0F = 0, n0R = 0;
  for (int pass = 0; pass < 2 && !anchored; ++pass) {
    if (tid == 0) { s_n[0] = 0; s_n[1] = 0; }
    __syncthreads();
    seed_sweep(a.g, tr, pass == 0, sink);
    __syncthreads();
    const uint32_t nF = s_n[0], nR = s_n[1];
    if (counting || nF > a.cap || nR > a.cap) {  // more votes than the lists hold: the spill kernel's trace, or the host's
      if (!a.spill) {
        if (tid == 0) write_status(a, t, TRACYHIP_SEED_DEFERRED);
        return;
      }
      // The trace reports the pass and its exact vote counts.  An overflow in the unique pass cannot know whether that pass
      // anchors: the second pass runs as a count (lists of no capacity keep nothing), and the host sizes everything the trace
      // can still need.
      if (pass == 0) {
        counting = true;
        n0F = nF;
        n0R = nR;
        sink.P = 0;
        __syncthreads();  // (every lane has read s_n, which the next pass clears)
        continue;
      }
      if (tid == 0) {
        const SeedSpillOut so{kSeedSpill, counting ? 0u : 1u, {{n0F, n0R}, {nF, nR}}};
        *reinterpret_cast<SeedSpillOut*>(&a.out[t]) = so;
      }
      return;
    }
    // findMaxFreq of both lists (fmindex.h:173-198): sorted ...
    uint32_t P2 = 2;
    while (P2 < nF || P2 < nR) P2 <<= 1;
    for (uint32_t i = tid; i < P2; i += kSeedThreads) {
      if (i >= nF) lf[i] = INT64_MAX;
      if (i >= nR) lr[i] = INT64_MAX;
    }
    __syncthreads();
    const uint32_t half = P2 >> 1;
    for (uint32_t size = 2; size <= P2; size <<= 1) {
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        for (uint32_t x = tid; x < P2; x += kSeedThreads) {  // x < half: a pair of the forward list, else of the reverse one
          int64_t* l = x < half ? lf : lr;
          const uint32_t j = x < half ? x : x - half;
          const uint32_t i = 2 * stride * (j / stride) + (j % stride);
          const bool up = (i & size) == 0;
          const int64_t u = l[i], v = l[i + stride];
          if ((u > v) == up) { l[i] = v; l[i + stride] = u; }
        }
        __syncthreads();
      }
    }
    // ... the longest run (the smallest value among the longest): from every run start, its end by bisection
    uint32_t bl[2] = {0, 0};
    int64_t bv[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
      const int64_t* l = s == 0 ? lf : lr;
      const uint32_t n = s == 0 ? nF : nR;
      for (uint32_t i = tid; i < n; i += kSeedThreads) {
        const int64_t v = l[i];
        if (i > 0 && l[i - 1] == v) continue;
        uint32_t lo2 = i + 1, hi2 = n;  // first index past the run
        while (lo2 < hi2) {
          const uint32_t m = (lo2 + hi2) >> 1;
          if (l[m] == v) lo2 = m + 1;
          else hi2 = m;
        }
        seed_better(bl[s], bv[s], lo2 - i, v);
      }
    }
    seed_fold_best(bl, bv, freq, best);  // (ends on a barrier: the lists and s_n are rewritten by the next pass)
    anchored = seed_anchors(freq, a.min_support, fwd);
  }
  seed_finish(a, t, tr.S, anchored, fwd, freq[fwd ? 0 : 1], best[fwd ? 0 : 1]);
}

// A trace whose votes did not fit the first kernel's lists, from the pass it reported on: the same sweep with every vote counted in
// the strand's table in device memory, findMaxFreq as a scan of the table, the same anchoring rule and end.
__global__ __launch_bounds__(kSeedThreads) void seed_spill_kernel(SeedArgs a, SeedSpillArgs sp) {
  __shared__ uint32_t s_lost;
  const SeedSpillDesc* const d = sp.desc + blockIdx.x;  // (read where it lies: uniform loads, no private copy to index)
  const uint32_t t = d->trace, tid = threadIdx.x;
  SeedTrace tr;
  if (seed_trace(a, t, tr) >= 0) return;  // (not a trace the first kernel swept: its record stays as it is)
  if (tid == 0) s_lost = 0;
  SeedTableSink sink{{sp.slots + d->tab[0], sp.slots + d->tab[1]}, {0, 0}, &s_lost};
  uint32_t freq[2] = {0, 0};
  int64_t best[2] = {0, 0};
  bool anchored = false, fwd = false;
  for (uint32_t pass = d->pass; pass < 2 && !anchored; ++pass) {
    for (int s = 0; s < 2; ++s) {
      sink.cap[s] = seed_table_capacity(d->votes[pass][s]);
      seed_table_clear<SeedMemDevice>(sink.tab[s], sink.cap[s], tid, kSeedThreads);
    }
    __syncthreads();
    seed_sweep(a.g, tr, pass == 0, sink);
    __syncthreads();
    uint32_t bl[2] = {0, 0};
    int64_t bv[2] = {0, 0};
    for (int s = 0; s < 2; ++s) seed_table_best<SeedMemDevice>(sink.tab[s], sink.cap[s], tid, kSeedThreads, bl[s], bv[s]);
    seed_fold_best(bl, bv, freq, best);
    anchored = seed_anchors(freq, a.min_support, fwd);
  }
  if (s_lost) {
    if (tid == 0) write_status(a, t, TRACYHIP_SEED_DEFERRED);
    return;
  }
  seed_finish(a, t, tr.S, anchored, fwd, freq[fwd ? 0 : 1], best[fwd ? 0 : 1]);
}

// what the tables of one spill launch may take where the budget allows more: enough for every workgroup a device holds at a time
constexpr uint64_t kSeedSpillLaunchBytes = 4ull << 30;

// The traces of a chunk that the first kernel left as kSeedSpill (res: its records, read back; a: its launch).  Their tables are
// laid out behind their descriptors in DB_SEED_SPILL, within the workspace budget; the spill kernel clears a table before the pass
// that counts in it.  Per sub-chunk: one launch, the records of its span of traces read back into res (for a host caller its span
// of windows too, into host_slices: the chunk's rows of the caller's array), one synchronisation.  A trace whose tables alone
// exceed the budget becomes DEFERRED.  Without a spilled trace nothing is launched or waited for.
int seed_spilled_traces(tracyhip_ctx* ctx, const SeedArgs& a, std::vector<SeedOut>& res, uint8_t* host_slices) {
  std::vector<SeedSpillDesc> desc;  // in trace order; tab[] relative to the trace's first slot until its sub-chunk is laid out
  std::vector<uint64_t> width;      // slots of both tables of desc[j]
  for (uint32_t i = 0; i < a.n; ++i) {
    if (res[i].status != kSeedSpill) continue;
    SeedSpillOut so;
    std::memcpy(&so, &res[i], sizeof(so));
    SeedSpillDesc d{};
    d.trace = i;
    d.pass = so.pass < 2 ? so.pass : 1;
    std::memcpy(d.votes, so.votes, sizeof(d.votes));
    uint64_t need[2];
    for (int s = 0; s < 2; ++s) need[s] = seed_table_capacity(d.pass == 0 ? std::max(d.votes[0][s], d.votes[1][s]) : d.votes[1][s]);
    d.tab[0] = 0;
    d.tab[1] = need[0];
    desc.push_back(d);
    width.push_back(need[0] + need[1]);
  }
  if (desc.empty()) return TRACYHIP_OK;
  uint64_t budget = 0;
  const int rc = workspace_budget(ctx, ctx->dev[DB_SEED_SPILL].cap, &budget);
  if (rc != TRACYHIP_OK) return rc;
  const uint64_t launch_bytes = std::min(budget, kSeedSpillLaunchBytes);
  for (size_t lo = 0; lo < desc.size();) {
    // [lo, hi): the traces of one launch; a trace larger than a launch's share runs alone, within the budget
    size_t hi = lo;
    uint64_t nslots = 0;
    auto bytes = [&](size_t count, uint64_t slots) { return ((sizeof(SeedSpillDesc) * count + 15) & ~(size_t)15) + sizeof(SeedSlot) * slots; };
    while (hi < desc.size() && bytes(hi + 1 - lo, nslots + width[hi]) <= (hi == lo ? budget : launch_bytes)) nslots += width[hi++];
    if (hi == lo) {
      ctx->stats.seed_spill_deferred += 1;
      ++lo;
      continue;
    }
    uint64_t at = 0;
    for (size_t j = lo; j < hi; ++j) {
      desc[j].tab[1] += at;
      desc[j].tab[0] = at;
      at += width[j];
    }
    uint8_t* d0;
    HIP_TRY(ensure_into(ctx->dev[DB_SEED_SPILL], bytes(hi - lo, nslots), d0));
    HIP_TRY(hipMemcpyAsync(d0, desc.data() + lo, sizeof(SeedSpillDesc) * (hi - lo), hipMemcpyHostToDevice, ctx->stream));
    const SeedSpillArgs sp{reinterpret_cast<const SeedSpillDesc*>(d0), reinterpret_cast<SeedSlot*>(d0 + bytes(hi - lo, 0))};
    hipLaunchKernelGGL(seed_spill_kernel, dim3((uint32_t)(hi - lo)), dim3(kSeedThreads), 0, ctx->stream, a, sp);
    HIP_TRY(hipGetLastError());
    const uint32_t first = desc[lo].trace, count = desc[hi - 1].trace - first + 1;
    HIP_TRY(hipMemcpyAsync(res.data() + first, a.out + first, sizeof(SeedOut) * count, hipMemcpyDeviceToHost, ctx->stream));
    if (host_slices && a.slice_cap)
      HIP_TRY(hipMemcpyAsync(host_slices + (uint64_t)first * a.slice_cap, a.slices + (uint64_t)first * a.slice_cap, (uint64_t)count * a.slice_cap,
                             hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx_sync(ctx));
    ctx->stats.seed_spill_launches += 1;
    for (size_t j = lo; j < hi; ++j) {
      const int32_t st = res[desc[j].trace].status;
      if (st == TRACYHIP_SEED_ANCHORED || st == TRACYHIP_SEED_UNANCHORED) ctx->stats.seed_spilled += 1;
    }
    lo = hi;
  }
  for (const SeedSpillDesc& d : desc)  // what no launch answered: the host's
    if (res[d.trace].status == kSeedSpill) { res[d.trace].status = TRACYHIP_SEED_DEFERRED; res[d.trace].slice_len = 0; }
  return TRACYHIP_OK;
}

template <class T>
hipError_t upload(tracyhip_genome* h, const T* src, uint64_t count, const T** dst) {
  *dst = nullptr;
  const uint64_t bytes = std::max<uint64_t>(count, 1) * sizeof(T);
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return e;
  h->mem.push_back(p);
  h->bytes += bytes;
  if (count) e = hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
  *dst = static_cast<const T*>(p);
  return e;
}

// the text and contig table of a descriptor, plus the cumulative length + 1 offsets and the contig_id map (identity when NULL)
hipError_t upload_text(tracyhip_genome* h, const tracyhip_genome_desc* d, const uint8_t** text) {
  std::vector<int64_t> cum(d->ncontigs, 0);
  for (uint32_t i = 1; i < d->ncontigs; ++i) cum[i] = cum[i - 1] + (int64_t)d->lengths[i - 1] + 1;
  std::vector<uint32_t> cid(d->ncontigs);
  for (uint32_t i = 0; i < d->ncontigs; ++i) cid[i] = d->contig_id ? d->contig_id[i] : i;
  SeedGenome& g = h->g;
  hipError_t e = upload(h, reinterpret_cast<const uint8_t*>(d->text), d->text_len, text);
  if (e == hipSuccess) e = upload(h, cum.data(), cum.size(), &g.cum);
  if (e == hipSuccess) e = upload(h, d->starts, d->ncontigs, &g.starts);
  if (e == hipSuccess) e = upload(h, d->lengths, d->ncontigs, &g.lengths);
  if (e == hipSuccess) e = upload(h, cid.data(), cid.size(), &g.contig_id);
  return e;
}

}  // namespace

extern "C" {

int tracyhip_genome_validate(const tracyhip_genome_desc* desc) {
  char why[256];
  const int rc = seed_validate(desc, why, sizeof(why));
  return rc == TRACYHIP_OK ? rc : set_error(rc, "tracyhip_genome: %s", why);
}

int tracyhip_genome_free(tracyhip_genome* h) {
  if (!h) return TRACYHIP_OK;
  (void)hipSetDevice(h->device);
  for (void* p : h->mem) (void)hipFree(p);
  delete h;
  return TRACYHIP_OK;
}

uint64_t tracyhip_genome_bytes(const tracyhip_genome* h) { return h ? h->bytes : 0; }

int tracyhip_genome_upload(tracyhip_ctx* ctx, const tracyhip_genome_desc* d, tracyhip_genome** out) {
  if (!out) return set_error(TRACYHIP_ERR_ARG, "null out pointer");
  *out = nullptr;
  const int rc = tracyhip_genome_validate(d);  // before any device call: a corrupt index never reaches a kernel
  if (rc != TRACYHIP_OK) return rc;
  const int rb = ctx_begin(ctx);
  if (rb != TRACYHIP_OK) return rb;
  tracyhip_genome* h = new tracyhip_genome();
  h->device = ctx->device;
  h->k = d->k; h->bucket_bits = d->bucket_bits; h->nc = d->ncontigs; h->ntab = d->ntab; h->text_len = d->text_len;
  SeedGenome& g = h->g;
  const uint8_t* text = nullptr;
  hipError_t e = upload(h, d->dir, (1ull << d->bucket_bits) + 1, &g.dir);
  if (e == hipSuccess) e = upload(h, d->tab, 2 * d->ntab, &g.tab);
  if (e == hipSuccess) e = upload_text(h, d, &text);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    tracyhip_genome_free(h);
    return set_error(e == hipErrorOutOfMemory ? TRACYHIP_ERR_OOM : TRACYHIP_ERR_HIP, "tracyhip_genome_upload: %s", hipGetErrorString(e));
  }
  g.text = text;
  g.ntab = d->ntab;
  g.text_len = d->text_len;
  g.nc = d->ncontigs;
  g.k = d->k;
  g.bucket_bits = d->bucket_bits;
  *out = h;
  return TRACYHIP_OK;
}

int tracyhip_genome_validate_text(const tracyhip_genome_desc* desc) {
  char why[256];
  const int rc = seed_validate_text(desc, why, sizeof(why));
  return rc == TRACYHIP_OK ? rc : set_error(rc, "tracyhip_genome_build: %s", why);
}

int tracyhip_genome_build(tracyhip_ctx* ctx, const tracyhip_genome_desc* d, tracyhip_genome** out) {
  if (!out) return set_error(TRACYHIP_ERR_ARG, "null out pointer");
  *out = nullptr;
  const int rc = tracyhip_genome_validate_text(d);  // before any device call
  if (rc != TRACYHIP_OK) return rc;
  const int rb = ctx_begin(ctx);
  if (rb != TRACYHIP_OK) return rb;
  tracyhip_genome* h = new tracyhip_genome();
  h->device = ctx->device;
  h->k = d->k; h->bucket_bits = d->bucket_bits; h->nc = d->ncontigs; h->text_len = d->text_len;
  SeedGenome& g = h->g;
  const uint8_t* text = nullptr;
  const uint64_t ndir = (1ull << d->bucket_bits) + 1;
  uint64_t* dir = nullptr;
  hipError_t e = hipMalloc(&dir, ndir * sizeof(uint64_t));
  if (e == hipSuccess) { h->mem.push_back(dir); h->bytes += ndir * sizeof(uint64_t); }
  if (e == hipSuccess) e = upload_text(h, d, &text);
  uint64_t* tab = nullptr;
  uint64_t ntab = 0;
  if (e == hipSuccess) e = index_build(ctx->stream, text, d->text_len, d->k, d->bucket_bits, dir, &tab, &ntab);
  if (e == hipSuccess) { h->mem.push_back(tab); h->bytes += std::max<uint64_t>(ntab, 1) * 2 * sizeof(uint64_t); }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    tracyhip_genome_free(h);
    return set_error(e == hipErrorOutOfMemory ? TRACYHIP_ERR_OOM : TRACYHIP_ERR_HIP, "tracyhip_genome_build: %s", hipGetErrorString(e));
  }
  g.dir = dir;
  g.tab = tab;
  g.text = text;
  g.ntab = h->ntab = ntab;
  g.text_len = d->text_len;
  g.nc = d->ncontigs;
  g.k = d->k;
  g.bucket_bits = d->bucket_bits;
  *out = h;
  return TRACYHIP_OK;
}

int tracyhip_genome_ntab(const tracyhip_genome* h, uint64_t* ntab) {
  if (!h || !ntab) return set_error(TRACYHIP_ERR_ARG, "null genome / ntab");
  *ntab = h->ntab;
  return TRACYHIP_OK;
}

int tracyhip_genome_download(const tracyhip_genome* h, uint64_t* dir, uint64_t* tab) {
  if (!h || !dir || (h->ntab && !tab)) return set_error(TRACYHIP_ERR_ARG, "null genome / dir / tab");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy(dir, h->g.dir, ((1ull << h->bucket_bits) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (h->ntab) HIP_TRY(hipMemcpy(tab, h->g.tab, h->ntab * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return TRACYHIP_OK;
}

int tracyhip_seed_traces(tracyhip_ctx* ctx, const tracyhip_genome* genome, const tracyhip_seqset* cons, const tracyhip_seed_params* prm, int mem,
                         const tracyhip_seed_result* out) {
  if (!genome || !cons || !prm || !out) return set_error(TRACYHIP_ERR_ARG, "null genome / consensus / params / result");
  if (cons->kind != TRACYHIP_SEQ_CHAR) return set_error(TRACYHIP_ERR_ARG, "consensus must be a CHAR set");
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return set_error(TRACYHIP_ERR_ARG, "bad mem");
  if ((prm->trim_left_each == nullptr) != (prm->trim_right_each == nullptr))
    return set_error(TRACYHIP_ERR_ARG, "trim_left_each and trim_right_each must be given together");
  const uint32_t n = cons->count;
  if (n == 0) return TRACYHIP_OK;
  if (!cons->data || !cons->offset || !cons->length) return set_error(TRACYHIP_ERR_ARG, "null consensus arrays");
  if (!out->status || !out->forward || !out->kmersupport || !out->pos || !out->contig || !out->slice_len || (!out->slices && out->slice_cap))
    return set_error(TRACYHIP_ERR_ARG, "null result array");
  int rc = ctx_begin(ctx);
  if (rc != TRACYHIP_OK) return rc;
  if (genome->device != ctx->device) return set_error(TRACYHIP_ERR_ARG, "genome uploaded to device %d, context on device %d", genome->device, ctx->device);
  ctx->stats.seed_spilled = ctx->stats.seed_spill_launches = ctx->stats.seed_spill_deferred = 0;  // (this call's; the other counters are the pipelines')
  const uint32_t cap = std::max<uint32_t>(1, std::min(ctx->knobs.seed_vote_cap, kSeedVoteCapMax));
  uint32_t P = 2;
  while (P < cap) P <<= 1;
  // host payloads go through in chunks (the staged windows of a chunk: at most ~512 MB of device memory); device payloads in one
  const uint64_t row = std::max<uint64_t>(out->slice_cap, 1);
  const uint32_t chunk = mem == TRACYHIP_MEM_DEVICE ? n : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, (512ull << 20) / row));
  std::vector<uint64_t> off;
  std::vector<SeedOut> res;
  for (uint32_t t0 = 0; t0 < n; t0 += chunk) {
    const uint32_t m = std::min(chunk, n - t0);
    // consensus: the chunk's span of the caller's bytes (host) or the caller's buffer itself (device); offsets relative to it
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < m; ++i) {
      lo = std::min(lo, cons->offset[t0 + i]);
      hi = std::max(hi, cons->offset[t0 + i] + cons->length[t0 + i]);
    }
    const uint8_t* d_cons = static_cast<const uint8_t*>(cons->data);
    if (mem == TRACYHIP_MEM_HOST) {
      HIP_TRY(ctx->dev[DB_SEED_CONS].ensure(hi - lo + 1));
      HIP_TRY(hipMemcpyAsync(ctx->dev[DB_SEED_CONS].p, d_cons + lo, hi - lo, hipMemcpyHostToDevice, ctx->stream));
      d_cons = static_cast<const uint8_t*>(ctx->dev[DB_SEED_CONS].p);
    } else {
      lo = 0;
    }
    // per-trace inputs and results: offsets (u64), lengths (u32), trims (two 16-bit values in a u32), SeedOut -- the inputs in one copy
    const size_t b_off = 0, b_len = b_off + 8ull * m, b_trim = b_len + 4ull * m, b_out = (b_trim + 4ull * m + 15) & ~15ull, b_end = b_out + sizeof(SeedOut) * m;
    off.resize(2 * (size_t)m);
    for (uint32_t i = 0; i < m; ++i) off[i] = cons->offset[t0 + i] - lo;
    std::memcpy(off.data() + m, cons->length + t0, 4ull * m);
    {
      uint32_t* tw = reinterpret_cast<uint32_t*>(off.data() + m) + m;
      for (uint32_t i = 0; i < m; ++i) {  // each value truncated to 16 bits as SageConfig holds it
        const uint32_t l = prm->trim_left_each ? prm->trim_left_each[t0 + i] : prm->trim_left, r = prm->trim_right_each ? prm->trim_right_each[t0 + i] : prm->trim_right;
        tw[i] = (l & 0xffffu) | ((r & 0xffffu) << 16);
      }
    }
    uint8_t* d0; HIP_TRY(ensure_into(ctx->dev[DB_SEED_TRACES], b_end, d0));
    HIP_TRY(hipMemcpyAsync(d0, off.data(), 16ull * m, hipMemcpyHostToDevice, ctx->stream));
    uint8_t* d_slices = out->slices + (uint64_t)t0 * out->slice_cap;
    if (mem == TRACYHIP_MEM_HOST) {
      HIP_TRY(ensure_into(ctx->dev[DB_SEED_WINDOWS], (uint64_t)m * row, d_slices));
      HIP_TRY(hipMemsetAsync(d_slices, 0, (uint64_t)m * out->slice_cap, ctx->stream));
    }
    SeedArgs a;
    a.g = genome->g;
    a.cons = d_cons;
    a.off = reinterpret_cast<const uint64_t*>(d0 + b_off);
    a.len = reinterpret_cast<const uint32_t*>(d0 + b_len);
    a.out = reinterpret_cast<SeedOut*>(d0 + b_out);
    a.slices = d_slices;
    a.slice_cap = out->slice_cap;
    a.n = m;
    a.P = P;
    a.cap = cap;
    a.trims = reinterpret_cast<const uint32_t*>(d0 + b_trim);
    a.kmer = (uint16_t)prm->kmer;
    a.min_support = (uint16_t)prm->min_support;
    a.maxindel = (uint16_t)prm->maxindel;
    a.spill = ctx->knobs.seed_spill ? 1u : 0u;
    hipLaunchKernelGGL(seed_traces_kernel, dim3(m), dim3(kSeedThreads), 2 * P * sizeof(int64_t), ctx->stream, a);
    HIP_TRY(hipGetLastError());
    res.resize(m);
    HIP_TRY(hipMemcpyAsync(res.data(), a.out, sizeof(SeedOut) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (mem == TRACYHIP_MEM_HOST && out->slice_cap)
      HIP_TRY(hipMemcpyAsync(out->slices + (uint64_t)t0 * out->slice_cap, d_slices, (uint64_t)m * out->slice_cap, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx_sync(ctx));
    if (a.spill) {
      rc = seed_spilled_traces(ctx, a, res, mem == TRACYHIP_MEM_HOST ? out->slices + (uint64_t)t0 * out->slice_cap : nullptr);
      if (rc != TRACYHIP_OK) return rc;
    }
    for (uint32_t i = 0; i < m; ++i) {  // metadata: status and slice_len always, the rest for anchored traces only
      const SeedOut& o = res[i];
      const uint32_t t = t0 + i;
      out->status[t] = o.status;
      out->slice_len[t] = o.status == TRACYHIP_SEED_ANCHORED ? o.slice_len : 0;
      if (o.status != TRACYHIP_SEED_ANCHORED) continue;
      out->forward[t] = (uint8_t)o.forward;
      out->kmersupport[t] = o.kmersupport;
      out->pos[t] = o.pos;
      out->contig[t] = o.contig;
    }
  }
  return TRACYHIP_OK;
}

}  // extern "C"
