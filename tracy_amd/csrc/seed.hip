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
};

__device__ __forceinline__ void write_status(const SeedArgs& a, uint32_t t, int32_t st) {
  a.out[t].status = st;
  a.out[t].slice_len = 0;
}

// best (length, value) of two runs: the longer, on ties the smaller value (findMaxFreq keeps the first of the sorted runs)
__device__ __forceinline__ void better(uint32_t& bl, int64_t& bv, uint32_t l, int64_t v) {
  if (l > bl || (l == bl && l != 0 && v < bv)) { bl = l; bv = v; }
}

__global__ __launch_bounds__(kSeedThreads) void seed_traces_kernel(SeedArgs a) {
  extern __shared__ int64_t lists[];  // [2][P]: forward votes, reverse votes
  __shared__ uint32_t s_n[2];
  __shared__ uint32_t s_bad;
  __shared__ uint32_t s_len[2][kSeedThreads / 64];
  __shared__ int64_t s_val[2][kSeedThreads / 64];
  __shared__ uint64_t s_src, s_wlen;
  __shared__ uint32_t s_fwd;
  const uint32_t t = blockIdx.x, tid = threadIdx.x;
  const uint32_t S = a.len[t];
  const uint8_t* c = a.cons + a.off[t];
  const uint32_t trims = a.trims[t];  // (indexed by the block: a scalar load)
  const uint32_t k = a.kmer, TL = trims & 0xffffu, TR = trims >> 16;
  // the domain of scanBothStrands (seed.hpp:614-619); outside it the host runs its two scans
  if (k != a.g.k || k < 1 || k > 32 || (uint64_t)S + k >= 65536u || TL + 1 < k || TR + 1 < k || S < TL || S < TR) {
    if (tid == 0) write_status(a, t, TRACYHIP_SEED_DEFERRED);
    return;
  }
  if (S <= TL + TR) {  // no window on either strand: zero votes in both passes
    if (tid == 0) write_status(a, t, TRACYHIP_SEED_UNANCHORED);
    return;
  }
  const uint32_t p_lo = TL + 1 - k, p_hi = S - TR, nwin = p_hi - p_lo;
  const uint32_t fwd_from = k - 1, rev_until = nwin >= k ? nwin - k + 1 : 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  // letters among the windows: A C G T N only (anything else: the host's two scans, seed.hpp:636)
  {
    uint32_t bad = 0;
    for (uint32_t q = p_lo + tid; q < p_hi - 1 + k; q += kSeedThreads) bad |= seed_letter(c[q]) == 5 ? 1u : 0u;
    if (bad) atomicOr(&s_bad, 1u);
  }
  __syncthreads();
  if (s_bad) {
    if (tid == 0) write_status(a, t, TRACYHIP_SEED_DEFERRED);
    return;
  }
  const uint64_t mask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
  const uint64_t bmask = (1ull << a.g.bucket_bits) - 1ull;
  int64_t* const lf = lists;
  int64_t* const lr = lists + a.P;
  uint32_t freqF = 0, freqR = 0;
  int64_t bestF = 0, bestR = 0;
  bool anchored = false, fwd = false;
  for (int pass = 0; pass < 2 && !anchored; ++pass) {
    const bool unique = pass == 0;
    if (tid == 0) { s_n[0] = 0; s_n[1] = 0; }
    __syncthreads();
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
          lo[j] = a.g.dir[b];
          hi[j] = a.g.dir[b + 1];
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < kSeedWin; ++j) {
        if (!info[j]) continue;
        const uint64_t e = hi[j] < a.g.ntab ? hi[j] : a.g.ntab;
        uint64_t i = lo[j] < e ? lo[j] : e;
        const uint64_t kk = key[j];
        while (i < e && a.g.tab[2 * i] < kk) ++i;
        const uint64_t own = i;  // [own, mid): the run's own code, [mid, end): its reverse complement's
        while (i < e && a.g.tab[2 * i] == kk && !(a.g.tab[2 * i + 1] & kSeedFlipped)) ++i;
        const uint64_t mid = i;
        while (i < e && a.g.tab[2 * i] == kk) ++i;
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
          const uint32_t slot = atomicAdd(&s_n[strand], (uint32_t)occs);
          int64_t* l = strand == 0 ? lf : lr;
          for (uint64_t q = 0; q < occs; ++q)
            if (slot + q < a.P) l[slot + q] = (int64_t)(a.g.tab[2 * (qlo + q) + 1] & ~kSeedFlipped) - at;
        }
      }
    }
    __syncthreads();
    const uint32_t nF = s_n[0], nR = s_n[1];
    if (nF > a.cap || nR > a.cap) {  // more votes than the lists hold: the host seeds this trace
      if (tid == 0) write_status(a, t, TRACYHIP_SEED_DEFERRED);
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
        better(bl[s], bv[s], lo2 - i, v);
      }
      for (int d = 32; d > 0; d >>= 1) {
        const uint32_t ol = __shfl_xor(bl[s], d);
        const int64_t ov = __shfl_xor(bv[s], d);
        better(bl[s], bv[s], ol, ov);
      }
    }
    if ((tid & 63) == 0) {
      for (int s = 0; s < 2; ++s) { s_len[s][tid >> 6] = bl[s]; s_val[s][tid >> 6] = bv[s]; }
    }
    __syncthreads();
    for (int s = 0; s < 2; ++s) {
      uint32_t l = 0;
      int64_t v = 0;
      for (uint32_t w = 0; w < kSeedThreads / 64; ++w) better(l, v, s_len[s][w], s_val[s][w]);
      if (s == 0) { freqF = l; bestF = v; } else { freqR = l; bestR = v; }
    }
    __syncthreads();  // (the lists and s_n are rewritten by the next pass)
    if (freqF >= a.min_support && freqF > 2 * freqR) { anchored = true; fwd = true; }
    else if (freqR >= a.min_support && freqR > 2 * freqF) { anchored = true; fwd = false; }
  }
  if (!anchored) {
    if (tid == 0) write_status(a, t, TRACYHIP_SEED_UNANCHORED);
    return;
  }
  if (tid == 0) {
    const SeedWindow win = seed_window(a.g.cum, a.g.starts, a.g.lengths, a.g.nc, a.g.text_len, fwd ? bestF : bestR, S, (uint16_t)a.maxindel);
    const uint64_t n = win.len < a.slice_cap ? win.len : a.slice_cap;
    s_src = win.src;
    s_wlen = win.len;
    s_fwd = fwd ? 1u : 0u;
    SeedOut o;
    o.status = TRACYHIP_SEED_ANCHORED;
    o.forward = fwd ? 1u : 0u;
    o.kmersupport = fwd ? freqF : freqR;
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
  if (s_fwd) {
    for (uint64_t i = tid; i < n; i += kSeedThreads) dst[i] = src[i];
  } else {
    for (uint64_t i = tid; i < n; i += kSeedThreads) {
      const uint8_t cc = seed_complement(src[L - 1 - i]);
      dst[i] = cc ? cc : src[i];
    }
  }
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
    hipLaunchKernelGGL(seed_traces_kernel, dim3(m), dim3(kSeedThreads), 2 * P * sizeof(int64_t), ctx->stream, a);
    HIP_TRY(hipGetLastError());
    res.resize(m);
    HIP_TRY(hipMemcpyAsync(res.data(), a.out, sizeof(SeedOut) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (mem == TRACYHIP_MEM_HOST && out->slice_cap)
      HIP_TRY(hipMemcpyAsync(out->slices + (uint64_t)t0 * out->slice_cap, d_slices, (uint64_t)m * out->slice_cap, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx_sync(ctx));
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
