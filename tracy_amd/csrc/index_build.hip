// index_build.hip -- the k-mer table of a genome built on the device (index_build.h): GenomeIndex::build's directory and table, word
// for word.
//
// The bucket directory is the exclusive scan of a histogram over the 2^bucket_bits slots, so the sort is a bucket sort whose first level
// is the directory itself: count, scan, scatter every entry into its bucket, then sort each bucket by (code, pos).  Buckets hold ~3
// entries at 50 Mb and 2^24 slots (one thread sorts them in registers), ~170 at 3 Gb (one wave sorts them in LDS); repeats -- a poly-A
// run, satellites, k <= 12 where a slot is one code -- put up to millions into one bucket, which is cut into LDS-sorted chunks and
// merged by global passes.  Every hand-off between workgroups is a kernel boundary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "index_build.h"
#include "seed.h"

namespace tracyhip {
namespace {

// GenomeIndex::base2: 0..3 for A C G T (upper case only), 4 for any other byte ('\n' between contigs included)
__device__ __forceinline__ uint32_t ib_letter(uint8_t c) {
  switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: return 4;
  }
}

__device__ __forceinline__ bool ib_less(uint64_t ca, uint64_t pa, uint64_t cb, uint64_t pb) { return ca < cb || (ca == cb && pa < pb); }

// Passes 1 and 3.  Workgroup b holds windows [b * kIbTile, (b + 1) * kIbTile): their text plus the (k - 1)-byte halo is read coalesced
// into LDS, then every thread rolls the code over its kIbPer consecutive windows.  Consecutive windows of one bucket (homopolymer runs)
// take one atomic per run: a poly-A stretch costs 1/kIbPer of the adds on its one slot.
template <bool kScatter>
__global__ __launch_bounds__(kIbThreads) void ib_keys(const uint8_t* __restrict__ text, uint64_t text_len, uint64_t nwin, uint32_t k,
                                                      uint64_t bmask, unsigned long long* __restrict__ cnt, uint64_t* __restrict__ tab) {
  __shared__ uint8_t tile[kIbTile + 32];
  const uint64_t p0 = (uint64_t)blockIdx.x * kIbTile;
  const uint32_t span = kIbTile + k - 1;
  for (uint32_t i = threadIdx.x; i < span; i += kIbThreads) {
    const uint64_t q = p0 + i;
    tile[i] = q < text_len ? text[q] : (uint8_t)0;
  }
  __syncthreads();
  const uint32_t t0 = threadIdx.x * kIbPer;
  const uint64_t mask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
  uint64_t code = 0;
  uint32_t run = 0;  // ACGT letters ending here, capped at k
  for (uint32_t q = 0; q + 1 < k; ++q) {
    const uint32_t b = ib_letter(tile[t0 + q]);
    if (b > 3) { run = 0; code = 0; }
    else { code = ((code << 2) | b) & mask; run = run < k ? run + 1 : k; }
  }
  uint64_t key[kIbPer];
  bool ok[kIbPer], flip[kIbPer];
#pragma unroll
  for (uint32_t j = 0; j < kIbPer; ++j) {
    const uint32_t b = ib_letter(tile[t0 + j + k - 1]);
    if (b > 3) { run = 0; code = 0; }
    else { code = ((code << 2) | b) & mask; run = run < k ? run + 1 : k; }
    const uint64_t rc = seed_revcomp(code, k);
    ok[j] = run == k && p0 + t0 + j < nwin;
    flip[j] = rc < code;
    key[j] = flip[j] ? rc : code;
  }
  uint32_t len[kIbPer];  // entries of the run of one slot that starts at window j
#pragma unroll
  for (int j = (int)kIbPer - 1; j >= 0; --j) {
    const bool joins = j + 1 < (int)kIbPer && ok[j] && ok[j + 1] && ((key[j] ^ key[j + 1]) & bmask) == 0;
    len[j] = joins ? len[j + 1] + 1 : 1;
  }
  uint64_t at = 0;
#pragma unroll
  for (uint32_t j = 0; j < kIbPer; ++j) {
    if (!ok[j]) continue;
    const bool starts = j == 0 || !ok[j - 1] || ((key[j] ^ key[j - 1]) & bmask) != 0;
    unsigned long long* c = cnt + (key[j] & bmask);
    if (kScatter) {
      if (starts) at = atomicAdd(c, (unsigned long long)len[j]);
      const uint64_t pos = (p0 + t0 + j) | (flip[j] ? kSeedFlipped : 0ull);
      *reinterpret_cast<ulonglong2*>(tab + 2 * at) = make_ulonglong2(key[j], pos);
      ++at;
    } else if (starts) {
      atomicAdd(c, (unsigned long long)len[j]);
    }
  }
}

// Exclusive scan, tile level: out[i] = the sum of v[tile start .. i) with v[i] = in[i] for i < n_in, 0 beyond (so out[n_in] is the
// total); sums[tile] = the tile's total.  kScanPer consecutive words per thread, the thread totals scanned in LDS.
constexpr uint32_t kScanThreads = 256, kScanPer = 8, kScanTile = kScanThreads * kScanPer;
__global__ __launch_bounds__(kScanThreads) void ib_scan_tile(const uint64_t* __restrict__ in, uint64_t n_in, uint64_t m, uint64_t* __restrict__ out,
                                                             uint64_t* __restrict__ sums) {
  __shared__ uint64_t s[kScanThreads];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
  uint64_t v[kScanPer], tot = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    v[j] = base + j < n_in ? in[base + j] : 0;
    tot += v[j];
  }
  s[threadIdx.x] = tot;
  __syncthreads();
  for (uint32_t d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan of the thread totals (Hillis-Steele)
    const uint64_t add = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  uint64_t acc = s[threadIdx.x] - tot;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    if (base + j < m) out[base + j] = acc;
    acc += v[j];
  }
  if (sums && threadIdx.x == kScanThreads - 1) sums[blockIdx.x] = s[threadIdx.x];
}

__global__ void ib_scan_add(uint64_t* __restrict__ out, uint64_t m, const uint64_t* __restrict__ offs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] += offs[i / kScanTile];
}

// Pass 4a: one thread per bucket.  Up to kIbSmall entries: sorted in registers (odd-even transposition over a fixed-size array, padded
// with the largest key); longer buckets are listed -- up to kIbChunk entries as {lo, lo, n} for the LDS sort, longer as {lo, n} for
// the chunked sort + merge.  counters: [0] listed for LDS, [1] listed long, [2] the longest bucket listed for LDS.
__global__ __launch_bounds__(256) void ib_small(const uint64_t* __restrict__ dir, uint64_t nb, uint64_t* __restrict__ tab,
                                                uint64_t* __restrict__ mid, uint64_t mid_cap, uint64_t* __restrict__ large, uint64_t large_cap,
                                                unsigned long long* __restrict__ counters) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  const uint64_t lo = dir[b], n = dir[b + 1] - lo;
  if (n <= 1) return;
  if (n <= kIbSmall) {
    uint64_t c[kIbSmall], p[kIbSmall];
#pragma unroll
    for (uint32_t i = 0; i < kIbSmall; ++i) {
      c[i] = ~0ull;
      p[i] = ~0ull;
      if (i < n) {
        const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(tab + 2 * (lo + i));
        c[i] = e.x;
        p[i] = e.y;
      }
    }
#pragma unroll
    for (uint32_t r = 0; r < kIbSmall; ++r) {
#pragma unroll
      for (uint32_t i = r & 1; i + 1 < kIbSmall; i += 2) {
        if (ib_less(c[i + 1], p[i + 1], c[i], p[i])) {
          const uint64_t tc = c[i], tp = p[i];
          c[i] = c[i + 1]; p[i] = p[i + 1];
          c[i + 1] = tc; p[i + 1] = tp;
        }
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < kIbSmall; ++i)
      if (i < n) *reinterpret_cast<ulonglong2*>(tab + 2 * (lo + i)) = make_ulonglong2(c[i], p[i]);
  } else if (n <= kIbChunk) {
    const unsigned long long i = atomicAdd(&counters[0], 1ull);
    atomicMax(&counters[2], (unsigned long long)n);
    if (i < mid_cap) { mid[3 * i] = lo; mid[3 * i + 1] = lo; mid[3 * i + 2] = n; }
  } else {
    const unsigned long long i = atomicAdd(&counters[1], 1ull);
    if (i < large_cap) { large[2 * i] = lo; large[2 * i + 1] = n; }
  }
}

// Pass 4b: one wave per segment {src index, dst index, n <= kIbChunk}: bitonic sort in LDS over the next power of two >= n (padded with
// the largest key), written to dst.  Dynamic LDS: 2 x P2 words, P2 >= every n of the launch.
__global__ __launch_bounds__(64) void ib_chunk_sort(const uint64_t* __restrict__ segs, const uint64_t* src, uint64_t* dst) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
  const uint64_t slo = segs[3 * blockIdx.x], dlo = segs[3 * blockIdx.x + 1];
  const uint32_t n = (uint32_t)segs[3 * blockIdx.x + 2], tid = threadIdx.x;
  uint32_t P = 2;
  while (P < n) P <<= 1;
  uint64_t* lc = lds;
  uint64_t* lp = lds + P;
  for (uint32_t i = tid; i < P; i += 64) {
    ulonglong2 e = make_ulonglong2(~0ull, ~0ull);
    if (i < n) e = *reinterpret_cast<const ulonglong2*>(src + 2 * (slo + i));
    lc[i] = e.x;
    lp[i] = e.y;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t x = tid; x < (P >> 1); x += 64) {
        const uint32_t i = ((x & ~(stride - 1)) << 1) | (x & (stride - 1)), j = i + stride;
        const bool up = (i & size) == 0;
        const uint64_t ci = lc[i], pi = lp[i], cj = lc[j], pj = lp[j];
        if (ib_less(cj, pj, ci, pi) == up) { lc[i] = cj; lp[i] = pj; lc[j] = ci; lp[j] = pi; }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < n; i += 64) *reinterpret_cast<ulonglong2*>(dst + 2 * (dlo + i)) = make_ulonglong2(lc[i], lp[i]);
}

// Pass 4c: one merge pass over every long bucket at once.  Long bucket s holds n_s = toff[s + 1] - toff[s] entries, at index lo[s] of
// the table and at index toff[s] of the scratch array; the pass reads sorted runs of w entries from one place and writes sorted runs of 2w
// to the other.  Thread g moves entry g of the concatenation: its rank in the partner run (keys are unique: a binary search for the
// entries below it) plus its own offset gives its place.
__global__ __launch_bounds__(256) void ib_merge(const uint64_t* __restrict__ toff, const uint64_t* __restrict__ lo, uint32_t L, uint64_t T,
                                                uint64_t w, bool from_tab, uint64_t* tab, uint64_t* scratch) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < T; g += (uint64_t)gridDim.x * blockDim.x) {
  uint32_t a = 0, z = L - 1;  // the last s with toff[s] <= g
  while (a < z) {
    const uint32_t m = (a + z + 1) >> 1;
    if (toff[m] <= g) a = m;
    else z = m - 1;
  }
  const uint64_t n = toff[a + 1] - toff[a], i = g - toff[a];
  const uint64_t* src = from_tab ? tab + 2 * lo[a] : scratch + 2 * toff[a];
  uint64_t* dst = from_tab ? scratch + 2 * toff[a] : tab + 2 * lo[a];
  const uint64_t r = i / w, a0 = (r & ~1ull) * w;
  const bool left = (r & 1) == 0;
  const uint64_t o_lo = left ? a0 + w : a0;
  const uint64_t o_hi = left ? (a0 + 2 * w < n ? a0 + 2 * w : n) : a0 + w;
  const ulonglong2 me = *reinterpret_cast<const ulonglong2*>(src + 2 * i);
  uint64_t x = o_lo < o_hi ? o_lo : o_hi, y = o_hi;  // first index of the partner run whose entry is not below me
  while (x < y) {
    const uint64_t m = (x + y) >> 1;
    if (ib_less(src[2 * m], src[2 * m + 1], me.x, me.y)) x = m + 1;
    else y = m;
  }
  const uint64_t below = x - (o_lo < o_hi ? o_lo : o_hi);
  const uint64_t out = a0 + (i - (left ? a0 : a0 + w)) + below;
  *reinterpret_cast<ulonglong2*>(dst + 2 * out) = me;
  }
}

// device temporaries of one build: every one freed when the build returns, whatever happened
struct Temps {
  std::vector<void*> p;
  template <class T>
  hipError_t get(T** out, uint64_t count) {
    *out = nullptr;
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<uint64_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    p.push_back(q);
    *out = static_cast<T*>(q);
    return hipSuccess;
  }
  ~Temps() {
    for (void* q : p) (void)hipFree(q);
  }
};

#define IB_TRY(expr)                       \
  do {                                     \
    const hipError_t e_ = (expr);          \
    if (e_ != hipSuccess) return e_;       \
  } while (0)

uint32_t grid_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

// out[0 .. n] = exclusive prefix sums of in[0 .. n) (out[n] = the total)
hipError_t scan_excl(hipStream_t st, const uint64_t* in, uint64_t n, uint64_t* out, Temps& tmp) {
  const uint64_t m = n + 1, nt = (m + kScanTile - 1) / kScanTile;
  if (nt == 1) {
    hipLaunchKernelGGL(ib_scan_tile, dim3(1), dim3(kScanThreads), 0, st, in, n, m, out, (uint64_t*)nullptr);
    return hipGetLastError();
  }
  uint64_t *sums = nullptr, *offs = nullptr;
  IB_TRY(tmp.get(&sums, nt));
  IB_TRY(tmp.get(&offs, nt + 1));
  hipLaunchKernelGGL(ib_scan_tile, dim3((uint32_t)nt), dim3(kScanThreads), 0, st, in, n, m, out, sums);
  IB_TRY(hipGetLastError());
  IB_TRY(scan_excl(st, sums, nt, offs, tmp));
  hipLaunchKernelGGL(ib_scan_add, dim3(grid_of(m, 256)), dim3(256), 0, st, out, m, (const uint64_t*)offs);
  return hipGetLastError();
}

hipError_t build_into(hipStream_t st, const uint8_t* text, uint64_t text_len, uint32_t k, uint32_t bits, uint64_t* dir, uint64_t** tab_out,
                      uint64_t* ntab_out, Temps& tmp) {
  const uint64_t nb = 1ull << bits, bmask = nb - 1;
  const uint64_t nwin = text_len >= k ? text_len - k + 1 : 0;
  // 1 + 2: histogram, directory
  unsigned long long* cnt = nullptr;
  IB_TRY(tmp.get(&cnt, nb));
  IB_TRY(hipMemsetAsync(cnt, 0, nb * sizeof(uint64_t), st));
  const uint32_t tiles = grid_of(nwin, kIbTile);
  if (tiles) {
    hipLaunchKernelGGL(ib_keys<false>, dim3(tiles), dim3(kIbThreads), 0, st, text, text_len, nwin, k, bmask, cnt, (uint64_t*)nullptr);
    IB_TRY(hipGetLastError());
  }
  IB_TRY(scan_excl(st, reinterpret_cast<const uint64_t*>(cnt), nb, dir, tmp));
  uint64_t ntab = 0;
  IB_TRY(hipMemcpyAsync(&ntab, dir + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IB_TRY(hipStreamSynchronize(st));
  if (ntab > nwin) return hipErrorUnknown;  // (cannot happen: every entry is a window)
  uint64_t* tab = nullptr;
  IB_TRY(tmp.get(&tab, 2 * ntab));  // (held as a temporary until the build has succeeded)
  if (ntab) {
    // 3: scatter (the histogram becomes the cursor: each bucket's next free index)
    IB_TRY(hipMemcpyAsync(cnt, dir, nb * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(ib_keys<true>, dim3(tiles), dim3(kIbThreads), 0, st, text, text_len, nwin, k, bmask, cnt, tab);
    IB_TRY(hipGetLastError());
    // 4a: small buckets; the others listed
    const uint64_t mid_cap = std::min<uint64_t>(nb, ntab / (kIbSmall + 1) + 1), large_cap = std::min<uint64_t>(nb, ntab / (kIbChunk + 1) + 1);
    uint64_t *mid = nullptr, *large = nullptr;
    unsigned long long* counters = nullptr;
    IB_TRY(tmp.get(&mid, 3 * mid_cap));
    IB_TRY(tmp.get(&large, 2 * large_cap));
    IB_TRY(tmp.get(&counters, 3));
    IB_TRY(hipMemsetAsync(counters, 0, 3 * sizeof(uint64_t), st));
    hipLaunchKernelGGL(ib_small, dim3(grid_of(nb, 256)), dim3(256), 0, st, (const uint64_t*)dir, nb, tab, mid, mid_cap, large, large_cap, counters);
    IB_TRY(hipGetLastError());
    uint64_t cn[3] = {0, 0, 0};
    IB_TRY(hipMemcpyAsync(cn, counters, sizeof(cn), hipMemcpyDeviceToHost, st));
    IB_TRY(hipStreamSynchronize(st));
    if (cn[0] > mid_cap || cn[1] > large_cap || cn[2] > kIbChunk) return hipErrorUnknown;  // (cannot happen: the caps count what fits)
    // 4b: buckets that fit one LDS sort
    if (cn[0]) {
      uint32_t P = 2;
      while (P < cn[2]) P <<= 1;
      hipLaunchKernelGGL(ib_chunk_sort, dim3((uint32_t)cn[0]), dim3(64), 2 * P * sizeof(uint64_t), st, (const uint64_t*)mid, (const uint64_t*)tab, tab);
      IB_TRY(hipGetLastError());
    }
    // 4c: long buckets: LDS-sorted chunks, then merge passes that double the sorted runs until each bucket is one run; the chunks go
    // to the scratch array when the number of passes is odd, so that the last pass writes the table
    if (cn[1]) {
      std::vector<uint64_t> lg(2 * cn[1]);
      IB_TRY(hipMemcpyAsync(lg.data(), large, lg.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      IB_TRY(hipStreamSynchronize(st));
      const uint32_t L = (uint32_t)cn[1];
      std::vector<uint64_t> lo(L), toff(L + 1, 0);
      std::vector<uint32_t> ord(L);
      for (uint32_t s = 0; s < L; ++s) ord[s] = s;
      std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return lg[2 * a] < lg[2 * b]; });  // (a layout independent of the listing order)
      uint64_t maxn = 0;
      for (uint32_t s = 0; s < L; ++s) {
        lo[s] = lg[2 * ord[s]];
        toff[s + 1] = toff[s] + lg[2 * ord[s] + 1];
        maxn = std::max(maxn, lg[2 * ord[s] + 1]);
      }
      const uint64_t T = toff[L];
      uint32_t passes = 0;
      for (uint64_t w = kIbChunk; w < maxn; w <<= 1) ++passes;
      const bool to_scratch = passes & 1;
      std::vector<uint64_t> chunks;
      for (uint32_t s = 0; s < L; ++s) {
        const uint64_t n = toff[s + 1] - toff[s];
        for (uint64_t c = 0; c < n; c += kIbChunk) {
          chunks.push_back(lo[s] + c);
          chunks.push_back(to_scratch ? toff[s] + c : lo[s] + c);
          chunks.push_back(std::min<uint64_t>(kIbChunk, n - c));
        }
      }
      uint64_t *scratch = nullptr, *d_chunks = nullptr, *d_toff = nullptr, *d_lo = nullptr;
      IB_TRY(tmp.get(&scratch, 2 * T));
      IB_TRY(tmp.get(&d_chunks, chunks.size()));
      IB_TRY(tmp.get(&d_toff, L + 1));
      IB_TRY(tmp.get(&d_lo, L));
      IB_TRY(hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      IB_TRY(hipMemcpyAsync(d_toff, toff.data(), toff.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      IB_TRY(hipMemcpyAsync(d_lo, lo.data(), lo.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(ib_chunk_sort, dim3((uint32_t)(chunks.size() / 3)), dim3(64), 2 * kIbChunk * sizeof(uint64_t), st, (const uint64_t*)d_chunks,
                         (const uint64_t*)tab, to_scratch ? scratch : tab);
      IB_TRY(hipGetLastError());
      bool from_tab = !to_scratch;
      for (uint64_t w = kIbChunk; w < maxn; w <<= 1) {
        hipLaunchKernelGGL(ib_merge, dim3(std::min<uint32_t>(grid_of(T, 256), 1u << 20)), dim3(256), 0, st, (const uint64_t*)d_toff, (const uint64_t*)d_lo, L, T, w, from_tab, tab,
                           scratch);
        IB_TRY(hipGetLastError());
        from_tab = !from_tab;
      }
      // (the chunk lists live until the stream has run them: synchronised below, before Temps frees them)
    }
  }
  IB_TRY(hipStreamSynchronize(st));
  tmp.p.erase(std::find(tmp.p.begin(), tmp.p.end(), static_cast<void*>(tab)));  // the table is the caller's from here
  *tab_out = tab;
  *ntab_out = ntab;
  return hipSuccess;
}

}  // namespace

hipError_t index_build(hipStream_t st, const uint8_t* text, uint64_t text_len, uint32_t k, uint32_t bits, uint64_t* dir, uint64_t** tab,
                       uint64_t* ntab) {
  *tab = nullptr;
  *ntab = 0;
  if (k < 1 || k > 32 || bits > 24 || bits > 2 * k) return hipErrorInvalidValue;
  Temps tmp;
  const hipError_t e = build_into(st, text, text_len, k, bits, dir, tab, ntab, tmp);
  if (e != hipSuccess) (void)hipStreamSynchronize(st);  // (nothing queued may still use a temporary when it is freed)
  return e;
}

}  // namespace tracyhip
