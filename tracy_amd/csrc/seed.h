// seed.h -- getReferenceSlice (fmindex.h:236-326) on the device: the per-trace rules of tracy_amd/host/seed.hpp (scanBothStrands,
// GenomeIndex::both_strands, findMaxFreq, the window geometry) as functions the kernel of seed.hip calls, plus the host-side check of
// an index descriptor.  Plain C++ apart from SEED_HD: the scalar rules compile with g++ as well.
#ifndef TRACY_AMD_SEED_H
#define TRACY_AMD_SEED_H

#include <stdint.h>

#include <cstdio>

#include "../../include/tracy_hip.h"

#if defined(__HIPCC__)
#define SEED_HD __host__ __device__ inline
#else
#define SEED_HD inline
#endif

namespace tracyhip {

constexpr uint64_t kSeedFlipped = 1ull << 63;  // bit 63 of a table entry's pos: the text holds the run code's reverse complement
constexpr uint32_t kSeedThreads = 256;         // one workgroup per trace
constexpr uint32_t kSeedVoteCapMax = 2048;     // votes per strand and pass held in LDS (2 x 2048 x 8 B = 32 KiB per workgroup)
constexpr uint32_t kSeedWin = 4;               // windows a lane looks up at once (their directory loads, then their table loads, in flight together)

// the uploaded index (device pointers)
struct SeedGenome {
  const uint64_t* dir;
  const uint64_t* tab;      // {code, pos} pairs
  uint64_t ntab;
  const uint8_t* text;
  uint64_t text_len;
  const int64_t* cum;       // [nc] sum of (length + 1) of the contigs before: the walk of getReferenceSlice (seed.hpp:723)
  const uint64_t* starts;
  const uint32_t* lengths;
  const uint32_t* contig_id;
  uint32_t nc, k, bucket_bits;
};

// one trace's result as the kernel leaves it (copied to the caller's host arrays afterwards)
struct SeedOut {
  int32_t status;
  uint32_t forward, kmersupport, pos, contig, slice_len;
};

// Internal status of the first kernel (never returned to a caller: 0 .. 2 are the public values): the trace collected more votes
// than the LDS lists hold and the context's seed_spill is on.  Its SeedOut then reads as a SeedSpillOut.
constexpr int32_t kSeedSpill = 3;
struct SeedSpillOut {
  int32_t status;        // kSeedSpill
  uint32_t pass;         // the pass whose lists overflowed: 0 = unique k-mers, 1 = every k-mer below 1000 occurrences
  uint32_t votes[2][2];  // [pass][strand]: the exact votes of the pass that overflowed and, where that was pass 0, of pass 1 as well
};
static_assert(sizeof(SeedSpillOut) == sizeof(SeedOut), "a spilled trace reports in its own result record");

// ---- vote counting beyond LDS: findMaxFreq (fmindex.h:173-198) over a counting hash table ----
// One table per strand: slots of {value, count}, a power of two >= 2 x the votes inserted (so never full), linear probing.  A slot
// is claimed by a compare-and-swap on its value and counted by an add, so the final table -- and with the tie rule below the
// answer -- does not depend on the order of the inserts.  Memory goes through a policy `Mem` (load / claim / add): atomics on the
// device (seed.hip), plain accesses in SeedMemPlain for one thread on the host.
struct SeedSlot {
  int64_t value;
  uint32_t count, pad;
};
// a vote is position - offset with position >= 0 and offset < 65 536: never this value
constexpr int64_t kSeedSlotEmpty = INT64_MIN;
constexpr uint64_t kSeedTableMin = 64;

SEED_HD uint64_t seed_table_capacity(uint64_t votes) {
  uint64_t c = kSeedTableMin;
  while (c < 2 * votes) c <<= 1;
  return c;
}
// the slot a value's probe starts at (mask = capacity - 1)
SEED_HD uint64_t seed_slot_of(int64_t v, uint64_t mask) {
  uint64_t h = (uint64_t)v * 0x9e3779b97f4a7c15ull;
  h ^= h >> 32;
  return h & mask;
}
struct SeedMemPlain {
  static SEED_HD int64_t load(const int64_t* p) { return *p; }
  static SEED_HD uint32_t load(const uint32_t* p) { return *p; }
  static SEED_HD void store(int64_t* p, int64_t v) { *p = v; }
  static SEED_HD void store(uint32_t* p, uint32_t v) { *p = v; }
  static SEED_HD int64_t claim(int64_t* p, int64_t expected, int64_t v) {  // compare-and-swap: what *p held before
    const int64_t old = *p;
    if (old == expected) *p = v;
    return old;
  }
  static SEED_HD void add(uint32_t* p, uint32_t n) { *p += n; }
};
// slots lo, lo + step, ... of a table set to empty
template <class Mem>
SEED_HD void seed_table_clear(SeedSlot* tab, uint64_t capacity, uint64_t lo, uint64_t step) {
  for (uint64_t i = lo; i < capacity; i += step) {
    Mem::store(&tab[i].value, kSeedSlotEmpty);
    Mem::store(&tab[i].count, 0u);
  }
}
// one vote: probe from the value's slot to its own slot or the first empty one, which it claims.  false: no slot within `capacity`
// probes (a table smaller than its votes: not reached with seed_table_capacity)
template <class Mem>
SEED_HD bool seed_table_insert(SeedSlot* tab, uint64_t capacity, int64_t v) {
  const uint64_t mask = capacity - 1;
  uint64_t s = seed_slot_of(v, mask);
  for (uint64_t probes = 0; probes < capacity; ++probes, s = (s + 1) & mask) {
    int64_t held = Mem::load(&tab[s].value);
    if (held == kSeedSlotEmpty) held = Mem::claim(&tab[s].value, kSeedSlotEmpty, v);
    if (held == kSeedSlotEmpty || held == v) {
      Mem::add(&tab[s].count, 1u);
      return true;
    }
  }
  return false;
}
// best (length, value) of two runs: the longer, on ties the smaller value (findMaxFreq keeps the first of the sorted runs)
SEED_HD void seed_better(uint32_t& bl, int64_t& bv, uint32_t l, int64_t v) {
  if (l > bl || (l == bl && l != 0 && v < bv)) { bl = l; bv = v; }
}
// findMaxFreq over slots lo, lo + step, ... of a table: folded into (bl, bv), which start at (0, 0)
template <class Mem>
SEED_HD void seed_table_best(const SeedSlot* tab, uint64_t capacity, uint64_t lo, uint64_t step, uint32_t& bl, int64_t& bv) {
  for (uint64_t i = lo; i < capacity; i += step) {
    const int64_t v = Mem::load(&tab[i].value);
    if (v != kSeedSlotEmpty) seed_better(bl, bv, Mem::load(&tab[i].count), v);
  }
}

// the reverse complement of a k-mer code (two bits per letter, first letter in the highest pair): GenomeIndex::revcomp_code
SEED_HD uint64_t seed_revcomp(uint64_t x, uint32_t k) {
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
  x = ((x >> 8) & 0x00ff00ff00ff00ffull) | ((x & 0x00ff00ff00ff00ffull) << 8);
  x = ((x >> 16) & 0x0000ffff0000ffffull) | ((x & 0x0000ffff0000ffffull) << 16);
  x = (x >> 32) | (x << 32);
  return (~x) >> (64 - 2 * k);
}

// 0..3 for A C G T, 4 for N, 5 for anything else
SEED_HD uint32_t seed_letter(uint8_t c) {
  switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    case 'N': return 4;
    default: return 5;
  }
}

// reverseComplement's table (sage_out.hpp): 0 = a letter outside ACGTNacgtn, whose output position keeps its ORIGINAL byte
SEED_HD uint8_t seed_complement(uint8_t c) {
  switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    case 'N': case 'n': return 'N';
    default: return 0;
  }
}

// The window of an anchored trace (getReferenceSlice after the votes, seed.hpp:721-736): contig `ref` of the hit (the cumulative
// length + 1 walk, found by bisection over cum), window start `pos` in the contig, text range [src, src + len) of the window (the
// TextView::substr clamp included).
struct SeedWindow {
  uint32_t ref, pos;
  uint64_t src, len;
};
SEED_HD SeedWindow seed_window(const int64_t* cum, const uint64_t* starts, const uint32_t* lengths, uint32_t nc, uint64_t text_len,
                               int64_t bestPos, uint32_t S, uint16_t maxindel) {
  uint32_t lo = 0, hi = nc - 1;  // the last contig r with r == 0 or bestPos >= cum[r]
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (bestPos >= cum[mid]) lo = mid;
    else hi = mid - 1;
  }
  SeedWindow w;
  w.ref = lo;
  const uint32_t seqlen = lengths[lo] + 1;
  const int64_t chrposSigned = bestPos - cum[lo];
  const uint32_t chrpos = chrposSigned > 0 ? (uint32_t)chrposSigned : 0;
  uint32_t slicestart = 0, sliceend = seqlen;
  if (chrpos > maxindel) slicestart = chrpos - maxindel;
  const uint32_t tmpend = chrpos + S + maxindel;
  if (tmpend < seqlen) sliceend = tmpend;
  w.pos = slicestart;
  const int64_t lastc = (int64_t)lengths[lo] - 1;
  const int64_t last = (int64_t)sliceend < lastc ? (int64_t)sliceend : lastc;
  w.src = 0;
  w.len = 0;
  if ((int64_t)slicestart <= last) {
    uint64_t p = starts[lo] + slicestart;
    if (p > text_len) p = text_len;
    const uint64_t want = (uint64_t)(last - slicestart + 1);
    w.src = p;
    w.len = want < text_len - p ? want : text_len - p;
  }
  return w;
}

// The host-side check of an index descriptor (tracyhip_genome_validate): nothing out of range may reach a kernel as an index.
inline int seed_validate(const tracyhip_genome_desc* d, char* why, size_t cap) {
  auto fail = [&](const char* m) { std::snprintf(why, cap, "%s", m); return TRACYHIP_ERR_ARG; };
  if (!d) return fail("null genome descriptor");
  if (d->k < 1 || d->k > 32) return fail("k must be 1 .. 32");
  if (d->bucket_bits > 24 || d->bucket_bits > 2 * d->k) return fail("bucket_bits must be <= min(2k, 24)");
  if (!d->dir || (d->ntab && !d->tab) || !d->text || !d->starts || !d->lengths) return fail("null array in the genome descriptor");
  if (d->ncontigs < 1) return fail("a genome needs at least one contig");
  const uint64_t nb = 1ull << d->bucket_bits;
  if (d->dir[0] != 0) return fail("directory does not start at 0");
  for (uint64_t b = 0; b < nb; ++b)
    if (d->dir[b] > d->dir[b + 1]) return fail("directory is not monotone");
  if (d->dir[nb] != d->ntab) return fail("last directory entry is not ntab");
  uint64_t end = 0;
  for (uint32_t i = 0; i < d->ncontigs; ++i) {
    if (d->starts[i] < end || d->starts[i] > d->text_len || d->lengths[i] > d->text_len - d->starts[i])
      return fail("contig outside the text (or out of order)");
    end = d->starts[i] + d->lengths[i];
    if (d->contig_id && d->contig_id[i] >= d->ncontigs) return fail("contig_id out of range");
  }
  return TRACYHIP_OK;
}

// The host-side check of a descriptor a table is to be BUILT from (tracyhip_genome_validate_text): the k / bucket_bits and contig rules of
// seed_validate, no directory or table given.
inline int seed_validate_text(const tracyhip_genome_desc* d, char* why, size_t cap) {
  auto fail = [&](const char* m) { std::snprintf(why, cap, "%s", m); return TRACYHIP_ERR_ARG; };
  if (!d) return fail("null genome descriptor");
  if (d->k < 1 || d->k > 32) return fail("k must be 1 .. 32");
  if (d->bucket_bits > 24 || d->bucket_bits > 2 * d->k) return fail("bucket_bits must be <= min(2k, 24)");
  if (d->dir || d->tab || d->ntab) return fail("dir, tab and ntab must be NULL / 0: the table is built");
  if (!d->text || !d->starts || !d->lengths) return fail("null array in the genome descriptor");
  if (d->ncontigs < 1) return fail("a genome needs at least one contig");
  uint64_t end = 0;
  for (uint32_t i = 0; i < d->ncontigs; ++i) {
    if (d->starts[i] < end || d->starts[i] > d->text_len || d->lengths[i] > d->text_len - d->starts[i])
      return fail("contig outside the text (or out of order)");
    end = d->starts[i] + d->lengths[i];
    if (d->contig_id && d->contig_id[i] >= d->ncontigs) return fail("contig_id out of range");
  }
  return TRACYHIP_OK;
}

}  // namespace tracyhip
#endif
