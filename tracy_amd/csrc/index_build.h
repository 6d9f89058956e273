// index_build.h -- GenomeIndex::build (tracy_amd/host/seed.hpp) on the device: the bucket directory and the sorted k-mer table of a
// genome text, word for word the host's (tracyhip_genome_build, index_build.hip).
//
// The order the host fixes (seed.hpp build + sort_table): every window of k letters from ACGT is filed under the smaller of its code and
// its reverse complement's (bit 63 of pos set when the reverse complement was the smaller; a palindrome is never flipped); the table is
// sorted by bucket (the low bucket_bits bits of that code), code, then the whole 64-bit pos; dir[b] is bucket b's first table index and
// dir[2^bucket_bits] = ntab.  pos is unique, so any correct sort gives the same bytes.
#ifndef TRACY_AMD_INDEX_BUILD_H
#define TRACY_AMD_INDEX_BUILD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tracyhip {

constexpr uint32_t kIbThreads = 256;               // key passes: one workgroup per tile of the text
constexpr uint32_t kIbPer = 16;                    // consecutive windows per thread (a rolling code, one atomic per run of one bucket)
constexpr uint32_t kIbTile = kIbThreads * kIbPer;  // windows per workgroup; the tile holds them + a (k - 1)-byte halo
constexpr uint32_t kIbSmall = 16;                  // buckets of up to this many entries: sorted by one thread in registers
constexpr uint32_t kIbChunk = 1024;                // longer ones: sorted in LDS by one wave, in chunks of this many entries, then merged

// The pipeline, all on `st` (kernel boundaries are the only hand-offs between workgroups):
//   1. count: per bucket, its valid windows (LDS tile of the text, rolling codes, atomic adds into a 2^bits histogram);
//   2. dir = exclusive scan of the histogram (so dir comes out of the sort itself); ntab = dir[2^bits];
//   3. scatter: every entry to its bucket's next free index (the histogram pass again, with a cursor copied from dir);
//   4. sort every bucket by (code, pos): <= kIbSmall entries in registers, <= kIbChunk in LDS, longer ones in LDS chunks + merge passes.
// dir: caller-owned device array of 2^bits + 1 words.  *tab: allocated here (2 * max(ntab, 1) words, {code, pos} pairs) and owned by the
// caller on success.  Temporaries are freed before the call returns; on any failure nothing stays allocated and *tab is NULL.
hipError_t index_build(hipStream_t st, const uint8_t* text, uint64_t text_len, uint32_t k, uint32_t bits, uint64_t* dir, uint64_t** tab,
                       uint64_t* ntab);

}  // namespace tracyhip
#endif
