// assemble_wave.h -- the three row-block primitives of `tracy assemble` on ONE wave, bit-identical with tracy_amd/host/msa.hpp:
//   msa_merge      the row merge along an op string       assemble.h:266-284 (one block new) / msa.h:121-150 (both blocks; msa.hpp:213-231)
//   msa_profile    _createProfile(char MSA)               align.h:138-180 (msa.hpp createProfile)
//   msa_consensus  consensus()                            msa.h:165-254   (msa.hpp consensus)
// and msa_span, the first / last non-gap column of a row, which the other two read.
//
// A row block is n rows x c columns of bytes, packed row by row.  All four bodies walk the columns in rounds of 64, one column per
// lane: every read and write of a row is one coalesced 64-byte access.  Positions that depend on the columns before (the source
// column of a merge, the output slot of a called consensus letter) are prefix counts of ballots, as in consensus_kernel.
//
// Floating point: the only float operation is the division cnt[k] / sum of msa_profile -- one correctly rounded fp32 division of two
// small integers (the library is built without fast-math and with -ffp-contract=off, stated again by the pragma; hipcc's default is
// the correctly rounded divide).  Everything else is integer arithmetic.
//
// W: the wave abstraction of decompose_wave.h (lane, ballot); tests/emu/emu_assemble.cpp runs the same bodies on the 64-fiber host wave.
#ifndef TRACY_AMD_ASSEMBLE_WAVE_H
#define TRACY_AMD_ASSEMBLE_WAVE_H

#include <cstdint>

#include "dp_lane.h"  // TR_HD

namespace tracyhip {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// one side of a merge: a block of n character rows, or (rows == null) ONE input profile that stands for its _profileConsChar row
struct MsaSide {
  const uint8_t* rows;  // n x c bytes, packed
  const float* prof;    // element (k, j) at k * stride + j
  uint32_t n, c, stride;
};

// _profileConsChar (align.h:254-270): the first maximum over k = 0 .. 5; never '-' (it would create gap-to-gap columns)
TR_HD uint8_t msa_cons_char(const float* p, uint64_t stride, uint32_t j) {
  uint32_t maxidx = 0;
  float maxval = p[j];
  for (uint32_t k = 1; k < 6; ++k) {
    const float v = p[k * stride + j];
    if (v > maxval) { maxval = v; maxidx = k; }
  }
  return (uint8_t)("ACGTNN"[maxidx]);
}

TR_HD uint32_t msa_popc(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

// first / last non-gap column of one row (both -1: the row holds gaps only) -> span[0], span[1]
template <class W>
TR_HD void msa_span_wave(W& w, const uint8_t* row, uint32_t ncol, int32_t* span) {
  const uint32_t lane = w.lane();
  int32_t first = -1, last = -1;
  for (uint32_t b = 0; b < ncol; b += 64) {
    const uint32_t j = b + lane;
    const uint64_t t = w.ballot(j < ncol && row[j] != '-');
    if (t) {
      if (first < 0) first = (int32_t)(b + (uint32_t)__builtin_ctzll(t));
      last = (int32_t)(b + 63u - (uint32_t)__builtin_clzll(t));
    }
  }
  if (lane == 0) { span[0] = first; span[1] = last; }
}

// numAligned of the overlap test of de novo assembly (assemble.h:436-439): the columns of an alignment that hold a character on both
// sides, which are the 's' ops of its op string (either order).  Every lane returns the count.
template <class W>
TR_HD uint32_t msa_count_aligned_wave(W& w, const uint8_t* ops, uint32_t L) {
  const uint32_t lane = w.lane();
  uint32_t n = 0;
  for (uint32_t b = 0; b < L; b += 64) {
    const uint32_t j = b + lane;
    n += msa_popc(w.ballot(j < L && ops[j] == 's'));
  }
  return n;
}

// One row of a merged block.  ops: the op string in the reference's PUSH order (the end of the alignment first, as
// tracyhip_gotoh_align writes it), L of them; column j of the result belongs to ops[L - 1 - j].  The row comes from the LEFT block
// (column taken unless the op is 'h') or the right one (unless 'v'); a skipped column is '-'.  The source column is the number of
// taken columns before j.  span (or null) receives what msa_span_wave would find in the row written.
template <class W>
TR_HD void msa_merge_row_wave(W& w, const uint8_t* ops, uint32_t L, const MsaSide& s, uint32_t src_row, bool left, uint8_t* out, int32_t* span) {
  const uint32_t lane = w.lane();
  const uint64_t below = (1ull << lane) - 1ull;
  const uint8_t skip = left ? 'h' : 'v';
  uint32_t at = 0;
  int32_t first = -1, last = -1;
  for (uint32_t b = 0; b < L; b += 64) {
    const uint32_t j = b + lane;
    const bool take = j < L && ops[L - 1u - j] != skip;
    const uint64_t t = w.ballot(take);
    const uint32_t pos = at + msa_popc(t & below);
    uint8_t ch = '-';
    if (take && pos < s.c) ch = s.rows ? s.rows[(uint64_t)src_row * s.c + pos] : msa_cons_char(s.prof, s.stride, pos);
    if (j < L) out[j] = ch;
    const uint64_t g = w.ballot(ch != '-');
    if (g) {
      if (first < 0) first = (int32_t)(b + (uint32_t)__builtin_ctzll(g));
      last = (int32_t)(b + 63u - (uint32_t)__builtin_clzll(g));
    }
    at += msa_popc(t);
  }
  if (span && lane == 0) { span[0] = first; span[1] = last; }
}

// _createProfile(char MSA) for the 64 columns from b on: prof(k, j) at prof[k * ncol + j].  A row counts in column j between its
// first and last non-gap character (a row of gaps only: everywhere); '-' inside the span counts in row 5; a byte outside
// ACGTNacgtn- is dropped from the column's sum; the value is cnt[k] / sum, or cnt[k] when the sum is 0.  span: 2 per row (msa_span_wave).
template <class W>
TR_HD void msa_profile_wave(W& w, const uint8_t* rows, uint32_t nrows, uint32_t ncol, const int32_t* span, uint32_t b, float* prof) {
  const uint32_t j = b + w.lane();
  if (j >= ncol) return;
  int32_t sum = 0;
  float cnt[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t i = 0; i < nrows; ++i) {
    const int32_t first = span[2 * i], last = span[2 * i + 1];
    if (first >= 0 && ((int32_t)j < first || (int32_t)j > last)) continue;
    ++sum;
    switch (rows[(uint64_t)i * ncol + j]) {
      case 'A': case 'a': cnt[0] += 1; break;
      case 'C': case 'c': cnt[1] += 1; break;
      case 'G': case 'g': cnt[2] += 1; break;
      case 'T': case 't': cnt[3] += 1; break;
      case 'N': case 'n': cnt[4] += 1; break;
      case '-': cnt[5] += 1; break;
      default: --sum; break;
    }
  }
  const float fsum = (float)sum;
  for (uint32_t k = 0; k < 6; ++k) prof[(uint64_t)k * ncol + j] = sum > 0 ? cnt[k] / fsum : cnt[k];
}

// consensus() over the first `rows` rows of a block (the caller leaves the last one out with ignoreLast).  A row covers the columns
// of its span; a column with coverage >= 1 and >= cov_threshold takes the majority among A, C, G, T and "other" (first maximum);
// "other" calls nothing.  The host carries `qualval` from column to column, but a column that emits a letter has just set it: the
// quality of a called column is always its own 47 + maxCount * 10 / rows.  gapped: ncol bytes; cons / qual: the called columns
// packed; cons_len: their number.
template <class W>
TR_HD void msa_consensus_wave(W& w, const uint8_t* rows_p, uint32_t rows, uint32_t ncol, const int32_t* span, int32_t cov_threshold, uint8_t* gapped,
                              uint8_t* cons, uint8_t* qual, uint32_t* cons_len) {
  const uint32_t lane = w.lane();
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t slot = 0;
  for (uint32_t b = 0; b < ncol; b += 64) {
    const uint32_t j = b + lane;
    bool called = false;
    uint8_t letter = '-', q = '#';
    if (j < ncol) {
      int32_t cov = 0;
      int32_t count[5] = {0, 0, 0, 0, 0};
      for (uint32_t i = 0; i < rows; ++i) {
        const int32_t first = span[2 * i], last = span[2 * i + 1];
        if (first < 0 || (int32_t)j < first || (int32_t)j > last) continue;
        ++cov;
        switch (rows_p[(uint64_t)i * ncol + j]) {
          case 'A': case 'a': ++count[0]; break;
          case 'C': case 'c': ++count[1]; break;
          case 'G': case 'g': ++count[2]; break;
          case 'T': case 't': ++count[3]; break;
          default: ++count[4]; break;
        }
      }
      if (cov >= 1 && cov >= cov_threshold) {
        int32_t max_idx = 0, max_count = count[0];
        for (int k = 1; k < 5; ++k)
          if (count[k] > max_count) { max_count = count[k]; max_idx = k; }
        if (max_idx < 4) {
          called = true;
          letter = (uint8_t)("ACGT"[max_idx]);
          q = (uint8_t)(47 + max_count * 10 / (int32_t)rows);
        }
      }
      gapped[j] = letter;
    }
    const uint64_t t = w.ballot(called);
    if (called) {
      const uint32_t o = slot + msa_popc(t & below);
      cons[o] = letter;
      qual[o] = q;
    }
    slot += msa_popc(t);
  }
  if (lane == 0) *cons_len = slot;
}

}  // namespace tracyhip
#endif
