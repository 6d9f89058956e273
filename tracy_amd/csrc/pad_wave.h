// pad_wave.h -- trimTrace(tr, bc, l, r, nbc) + reverseComplementTrace() + alignmentTracePadding() of ONE trace on ONE wave
// (trim.h:77-99, 102-150; json.h:383-472), equal in every field to tracy_amd/host/assemble_out.hpp and sage_out.hpp.
//
// What the reference does, one push_back at a time (sage_out.hpp alignmentTracePadding):
//     step = bcPos.size() > 1 ? (uint32)(sum of neighbour differences as double / (size - 1)) : 6
//     for ch in row: a run of g gaps that ends before letter p >= 1 is an insert (at = (uint32)((b[p-1] + b[p]) / 2.0), g);
//                    a run before letter 0 is leadingGaps, a run behind the last letter trailingGaps
//     for x in [0, ns): push sample x of the four channels;
//                       if x == at[ins]:  g times { push pseudo call '-' of quality 0 at x + offset + (uint32)(step / 2.0);
//                                                   step times { push -99 to the four channels; ++offset } }, next insert
//                       if x == b[call]:  push the call at b[call] + offset, next call
// in front of it the hard trim keeps the calls [l, n - r) (positions unchanged), and the reverse complement mirrors the samples
// (x -> ns - 1 - x, channel k -> 3 - k), reverses the calls (bcPos -> ns - 1 - bcPos) and complements their letters.
//
// The closed forms this file computes instead.  b[0 .. m): the kept calls after trim and reverse, strictly increasing inside [0, ns):
//     step = m > 1 ? (b[m-1] - b[0]) / (m - 1) : 6      the double sum telescopes and the quotient of ints below 2^23 by ints below 2^17,
//                                                       correctly rounded, cannot reach an integer it does not reach exactly, so the
//                                                       truncation is the integer division;  (uint32)(step / 2.0) = step >> 1
//     insert i = (q, g) with q = (b[p-1] + b[p]) >> 1 for the run of g gaps that ends before letter p >= 1;  q is strictly increasing in p
//     Gex(i) / Ginc(i) = sum of g over the inserts before i / up to and including i
//     source sample x lands at x + step * G<(x), G<(x) = sum of g over inserts with q < x; the step * g samples behind source sample q
//     are -99: insert i is the output samples [E, F) with E = q + 1 + step * Gex(i), F = q + 1 + step * Ginc(i)
//     ns' = ns + step * sum g,  m' = m + sum g
//     call c goes to bcPos' = b[c] + step * G<=(c), G<=(c) = sum of g over inserts with q <= b[c], behind all those pseudo calls:
//     output index c + G<=(c).  The <= matters: with b[p] = b[p-1] + 1 the insert sits AT sample b[p-1] and is emitted before the call of
//     that sample (row A--C, positions [5, 6]: bcPos' [5, 6, 7, 8], primary' "--AC"; positions [5, 8]: [5, 7, 10, 14], "A--C")
//     pseudo call j of insert i goes to bcPos' = q + step * Gex(i) + j * step + (step >> 1), output index cb(i) + Gex(i) + j with
//     cb(i) = the calls emitted before it = p - 1 when b[p-1] == q, else p
//
// Data flow.  Pass A scans the row 64 columns at a time: gap-run ends from a ballot and the run length carried across steps, the letter
// index from the ballot of the letters below, the running sum of g from excl_sum; the inserts (q, Gex, Ginc, cb) go to a scratch region
// of the trace that this wave alone writes and reads.  No trimmed or reversed array exists: PadMap maps a kept call to its entry of
// the caller's arrays and to its position.  The sizes-only form ends here.  Pass B takes 64 calls at a time, pass C 64 x kPadVec OUTPUT samples at
// a time; both need "how many inserts have a key <= v" for keys that grow along the pass (q for the calls, E for the samples), so the
// insert list is staged through the wave's LDS in tiles of kPadTile entries that move forward with the pass (pad_search).  Every output
// element is written exactly once: calls by the lane that owns the call, pseudo calls by the lane that owns the insert, samples by the
// lane that owns the output index (either -99 or the one source sample y - step * G, mirrored with `reverse`); a lane's kPadVec samples
// of a channel leave as one 16-byte (int32) or 8-byte (int16) store where they are aligned.  No atomics.
//
// Answered: bc_len in 1 .. kPadMaxCalls, nsamples in 1 .. kPadMaxSamples, every position (trimmed ones included) strictly increasing
// inside [0, nsamples), l + r < bc_len, letters of the row <= kept calls, ns' and m' below 2^31.  Anything else is DEFERRED: status and
// zero sizes are written, nothing else.  The reference stalls on an equal neighbour, reads bcPos[0] of an empty set, wraps for r > n and
// indexes bcPos past its end for a row with more letters than calls.  All positions are checked before the first read that depends on one.
//
// W: the wave abstraction of decompose_wave.h / basecall_wave.h (lane, ballot, bcast, sum, excl_sum, sync, lds).
#ifndef TRACY_AMD_PAD_WAVE_H
#define TRACY_AMD_PAD_WAVE_H

#include <cstdint>

#include "dp_lane.h"  // TR_HD

namespace tracyhip {

constexpr int32_t kPadStatusOk = 0, kPadStatusDeferred = 1, kPadStatusTooSmall = 2;  // TRACYHIP_PAD_*
constexpr uint32_t kPadMaxCalls = 131071;         // the decompose limit, as basecalling
constexpr uint32_t kPadMaxSamples = 1u << 23;
constexpr int32_t kPadEmpty = -99;                // EMPTY_TRACE_SIGNAL, json.h:12-14
constexpr uint32_t kPadTile = 256;                // inserts per LDS tile
constexpr uint32_t kPadVec = 4;                   // output samples per lane and step
constexpr uint32_t kPadLdsBytes = 3 * kPadTile * 4;  // per wave: key, Ginc, q of a tile
constexpr uint32_t kPadInsWords = 4;              // scratch words per insert: q, Gex, Ginc, cb

struct PadTrace {  // per trace, built by the host from the job's and the result's HOST arrays
  uint64_t sig_off;       // elements
  uint64_t bc_off;        // elements: the five basecall arrays
  uint64_t row_off;       // bytes
  uint64_t scratch_off;   // words: kPadInsWords * pad_max_inserts()
  uint64_t out_sig_off;   // elements
  uint64_t out_call_off;  // elements
  uint32_t nsamples, bc_len, row_len;
  uint32_t trim_l, trim_r, reverse;
  uint32_t sample_cap, call_cap;
};
struct PadOut {
  int32_t status;
  uint32_t nsamples_out, ncalls_out, leading, trailing, step;
};
struct PadArgs {
  const void* signal;  // int32 or int16 samples; null in the sizes-only form
  const int32_t* bcpos;
  const uint8_t *primary, *secondary, *consensus, *estqual;  // each needed only where its result is wanted
  const uint8_t* rows;
  const PadTrace* tr;
  PadOut* out;
  uint32_t* scratch;   // null in the sizes-only form
  void* o_signal;      // payload results, each may be null
  int32_t* o_bcpos;
  uint8_t *o_primary, *o_secondary, *o_consensus, *o_estqual;
  uint32_t ntraces;
};

// what the host can tell from its own arrays (it sizes the scratch region by it; the wave checks the same first)
TR_HD bool pad_sizes_answerable(uint32_t ns, uint32_t n, uint32_t l, uint32_t r) {
  return n >= 1 && n <= kPadMaxCalls && ns >= 1 && ns <= kPadMaxSamples && (uint64_t)l + r < n;
}
// an insert takes a gap and the letter behind it, and sits before one of the letters 1 .. m - 1
TR_HD uint32_t pad_max_inserts(uint32_t m, uint32_t row_len) { return m - 1 < row_len / 2 ? m - 1 : row_len / 2; }

TR_HD uint8_t pad_complement(uint8_t c) {  // reverseComplement(char), trim.h:102-123
  switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'N': return 'N';
    case 'H': return 'D'; case 'V': return 'B'; case 'M': return 'K'; case 'Y': return 'R'; case 'D': return 'H';
    case 'B': return 'V'; case 'K': return 'M'; case 'R': return 'Y'; case 'U': return 'A'; case 'S': return 'S'; case 'W': return 'W';
    default: return c;
  }
}

struct PadMap {  // kept call c of the trimmed, reversed trace -> entry of the caller's arrays, and its position
  uint32_t n, l, r, ns;
  bool rev;
  TR_HD uint32_t index(uint32_t c) const { return rev ? n - r - 1 - c : l + c; }
  TR_HD int32_t b(const int32_t* pos, uint32_t c) const { return rev ? (int32_t)ns - 1 - pos[index(c)] : pos[index(c)]; }
};

// The moving tile of the insert list.  cnt = inserts whose key is <= v, with Ginc and q of insert cnt - 1 (0, 0 for none); keys grow with
// the insert index and a pass asks for values that do not fall from one step to the next, so the tiles only move forward: [0, kdone) are
// known to be <= every v of this step, gdone / qdone belong to insert kdone - 1.  key(i) = q (samples == false) or E (samples == true).
// Every lane of the wave calls this (lanes with valid == false take no part in the search but pass the same barriers).
struct PadList {
  const uint32_t* ins;  // kPadInsWords per insert
  uint32_t nins, step;
  uint32_t kdone, gdone, qdone;
  uint32_t tile_start, tile_n;  // the inserts the LDS tile holds (tile_n == 0: none; a pass with other keys starts so)
};
template <bool SAMPLES>
TR_HD uint32_t pad_key(const uint32_t* e, uint32_t step) { return SAMPLES ? e[0] + 1 + step * e[1] : e[0]; }

template <bool SAMPLES, class W>
TR_HD void pad_search(W& w, PadList& L, bool valid, uint32_t v, uint32_t& cnt, uint32_t& G, uint32_t& q) {
  uint32_t* tk = reinterpret_cast<uint32_t*>(w.lds());
  uint32_t* tg = tk + kPadTile;
  uint32_t* tq = tg + kPadTile;
  const uint32_t lane = w.lane();
  cnt = L.kdone; G = L.gdone; q = L.qdone;
  bool active = valid;
  // the tile of the step before serves as long as the first insert in question is in it
  bool have = L.tile_n != 0 && L.kdone >= L.tile_start && L.kdone - L.tile_start < L.tile_n;
  uint32_t start = have ? L.tile_start : L.kdone;
  for (;;) {  // (every condition that leaves or steers the loop is the same in all lanes)
    uint32_t tn = L.tile_n;
    if (!have) {
      tn = L.nins - start < kPadTile ? L.nins - start : kPadTile;
      if (tn == 0) break;
      w.sync();  // (the previous tile has been read)
      for (uint32_t i = lane; i < tn; i += 64) {
        const uint32_t* e = L.ins + (uint64_t)kPadInsWords * (start + i);
        tk[i] = pad_key<SAMPLES>(e, L.step); tg[i] = e[2]; tq[i] = e[0];
      }
      w.sync();
      L.tile_start = start; L.tile_n = tn;
    }
    have = false;
    if (active) {
      uint32_t lo = 0, hi = tn;  // first entry of the tile whose key is > v
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tk[mid] <= v) lo = mid + 1; else hi = mid;
      }
      if (lo) { cnt = start + lo; G = tg[lo - 1]; q = tq[lo - 1]; }
      if (lo < tn) active = false;
    }
    if (w.ballot(active) == 0) break;
    start += tn;
  }
  // the next step starts where this step's last lane ended (a lane without a value took the start values)
  const uint32_t c63 = w.bcast(cnt, 63), g63 = w.bcast(G, 63), q63 = w.bcast(q, 63);
  L.kdone = c63; L.gdone = g63; L.qdone = q63;
}
// the same answer for one value without the tile: a binary search of the whole list in memory (a lane whose samples straddle an insert)
TR_HD void pad_search_slow(const PadList& L, uint32_t v, uint32_t& cnt, uint32_t& G, uint32_t& q) {
  uint32_t lo = 0, hi = L.nins;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (pad_key<true>(L.ins + (uint64_t)kPadInsWords * mid, L.step) <= v) lo = mid + 1; else hi = mid;
  }
  cnt = lo; G = 0; q = 0;
  if (lo) { const uint32_t* e = L.ins + (uint64_t)kPadInsWords * (lo - 1); G = e[2]; q = e[0]; }
}

template <bool S16>
TR_HD int32_t pad_load(const void* sig, uint64_t idx) {
  return S16 ? (int32_t) static_cast<const int16_t*>(sig)[idx] : static_cast<const int32_t*>(sig)[idx];
}
// kPadVec samples of one channel from element `at` on: one wide store (the caller has checked the alignment)
struct alignas(16) PadQuad32 { int32_t v[4]; };
struct alignas(8) PadQuad16 { int16_t v[4]; };
template <bool S16>
TR_HD void pad_store_vec(void* out, uint64_t at, const int32_t (&v)[kPadVec]) {
  if (S16) {
    PadQuad16 p;
    for (uint32_t j = 0; j < kPadVec; ++j) p.v[j] = (int16_t)v[j];
    *reinterpret_cast<PadQuad16*>(static_cast<int16_t*>(out) + at) = p;
  } else {
    PadQuad32 p;
    for (uint32_t j = 0; j < kPadVec; ++j) p.v[j] = v[j];
    *reinterpret_cast<PadQuad32*>(static_cast<int32_t*>(out) + at) = p;
  }
}
template <bool S16>
TR_HD void pad_store_one(void* out, uint64_t at, int32_t v) {
  if (S16) static_cast<int16_t*>(out)[at] = (int16_t)v;
  else static_cast<int32_t*>(out)[at] = v;
}

template <bool S16, class W>
TR_HD void pad_wave_body(W& w, const PadArgs& a, uint32_t t) {
  const uint32_t lane = w.lane();
  const PadTrace tr = a.tr[t];
  const uint32_t n = tr.bc_len, ns = tr.nsamples;
  const int32_t* pos = a.bcpos + tr.bc_off;
  const uint8_t* row = a.rows + tr.row_off;
  auto defer = [&]() {
    if (lane == 0) a.out[t] = PadOut{kPadStatusDeferred, 0, 0, 0, 0, 0};
  };

  // ---- every position checked before anything depends on one ----
  if (!pad_sizes_answerable(ns, n, tr.trim_l, tr.trim_r)) { defer(); return; }  // (the whole wave)
  bool bad = false;
  for (uint32_t i0 = 0; i0 < n; i0 += 64) {
    const uint32_t i = i0 + lane;
    if (i < n) {
      const int32_t cur = pos[i];
      if (cur < 0 || (uint32_t)cur >= ns || (i && cur <= pos[i - 1])) bad = true;
    }
  }
  if (w.ballot(bad) != 0) { defer(); return; }

  const PadMap map{n, tr.trim_l, tr.trim_r, ns, tr.reverse != 0};
  const uint32_t m = n - tr.trim_l - tr.trim_r;
  const uint32_t step = m > 1 ? (uint32_t)(map.b(pos, m - 1) - map.b(pos, 0)) / (m - 1) : 6u;
  uint32_t* ins = a.scratch ? a.scratch + tr.scratch_off : nullptr;

  // ---- pass A: the row, 64 columns at a time ----
  uint32_t letters = 0;  // letters before this step
  uint32_t run = 0;      // gaps that end the columns before this step
  uint32_t nins = 0, gsum = 0, leading = 0;
  bool wide = false;     // a sum that leaves 32 bits
  for (uint32_t j0 = 0; j0 < tr.row_len; j0 += 64) {
    const uint32_t j = j0 + lane;
    const bool in = j < tr.row_len;
    const bool gap = in && row[j] == '-';
    const uint64_t gm = w.ballot(gap), lm = w.ballot(in && !gap);
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const uint32_t p = letters + (uint32_t)__builtin_popcountll(lm & below);  // index of this column's letter
    // a letter with a gap before it ends a run
    uint32_t g = 0;
    if (in && !gap) {
      const uint64_t lb = lm & below;  // letters below this lane
      if (lb) g = lane - (64 - (uint32_t)__builtin_clzll(lb));  // gaps since the nearest one
      else g = lane + run;
    }
    const bool ends = g != 0;
    if (ends && p == 0) leading = g;
    const bool is_ins = ends && p >= 1;
    if (is_ins && p >= m) bad = true;  // more letters than calls (checked again for the row as a whole below)
    const bool wr = is_ins && !bad;
    const uint64_t im = w.ballot(wr);
    const uint32_t gex = gsum + w.excl_sum(wr ? g : 0u);
    if (wr && ins) {
      const int32_t b0 = map.b(pos, p - 1), b1 = map.b(pos, p);
      const uint32_t q = (uint32_t)(b0 + b1) >> 1;
      uint32_t* e = ins + (uint64_t)kPadInsWords * (nins + (uint32_t)__builtin_popcountll(im & below));
      e[0] = q; e[1] = gex; e[2] = gex + g; e[3] = (uint32_t)b0 == q ? p - 1 : p;
    }
    const uint32_t add = w.sum(wr ? g : 0u);
    if (add > 0xffffffffu - gsum) wide = true;
    gsum += add;
    nins += (uint32_t)__builtin_popcountll(im);
    letters += (uint32_t)__builtin_popcountll(lm);
    // the run that ends this step
    const uint32_t cols = tr.row_len - j0 < 64 ? tr.row_len - j0 : 64;
    if (lm == 0) run += cols;
    else run = cols - (64 - (uint32_t)__builtin_clzll(lm));
  }
  const uint32_t trailing = run;
  leading = w.umax(leading);  // (one lane of one step saw it)
  if (letters > m) bad = true;
  const uint64_t ns_out64 = (uint64_t)ns + (uint64_t)step * gsum, nc_out64 = (uint64_t)m + gsum;
  if (wide || ns_out64 > 0x7fffffffull || nc_out64 > 0x7fffffffull) bad = true;
  if (w.ballot(bad) != 0) { defer(); return; }
  const uint32_t ns_out = (uint32_t)ns_out64, nc_out = (uint32_t)nc_out64;

  const bool want_calls = a.o_bcpos || a.o_primary || a.o_secondary || a.o_consensus || a.o_estqual;
  const bool want_samples = a.o_signal != nullptr;
  const bool small = (want_samples && ns_out > tr.sample_cap) || (want_calls && nc_out > tr.call_cap);
  if (lane == 0) a.out[t] = PadOut{small ? kPadStatusTooSmall : kPadStatusOk, ns_out, nc_out, leading, trailing, step};
  if (small || !ins || (!want_calls && !want_samples)) return;
  w.sync_global();  // the inserts are in memory for every lane

  PadList L{ins, nins, step, 0, 0, 0, 0, 0};
  // ---- pass B: the calls, 64 at a time, and the pseudo calls of every insert ----
  if (want_calls) {
    const uint64_t ob = tr.out_call_off;
    const uint8_t *pri = a.primary ? a.primary + tr.bc_off : nullptr, *sec = a.secondary ? a.secondary + tr.bc_off : nullptr,
                  *con = a.consensus ? a.consensus + tr.bc_off : nullptr, *eq = a.estqual ? a.estqual + tr.bc_off : nullptr;
    for (uint32_t c0 = 0; c0 < m; c0 += 64) {
      const uint32_t c = c0 + lane;
      const bool valid = c < m;
      const int32_t b = valid ? map.b(pos, c) : 0;
      uint32_t cnt, G, q;
      pad_search<false>(w, L, valid, (uint32_t)b, cnt, G, q);
      if (!valid) continue;
      const uint32_t src = map.index(c);
      const uint64_t o = ob + c + G;
      if (a.o_bcpos) a.o_bcpos[o] = (int32_t)((uint32_t)b + step * G);
      if (a.o_primary) a.o_primary[o] = map.rev ? pad_complement(pri[src]) : pri[src];
      if (a.o_secondary) a.o_secondary[o] = map.rev ? pad_complement(sec[src]) : sec[src];
      if (a.o_consensus) a.o_consensus[o] = map.rev ? pad_complement(con[src]) : con[src];
      if (a.o_estqual) a.o_estqual[o] = eq[src];
    }
    for (uint32_t i = lane; i < nins; i += 64) {
      const uint32_t* e = ins + (uint64_t)kPadInsWords * i;
      const uint32_t q = e[0], gex = e[1], g = e[2] - e[1];
      uint64_t o = ob + e[3] + gex;
      uint32_t at = q + step * gex + (step >> 1);
      for (uint32_t k = 0; k < g; ++k, ++o, at += step) {
        if (a.o_bcpos) a.o_bcpos[o] = (int32_t)at;
        if (a.o_primary) a.o_primary[o] = '-';
        if (a.o_secondary) a.o_secondary[o] = '-';
        if (a.o_consensus) a.o_consensus[o] = '-';
        if (a.o_estqual) a.o_estqual[o] = 0;
      }
    }
  }

  // ---- pass C: the OUTPUT samples, 64 x kPadVec at a time ----
  if (want_samples) {
    L.kdone = L.gdone = L.qdone = L.tile_n = 0;
    const uint64_t so = tr.out_sig_off;
    // channel k's element (so + k * ns_out + y) is aligned for a wide store where y = shift[k] (mod kPadVec)
    uint32_t shift[4];
    for (uint32_t k = 0; k < 4; ++k) shift[k] = (uint32_t)((so + (uint64_t)k * ns_out) % kPadVec);
    const bool base_ok = reinterpret_cast<uintptr_t>(a.o_signal) % (kPadVec * (S16 ? 2 : 4)) == 0;
    auto sample = [&](uint32_t k, uint32_t y, uint32_t cnt, uint32_t G, uint32_t q) -> int32_t {
      // insert cnt - 1 is the output samples [., q + 1 + step * G)
      if (cnt && y < q + 1 + step * G) return kPadEmpty;
      const uint32_t x = y - step * G;
      return map.rev ? pad_load<S16>(a.signal, tr.sig_off + (uint64_t)(3 - k) * ns + (ns - 1 - x))
                     : pad_load<S16>(a.signal, tr.sig_off + (uint64_t)k * ns + x);
    };
    // a lane's window: the kPadVec samples from yb on, moved back by up to kPadVec - 1 per channel to where the store is aligned
    for (uint64_t y0 = 0; y0 < (uint64_t)ns_out + kPadVec - 1; y0 += 64 * kPadVec) {
      const uint64_t yb = y0 + (uint64_t)lane * kPadVec;
      const bool valid = yb < (uint64_t)ns_out + kPadVec - 1;
      const uint32_t vlo = yb >= kPadVec - 1 ? (uint32_t)(yb - (kPadVec - 1)) : 0u;
      uint32_t cnt, G, q;
      pad_search<true>(w, L, valid, vlo, cnt, G, q);
      if (!valid) continue;
      // no insert begins inside the window: one answer serves all its samples
      const bool same = cnt >= nins || (uint64_t)pad_key<true>(ins + (uint64_t)kPadInsWords * cnt, step) > yb + kPadVec - 1;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        // the window of channel k: [ys, ys + kPadVec) with ys = yb - shift[k] (yb is a multiple of kPadVec), where the store is aligned
        const int64_t ys = (int64_t)yb - shift[k];
        int32_t v[kPadVec];
        bool all = base_ok;
#pragma unroll
        for (uint32_t j = 0; j < kPadVec; ++j) {
          const int64_t y = ys + j;
          v[j] = 0;
          if (y < 0 || y >= (int64_t)ns_out) { all = false; continue; }
          if (same) v[j] = sample(k, (uint32_t)y, cnt, G, q);
          else {
            uint32_t c2, g2, q2;
            pad_search_slow(L, (uint32_t)y, c2, g2, q2);
            v[j] = sample(k, (uint32_t)y, c2, g2, q2);
          }
        }
        const uint64_t at = so + (uint64_t)k * ns_out + (uint64_t)ys;  // (ys < 0 only with all == false)
        if (all) pad_store_vec<S16>(a.o_signal, at, v);
        else
          for (uint32_t j = 0; j < kPadVec; ++j) {
            const int64_t y = ys + j;
            if (y >= 0 && y < (int64_t)ns_out) pad_store_one<S16>(a.o_signal, so + (uint64_t)k * ns_out + (uint64_t)y, v[j]);
          }
      }
    }
  }
}

}  // namespace tracyhip
#endif
