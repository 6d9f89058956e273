// basecall_wave.h -- basecall() + estimateQualities() + findBestTraceSection() + trimTrace() + createProfile() of ONE trace on ONE wave
// (abif.h:77-97, 164-253, 408-511; trim.h:35-73; profile.h:21-52), bit-identical with tracy_amd/host/tracy_host.hpp and sage_out.hpp.
//
// Data flow.  Basecall i owns the samples [floor(st_i), floor(ed_i)) of the chromatogram; ed_i == st_(i+1), so the windows of a trace tile
// its sample axis in order.  The wave takes 64 basecalls at a time (one per lane) and streams the samples they cover through LDS in tiles
// of kBcTile samples per channel with one halo sample on each side (the two local-maximum predicates look at i - 1 and i + 1): every
// sample is loaded once, coalesced, and a lane then scans its own ~12 samples from LDS.  Whatever a lane may need later of the
// chromatogram -- the four channels at each channel's best peak, at floor(st) and at the midpoint -- is kept in registers while the tile
// is there, so the peak table and the profile never read the chromatogram again.  Windows with floor(st) == floor(ed) give no basecall:
// the outputs are compacted with a wave scan, and bc_len is counted before the first output is written (the profile's row stride).
// The O(m) scans of the quality / trim stage run over three words per basecall in a global scratch region of the trace (bcPos + the
// ambiguity bit, penalty, prefix sum of the penalties), written and read by this wave only; neighbourhoods (10 basecalls) are staged
// through the same LDS.
//
// Floating point (every rule below is the reference's; the file must be compiled with -ffp-contract=off, stated again by the pragma):
//   st, ed          double arithmetic on (float)pos and (float)diff -- the last ed on the ints themselves -- rounded to float once
//   floor(st/ed)    float;  mid = (int)(((st + ed) rounded to float) / 2.0 in double);  mid >= floor(ed) compares as float
//   threshold       (int)(sigratio * (float)est): float product, truncated
//   ratio           (float)pv / (float)top: fp32 division, correctly rounded (no fast-math, no __fdividef)
//   mean spacing    double;  spread = (uint32)(int32)((|hi - mean| + |lo - mean|) / 2) in double, hi / lo 32-bit unsigned differences
//   estQual         60.0 - (60.0 / top) * penalty in double, product rounded before the subtraction; NaN -> 0; clamp to 0..60; truncated
//   stretch         (int)(0.1 * n) in double;  trim limit ((float)stringency * ((double)best / (double)stretch)) * 10 in double
//   profile         allsig / totalsig float sums in channel order; normfac, frac float divisions; normfac * frac rounded to float, then
//                   + (double)(1 - normfac) * 0.25 in double, rounded to float once
// Integer arithmetic on penalties and positions is 32-bit and wraps as the host's does.
//
// A trace is answered only when npos is in 1 .. kBcMaxPos, nsamples in 3 .. kBcMaxSamples and the positions are non-decreasing inside
// [0, nsamples); otherwise its status is TRACYHIP_BASECALL_DEFERRED, bc_len 0, and nothing else is written.  All positions are checked
// before the first read that depends on one.
//
// W: the wave abstraction of decompose_wave.h (lane, ballot, bcast, sum / umin / umax / excl_sum, sync, sync_global, lds).
#ifndef TRACY_AMD_BASECALL_WAVE_H
#define TRACY_AMD_BASECALL_WAVE_H

#include <cmath>
#include <cstdint>

#include "dp_lane.h"  // TR_HD

namespace tracyhip {

constexpr int32_t kBcStatusOk = 0, kBcStatusDeferred = 1;  // TRACYHIP_BASECALL_OK / _DEFERRED
constexpr uint32_t kBcMaxPos = 131071;                     // the decompose limit (tracyhip_decomp_params)
constexpr uint32_t kBcMaxSamples = 1u << 23;               // every position and half position is an exact float below this
constexpr uint32_t kBcRow = 512;                           // LDS words per channel: kBcTile samples + the two halo samples
constexpr uint32_t kBcTile = kBcRow - 2;
constexpr uint32_t kBcLdsBytes = 4 * kBcRow * 4;           // per wave

struct BasecallTrace {   // per trace, built by the host from the job's HOST arrays
  uint64_t sig_off;      // elements
  uint64_t pos_off;      // elements: positions in, and every per-basecall result out
  uint64_t scratch_off;  // words: 3 * npos + 1 of them
  uint32_t nsamples;
  uint32_t npos;
};
struct BasecallOut {
  int32_t status;
  uint32_t bc_len, trim_left, trim_right, best_section;
};
struct BasecallArgs {
  const void* signal;  // int32 or int16 samples
  const int32_t* pos;
  const BasecallTrace* tr;
  BasecallOut* out;
  uint32_t* scratch;
  // payload results, each may be null
  uint8_t *primary, *secondary, *consensus, *estqual;
  int32_t *bcpos, *peaks;
  float* profiles;
  uint32_t ntraces;
  float sigratio;
  float stringency;  // 0: no trim, else 1 .. 9
};

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// window borders of basecall i (abif.h:413-426): prev / next = the neighbouring positions (prev = 0 for the first)
TR_HD void bc_window(int32_t prev, int32_t cur, int32_t next, bool last, float& st, float& ed) {
  const int32_t diff = cur - prev;
  st = (float)((float)cur - 0.5 * (float)diff);
  if (last) ed = (float)(cur + 0.5 * diff);
  else ed = (float)((float)cur + 0.5 * (float)(next - cur));
}

TR_HD uint8_t bc_letter(uint32_t mask) {  // one or two of the bits A C G T -> the letter / IUPAC code (abif.h:135-161)
  switch (mask) {
    case 1: return 'A'; case 2: return 'C'; case 4: return 'G'; case 8: return 'T';
    case 3: return 'M'; case 5: return 'R'; case 9: return 'W'; case 6: return 'S'; case 10: return 'Y'; case 12: return 'K';
    default: return 'N';
  }
}

template <bool S16>
TR_HD int32_t bc_sample(const void* sig, uint64_t idx) {
  return S16 ? (int32_t) static_cast<const int16_t*>(sig)[idx] : static_cast<const int32_t*>(sig)[idx];
}

template <bool S16, class W>
TR_HD void basecall_wave_body(W& w, const BasecallArgs& a, uint32_t t) {
  const uint32_t lane = w.lane();
  const BasecallTrace tr = a.tr[t];
  const uint32_t np = tr.npos, ns = tr.nsamples;
  const int32_t* pos = a.pos + tr.pos_off;
  int32_t* tile = reinterpret_cast<int32_t*>(w.lds());  // tile[k * kBcRow + 1 + (p - s)]: sample p of channel k, tile core from s

  // ---- every position checked, and the basecalls counted, before anything depends on a position ----
  bool bad = np < 1 || np > kBcMaxPos || ns < 3 || ns > kBcMaxSamples;
  uint32_t n = 0;
  if (!bad) {
    uint32_t cnt = 0;
    for (uint32_t i0 = 0; i0 < np; i0 += 64) {
      const uint32_t i = i0 + lane;
      if (i < np) {
        const int32_t prev = i ? pos[i - 1] : 0, cur = pos[i], next = i + 1 < np ? pos[i + 1] : 0;
        if (cur < 0 || (uint32_t)cur >= ns || (i && cur < prev)) bad = true;
        float st, ed;
        bc_window(prev, cur, next, i + 1 == np, st, ed);
        if (floorf(st) != floorf(ed)) ++cnt;
      }
    }
    n = w.sum(cnt);
  }
  if (w.ballot(bad) != 0) {
    if (lane == 0) { a.out[t].status = kBcStatusDeferred; a.out[t].bc_len = 0; }
    return;
  }

  uint32_t* s0 = a.scratch + tr.scratch_off;  // bcPos | ambiguous(secondary) << 31
  uint32_t* s1 = s0 + np;                     // penalty
  uint32_t* s2 = s1 + np;                     // exclusive prefix sum of the penalties, n + 1 entries
  const uint64_t ob = tr.pos_off;
  const float sigratio = a.sigratio;

  // ---- windows, peaks, calls, peak table, profile: 64 basecalls at a time ----
  uint32_t base = 0;  // basecalls written so far
  for (uint32_t i0 = 0; i0 < np; i0 += 64) {
    const uint32_t i = i0 + lane;
    bool valid = false;
    int32_t fs = 0, fe = 0, mid = 0;
    float st = 0, ed = 0;
    if (i < np) {
      const int32_t prev = i ? pos[i - 1] : 0, cur = pos[i], next = i + 1 < np ? pos[i + 1] : 0;
      bc_window(prev, cur, next, i + 1 == np, st, ed);
      fs = (int32_t)floorf(st);
      fe = (int32_t)floorf(ed);
      valid = fs != fe;
      mid = (int32_t)((st + ed) / 2.0);
      if (mid >= floorf(ed)) mid = (int32_t)floorf(st);
    }
    const uint64_t vmask = w.ballot(valid);
    if (vmask == 0) continue;  // (wave-uniform)
    const uint32_t A = w.umin(valid ? (uint32_t)fs : 0xffffffffu);
    uint32_t B = w.umax(valid ? (uint32_t)fe : 0u);
    if (B > ns) B = ns;
    const int32_t lo = fs > 1 ? fs : 1, hi = (int32_t)ns - 1 < fe ? (int32_t)ns - 1 : fe;  // window_peaks' loop bounds
    int32_t bv[4] = {0, 0, 0, 0}, bi[4] = {fs, fs, fs, fs};
    int32_t cpk[4][4] = {}, cfs[4] = {0, 0, 0, 0}, cmid[4] = {0, 0, 0, 0};  // the four channels at bi[k], at fs, at mid
    for (uint32_t s = A; s < B; s += kBcTile) {
      const uint32_t e = s + kBcTile < B ? s + kBcTile : B;
      const uint32_t words = e - s + 2;  // samples s - 1 .. e
      w.sync();                          // (the previous tile has been read)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        for (uint32_t x = lane; x < words; x += 64) {
          const int64_t p = (int64_t)s - 1 + x;
          tile[k * kBcRow + x] = (p >= 0 && p < (int64_t)ns) ? bc_sample<S16>(a.signal, tr.sig_off + (uint64_t)k * ns + (uint64_t)p) : 0;
        }
      w.sync();
      if (valid) {
        const int32_t* T = tile + 1 - (int32_t)s;  // T[k * kBcRow + p]
        if ((uint32_t)fs >= s && (uint32_t)fs < e)
          for (int k = 0; k < 4; ++k) cfs[k] = T[k * kBcRow + fs];
        if ((uint32_t)mid >= s && (uint32_t)mid < e)
          for (int k = 0; k < 4; ++k) cmid[k] = T[k * kBcRow + mid];
        const int32_t x0 = lo > (int32_t)s ? lo : (int32_t)s, x1 = hi < (int32_t)e ? hi : (int32_t)e;
        if (x0 < x1) {
          int32_t pv[4], cv[4], nv[4];
          for (int k = 0; k < 4; ++k) { pv[k] = T[k * kBcRow + x0 - 1]; cv[k] = T[k * kBcRow + x0]; }
          for (int32_t x = x0; x < x1; ++x) {
            for (int k = 0; k < 4; ++k) nv[k] = T[k * kBcRow + x + 1];
            for (int k = 0; k < 4; ++k) {
              const bool rising_edge_top = (pv[k] <= cv[k]) && (cv[k] > nv[k]);
              const bool plateau_end = (pv[k] < cv[k]) && (cv[k] >= nv[k]);
              if ((rising_edge_top || plateau_end) && cv[k] > bv[k]) {
                bi[k] = x; bv[k] = cv[k];
                for (int c = 0; c < 4; ++c) cpk[k][c] = cv[c];
              }
            }
            for (int k = 0; k < 4; ++k) { pv[k] = cv[k]; cv[k] = nv[k]; }
          }
        }
      }
    }
    // abif.h:440-505
    const uint32_t j = base + w.excl_sum(valid ? 1u : 0u);
    base += (uint32_t)__builtin_popcountll(vmask);
    if (!valid) continue;  // (no barrier below in this iteration)
    for (int k = 0; k < 4; ++k)
      if (bv[k] == 0) { for (int c = 0; c < 4; ++c) cpk[k][c] = cfs[c]; }  // no peak in channel k: bi[k] is still fs
    int32_t est = 1;
    for (int k = 0; k < 4; ++k) if (cmid[k] > est) est = cmid[k];
    const int32_t threshold = (int32_t)(sigratio * est);
    if (bv[0] <= threshold && bv[1] <= threshold && bv[2] <= threshold && bv[3] <= threshold) {
      for (int k = 0; k < 4; ++k) {
        bi[k] = mid; bv[k] = cmid[k];
        for (int c = 0; c < 4; ++c) cpk[k][c] = cmid[c];
      }
    }
    int32_t top = 1;
    for (int k = 0; k < 4; ++k) if (bv[k] > top) top = bv[k];
    float ratio[4];
    for (int k = 0; k < 4; ++k) ratio[k] = (float)bv[k] / (float)top;
    float best = sigratio;
    int32_t sel = -1, selpos = bi[0], nvalid = 0;
    uint32_t vm = 0;
    int32_t pk[4] = {cpk[0][0], cpk[0][1], cpk[0][2], cpk[0][3]};
    for (int k = 0; k < 4; ++k) {
      if (ratio[k] >= sigratio) {
        ++nvalid;
        vm |= 1u << k;
        if (ratio[k] >= best) {  // last wins on exact ties
          best = ratio[k]; selpos = bi[k]; sel = k;
          for (int c = 0; c < 4; ++c) pk[c] = cpk[k][c];
        }
      }
    }
    uint8_t pri = 'N', sec = 'N', con = 'N';
    uint32_t in = 0;  // channels the calls name (_inBaseCalled, profile.h:7-19)
    if (!(nvalid == 4 || sel == -1)) {
      pri = bc_letter(1u << sel);
      in = vm;
      if (nvalid > 1) sec = bc_letter(vm & ~(1u << sel));
      else sec = con = pri;
    }
    if (a.primary) a.primary[ob + j] = pri;
    if (a.secondary) a.secondary[ob + j] = sec;
    if (a.consensus) a.consensus[ob + j] = con;
    if (a.bcpos) a.bcpos[ob + j] = selpos;
    if (a.peaks)
      for (int c = 0; c < 4; ++c) a.peaks[4 * (ob + j) + c] = pk[c];
    const bool amb = !(sec == 'A' || sec == 'C' || sec == 'G' || sec == 'T');
    s0[j] = (uint32_t)selpos | (amb ? 0x80000000u : 0u);
    if (a.profiles) {  // profile.h:21-52 on the peak table
      float* P = a.profiles + 6 * ob;
      float totalsig = 0, allsig = 0;
      for (int k = 0; k < 4; ++k) {
        allsig += pk[k];
        if ((in >> k) & 1u) totalsig += pk[k];
      }
      float v[4];
      if (totalsig == 0) {
        for (int k = 0; k < 4; ++k) v[k] = 0.25;
      } else {
        const float normfac = totalsig / allsig;
        for (int k = 0; k < 4; ++k) {
          const float frac = ((in >> k) & 1u) ? ((float)pk[k] / totalsig) : 0.0f;
          v[k] = normfac * frac + (1 - normfac) * 0.25;
        }
      }
      for (int k = 0; k < 4; ++k) P[(uint64_t)k * n + j] = v[k];
      P[4ull * n + j] = 0.0f;
      P[5ull * n + j] = 0.0f;
    }
  }

  // ---- findBestTraceSection (abif.h:164-220): penalties and their prefix sums ----
  w.sync_global();
  uint32_t* X = reinterpret_cast<uint32_t*>(tile);  // X[q - (b - 32)] = s0[q] for the 128 basecalls around chunk b
  uint32_t best_at = 0;
  int32_t best_sum = 99999999;
  uint32_t tl = 0, trr = 0;
  if (n) {
    const uint32_t win = 10, half = 5;
    const uint32_t lastpos = s0[n - 1] & 0x7fffffffu, firstpos = s0[0] & 0x7fffffffu;
    double mean = (double)(int32_t)(lastpos - firstpos);
    mean /= (double)(uint64_t)((uint64_t)n - 1);
    uint32_t carry = 0, topu = 0;
    for (uint32_t b = 0; b < n; b += 64) {
      w.sync();
      for (uint32_t x = lane; x < 128; x += 64) {
        const int64_t q = (int64_t)b - 32 + x;
        X[x] = (q >= 0 && q < (int64_t)n) ? s0[q] : 0u;
      }
      w.sync();
      const uint32_t jj = b + lane;
      uint32_t pen = 0;
      if (jj < n) {
        const uint32_t* Xq = X + 32 - (int32_t)b;  // Xq[q]
        uint32_t w0 = 0, wl = n;
        if (n >= win) { wl = win; w0 = jj < 4 ? 0 : jj - 4; if (w0 > n - win) w0 = n - win; }
        for (uint32_t q = 0; q < wl; ++q) pen += Xq[w0 + q] >> 31;
        if (n > win) {  // the spread of the ten spacings from basecall i on, i = jj - 5 clamped to the iterations that run
          uint32_t i = jj < half ? 0 : jj - half;
          if (i > n - win - 1) i = n - win - 1;
          uint32_t last = i > 0 ? (Xq[i - 1] & 0x7fffffffu) : 0u;
          uint32_t lo = lastpos, hi = 0;
          for (uint32_t k = 0; k < win; ++k) {
            const uint32_t c = Xq[i + k] & 0x7fffffffu;
            const uint32_t d = c - last;
            last = c;
            if (d < lo) lo = d;
            if (d > hi) hi = d;
          }
          const uint32_t spread = (uint32_t)(int32_t)((fabs((double)hi - mean) + fabs((double)lo - mean)) / 2);
          pen += spread;
        }
        s1[jj] = pen;
      }
      const uint32_t ex = w.excl_sum(jj < n ? pen : 0u);
      if (jj < n) s2[jj] = carry + ex;
      carry += w.sum(jj < n ? pen : 0u);
      const uint32_t nonneg = (jj < n && (int32_t)pen > 0) ? pen : 0u;
      const uint32_t m = w.umax(nonneg);
      if (m > topu) topu = m;
    }
    if (lane == 0) s2[n] = carry;
    w.sync_global();

    // ---- estimateQualities (abif.h:232-253) and the best 10 % stretch ----
    const int32_t top = (int32_t)topu;
    const double scaling = 60.0 / (double)top;
    const uint32_t stretch = (uint32_t)(int32_t)(0.1 * (double)(uint64_t)n);
    int32_t lbest = 99999999;
    uint32_t lat = 0xffffffffu;
    for (uint32_t b = 0; b < n; b += 64) {
      const uint32_t jj = b + lane;
      if (jj < n) {
        if (a.estqual) {
          const double q = 60.0 - scaling * (double)(int32_t)s1[jj];
          const int32_t v = (q != q) ? 0 : (q < 0 ? 0 : q > 60 ? 60 : (int32_t)q);
          a.estqual[ob + jj] = (uint8_t)v;
        }
        if (jj + stretch < n) {
          const int32_t sum = (int32_t)(s2[jj + stretch] - s2[jj]);
          if (sum < lbest) { lbest = sum; lat = jj; }
        }
      }
    }
    const uint32_t key = (uint32_t)lbest ^ 0x80000000u;
    const uint32_t kmin = w.umin(key);
    best_sum = (int32_t)(kmin ^ 0x80000000u);
    const uint32_t at = w.umin(key == kmin ? lat : 0xffffffffu);
    if (at != 0xffffffffu) best_at = at + stretch / 2;

    // ---- trimTrace (trim.h:35-73): first window sum above the limit on either side of the best stretch ----
    if (a.stringency >= 1) {
      const double per_base = (double)best_sum / (double)stretch;
      const double limit = (a.stringency * per_base) * win;
      const uint32_t centre = best_at;
      uint32_t right = n;
      for (uint32_t b = centre; b + win < n; b += 64) {  // local after step i: penalty[i + 1 .. i + 10]
        const uint32_t i = b + lane;
        const bool hit = i + win < n && (double)(int32_t)(s2[i + win + 1] - s2[i + 1]) > limit;
        const uint64_t hm = w.ballot(hit);
        if (hm) { right = b + (uint32_t)__builtin_ctzll(hm); break; }
      }
      trr = right < n ? n - right : 0;
      for (int64_t b = (int64_t)centre - 1; b >= 0; b -= 64) {  // local after step i: penalty[i .. min(i + 10, n))
        const int64_t i = b - lane;
        bool hit = false;
        if (i >= 0) {
          const uint32_t e = (uint32_t)i + win < n ? (uint32_t)i + win : n;
          hit = (double)(int32_t)(s2[e] - s2[i]) > limit;
        }
        const uint64_t hm = w.ballot(hit);
        if (hm) { tl = (uint32_t)(b - __builtin_ctzll(hm)) + win - 1; break; }
      }
    }
  }
  if (lane == 0) {
    BasecallOut o;
    o.status = kBcStatusOk;
    o.bc_len = n;
    o.trim_left = (uint16_t)tl;   // SageConfig holds the trims in 16 bits (sage.h:39-40)
    o.trim_right = (uint16_t)trr;
    o.best_section = best_at;
    a.out[t] = o;
  }
}

}  // namespace tracyhip
#endif
