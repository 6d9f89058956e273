// consensus.h -- one column of `tracy consensus` (gtLetter, consensus.h:94-171 of the reference; host mirror
// tracy_amd/host/consensus_out.hpp) for the device, with the screen that decides which columns the host recomputes.
//
// Host and device compile this same header: consensus.hip's consensus_kernel calls cons_column per column, the CPU test
// (tests/test_consensus_host.py) builds it with g++ and checks letters, qualities and the screen against gtLetter.
//
// Exactness (DESIGN.md "Two-trace consensus"): every step of gtLetter is an IEEE double operation the device performs
// bit for bit like the host (adds, one division, compares, round) except log10.  Two observations remove the rest:
//   - bestPL is always 0 (gl[best] - bestVal == 0), so gq is a function of the integer secondPL in [0, 10000] alone; the
//     host tabulates it once with its own pow / log10 (cons_gq_table) and the device looks it up.
//   - gl[k] = log10(cl[k] / total) may differ between ocml and glibc in the last ulps.  A difference can only change the
//     result where a decision sits within that error of its threshold: two gl that order the classes, the half-integer
//     that rounds secondPL, the IUPAC threshold -1.  cons_column flags every column that comes within kConsTolGL /
//     kConsTolPL of one of them; the library recomputes flagged columns with the host gtLetter.
#ifndef TRACY_AMD_CONSENSUS_H
#define TRACY_AMD_CONSENSUS_H

#include <stdint.h>

#include "dp_lane.h"

#include <cmath>

namespace tracyhip {

// |gl| < 324 for every positive ratio of doubles (and gl = -1000 for zero), so one ulp of a gl is at most 2^-44.  glibc's
// log10 is documented within 2 ulp, ocml's double log10 within 1 ulp (4 ulp assumed here): a device and a host gl differ by
// less than 6 * 2^-44 < 2^-41.  The screens are 2^11 times wider than that.
constexpr double kConsTolGL = 1.0 / 1073741824.0;  // 2^-30: closeness of two gl, of gl[second] to -1
constexpr double kConsTolPL = 1.0 / 1048576.0;     // 2^-20: -10 (gl2 - gl1) against a half-integer (error <= 20 * 2^-41 + 2 ulp)
constexpr double kConsSmallestGL = -1000;          // SMALLEST_GL
constexpr uint32_t kConsMaxPL = 10000;             // -10 * SMALLEST_GL: the largest secondPL

struct ConsFixup {     // a screened column: the host recomputes it from the six class weights
  uint64_t slot;       // element index in cons / qual
  uint32_t pair;
  uint32_t pad;
  float cl[6];
};

TR_HD double cons_log10(double x) {
#if defined(CONS_HOST_LOG10)
  return CONS_HOST_LOG10(x);  // (the CPU test builds the header with a perturbed log10 to exercise the screen)
#elif defined(__HIP_DEVICE_COMPILE__)
  return log10(x);
#else
  return std::log10(x);
#endif
}
TR_HD double cons_round(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return round(x);
#else
  return std::round(x);
#endif
}
TR_HD double cons_floor(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return floor(x);
#else
  return std::floor(x);
#endif
}
TR_HD double cons_fabs(double x) { return x < 0 ? -x : x; }
TR_HD bool cons_finite(double x) { return x == x && x - x == 0.0; }

// IUPAC code of two different bases among A C G T (tracy_host.hpp iupac)
TR_HD char cons_iupac(uint32_t a, uint32_t b) {
  if (b < a) { const uint32_t t = a; a = b; b = t; }
  // (a, b) with a < b: AC M, AG R, AT W, CG S, CT Y, GT K
  const char tab[16] = {'N', 'M', 'R', 'W', 'N', 'N', 'S', 'Y', 'N', 'N', 'N', 'K', 'N', 'N', 'N', 'N'};
  return tab[a * 4 + b];
}

// gtLetter of one column from its six class weights (A C G T N -).  letter / qual receive what the device computes; the return value
// is true when the column lies within the screen of a decision and must be recomputed by the host gtLetter.  gq_tab: the quality of
// every secondPL 0 .. 10000 (cons_gq_table).
TR_HD bool cons_column(const double cl_in[6], bool use_iupac, const uint16_t* gq_tab, uint8_t* letter, uint16_t* qual) {
  double cl[6], gl[6];
  double total = 0;
  bool flag = false;
  for (int k = 0; k < 6; ++k) total += cl_in[k];
  if (!cons_finite(total)) flag = true;
  for (int k = 0; k < 6; ++k) {
    if (!(cl_in[k] >= 0)) flag = true;  // negative or NaN weights: the host alone
    cl[k] = total > 0 ? cl_in[k] / total : 0;
    if (cl[k] > 0) {
      gl[k] = cons_log10(cl[k]);
      if (gl[k] < kConsSmallestGL) gl[k] = kConsSmallestGL;
    } else gl[k] = kConsSmallestGL;
  }
  // two classes whose weights differ but whose gl lie within the error of each other may order differently on the host
  for (int a = 0; a < 6; ++a)
    for (int b = a + 1; b < 6; ++b)
      if (cl[a] != cl[b] && cons_fabs(gl[a] - gl[b]) < kConsTolGL) flag = true;
  uint32_t best = 0, second = 1;
  if (gl[best] < gl[second]) { best = 1; second = 0; }
  for (uint32_t k = 2; k < 6; ++k) {
    if (gl[k] > gl[best]) { second = best; best = k; }
    else if (gl[k] > gl[second]) second = k;
  }
  const double bestVal = gl[best];
  const double gs = gl[second];
  if (use_iupac && cons_fabs(gs + 1.0) < kConsTolGL) flag = true;
  const bool ambiguous = use_iupac && gs > -1 && best <= 3 && second <= 3;
  const double x = -10 * (gs - bestVal);
  if (cons_fabs(x - cons_floor(x) - 0.5) < kConsTolPL) flag = true;
  const double r = cons_round(x);
  uint32_t pl = 0;
  if (r >= 0 && r <= (double)kConsMaxPL) pl = (uint32_t)r;
  else flag = true;
  *letter = (uint8_t)(ambiguous ? cons_iupac(best, second) : "ACGTN-"[best]);
  *qual = gq_tab[pl];
  return flag;
}

// gq of gtLetter for bestPL = 0 and every secondPL 0 .. 10000, with the host's pow / log10 (the expression of consensus_out.hpp)
inline void cons_gq_table(uint16_t* tab) {
  const uint32_t bestPL = 0;
  for (uint32_t secondPL = 0; secondPL <= kConsMaxPL; ++secondPL) {
    double likelihood = std::log10(1 - 1 / (std::pow((double)10, -((double)bestPL / (double)10)) + std::pow((double)10, -((double)secondPL / (double)10))));
    likelihood = likelihood > kConsSmallestGL ? likelihood : kConsSmallestGL;
    int32_t gq = (int32_t)std::round(-10 * likelihood);
    if (gq < 0) gq = 0;
    tab[secondPL] = (uint16_t)gq;
  }
}

}  // namespace tracyhip
#endif
