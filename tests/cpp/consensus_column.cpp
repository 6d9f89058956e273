// consensus_column.cpp -- host build of tracy_amd/csrc/consensus.h (the column body consensus_kernel runs) for
// tests/test_consensus_host.py: letters, qualities and the fix-up screen against the host gtLetter (consensus_out.hpp).
//
// cons_log10 is routed through test_log10, which can move every result by up to `g_ulps` ulps (direction from the bits of the
// argument): a stand-in for a device log10 that differs from glibc's in the last places.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

static int g_ulps = 0;
static double test_log10(double x) {
  double r = std::log10(x);
  if (g_ulps == 0) return r;
  uint64_t b;
  std::memcpy(&b, &x, 8);
  b ^= b >> 29;
  b *= 0x9E3779B97F4A7C15ull;
  const int steps = (int)((b >> 40) % (uint64_t)(2 * g_ulps + 1)) - g_ulps;
  for (int s = 0; s < (steps < 0 ? -steps : steps); ++s) r = std::nextafter(r, steps < 0 ? -INFINITY : INFINITY);
  return r;
}
#define CONS_HOST_LOG10 test_log10

#include "../../tracy_amd/csrc/consensus.h"
#include "../../tracy_amd/host/consensus_out.hpp"

extern "C" {

void cc_gq_table(uint16_t* tab) { tracyhip::cons_gq_table(tab); }

// the device column body on n columns of six float weights (cl[6 i + k])
void cc_screen(uint64_t n, const float* cl, int iupac, int ulps, uint8_t* letter, uint16_t* qual, uint8_t* flag) {
  std::vector<uint16_t> tab(tracyhip::kConsMaxPL + 1);
  tracyhip::cons_gq_table(tab.data());
  g_ulps = ulps;
  for (uint64_t i = 0; i < n; ++i) {
    double c[6];
    for (int k = 0; k < 6; ++k) c[k] = (double)cl[6 * i + k];
    flag[i] = tracyhip::cons_column(c, iupac != 0, tab.data(), &letter[i], &qual[i]) ? 1 : 0;
  }
  g_ulps = 0;
}

// the host gtLetter (what a fixed-up column receives)
void cc_gt_letter(uint64_t n, const float* cl, int iupac, uint8_t* letter, uint32_t* qual) {
  tracy_amd::ConsensusOptions co;
  co.useIUPAC = iupac != 0;
  for (uint64_t i = 0; i < n; ++i) {
    double c[6];
    for (int k = 0; k < 6; ++k) c[k] = (double)cl[6 * i + k];
    std::string s;
    std::vector<uint32_t> q;
    tracy_amd::gtLetter(co, c, s, q);
    letter[i] = (uint8_t)s[0];
    qual[i] = q[0];
  }
}
}
