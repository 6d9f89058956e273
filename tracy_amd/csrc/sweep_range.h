// sweep_range.h -- value-range rules of the 16-bit score sweeps (host side, plain C++: capi.hip wraps them, tests build them alone).
#ifndef TRACY_AMD_SWEEP_RANGE_H
#define TRACY_AMD_SWEEP_RANGE_H

#include <stdint.h>

#include <algorithm>

#include "../../include/tracy_hip.h"
#include "dp_lane.h"

namespace tracyhip {

inline int64_t range_abs64(int32_t x) { return x < 0 ? -(int64_t)x : (int64_t)x; }
inline int64_t range_sub_limit(const tracyhip_params* prm) { return std::max(range_abs64(prm->match), range_abs64(prm->mismatch)); }

// 16-bit score kernel: every real DP value must fit int16 with room below for the sentinel.  Q bounds the absolute value of
// a substitution score: max(|match|, |mismatch|) for strings and normalised profiles (the a-priori call, Q = 0), the
// device-reported maximum when a launch has seen a larger query-profile entry (range_verdict).
inline bool narrow_ok_rule(const tracyhip_params* prm, uint32_t maxm, int K, int64_t Q) {
  // free end gaps on the first/last row only, strictly negative extension, one pass of the strip height
  if (!prm->hfree || prm->vfree || prm->go > 0 || prm->ge >= 0 || num_passes(maxm ? maxm : 1, K) != 1) return false;
  Q = std::max<int64_t>(Q, range_sub_limit(prm));
  const int64_t rows = (int64_t)num_passes(maxm ? maxm : 1, K) * 64 * K;
  const int64_t low = range_abs64(prm->go) + rows * range_abs64(prm->ge) + 2 * (range_abs64(prm->go) + range_abs64(prm->ge)) + 2 * Q;
  const int64_t high = rows * Q;
  return (low < -(int64_t)kNegInf16 - range_abs64(prm->ge) - 64) && (high < 30000);
}

// The offset form of the 16-bit query-profile sweeps (dp_kernels.h gotoh_narrow_qp_body, DIAG): steps between two re-bases, or 0
// when the form has no room.  A live value is a true value under an offset of (row + column) |ge| - base.  The true values lie in
// narrow_ok's interval (-low, high) -- Q as there, rows = lanes x K.  Across the busy lanes of one wave step row + column spans
// (K - 1)(lanes - 1) + K + 1 (the lane that holds the last rows against the first lane's diagonal neighbour), the smallest of them
// sits at most K - 1 below the base (the padding slots above row 1), and between two re-bases the offsets grow by one |ge| per
// step.  Below, -low - (K - 1)|ge| has to stay inside int16; above, high + |ge| (span + period) under narrow_ok's ceiling -- and
// under int16 less one cell's own excursion (the diagonal candidate before the closing add: |go| + |ge| + Q).  The period is the
// largest power of two that fits, from 64 on (a period is a multiple of four -- a round of the sweep -- and no shorter than the ramp).
inline uint32_t sweep_diag_period_rule(const tracyhip_params* prm, int K, int lanes, int64_t Q) {
  if (!prm->hfree || prm->vfree || prm->go > 0 || prm->ge >= 0 || K < 1 || lanes < 1 || lanes > 64) return 0;
  Q = std::max<int64_t>(Q, range_sub_limit(prm));
  const int64_t g = range_abs64(prm->ge), go = range_abs64(prm->go), rows = (int64_t)lanes * K;
  const int64_t low = go + rows * g + 2 * (go + g) + 2 * Q;
  const int64_t high = rows * Q;
  if (low + (K - 1) * g >= 32768 - 64 - g) return 0;
  const int64_t span = (int64_t)(K - 1) * (lanes - 1) + K + 1;
  const int64_t room = std::min<int64_t>(30000, 32767 - 64 - (go + g + Q)) - high - g * span;  // g * period < room
  uint32_t period = 0;
  for (uint32_t p = 64; p <= 32768u && g * (int64_t)p < room; p *= 2) period = p;
  return period;
}

}  // namespace tracyhip
#endif
