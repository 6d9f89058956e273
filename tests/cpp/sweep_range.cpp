// sweep_range.cpp -- the value-range rules of the 16-bit sweeps (tracy_amd/csrc/sweep_range.h) behind C entry points, for
// tests/test_sweep_range_host.py.  Rows of int64 in, rows of int64 out.
#include "../../tracy_amd/csrc/sweep_range.h"

using namespace tracyhip;

extern "C" {
// in: match, mismatch, go, ge, hfree, vfree, maxm, K, lanes, Q   out: narrow_ok, period
void sr_rules(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i) {
    const int64_t* r = in + 10 * i;
    tracyhip_params p{};
    p.match = (int32_t)r[0]; p.mismatch = (int32_t)r[1]; p.go = (int32_t)r[2]; p.ge = (int32_t)r[3]; p.hfree = (int32_t)r[4]; p.vfree = (int32_t)r[5];
    out[2 * i] = narrow_ok_rule(&p, (uint32_t)r[6], (int)r[7], r[9]) ? 1 : 0;
    out[2 * i + 1] = sweep_diag_period_rule(&p, (int)r[7], (int)r[8], r[9]);
  }
}
}
