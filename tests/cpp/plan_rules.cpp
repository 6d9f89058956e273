// plan_rules.cpp -- host build of the per-trace planning rules of tracy_amd/csrc/stream_plan.h and dp_lane.h (the functions both planners call)
// for tests/test_plan_rules_host.py.  Every entry point takes n rows of int64 arguments (row-major, cast to the rule's parameter
// types as a caller's would be) and writes n rows of int64 results.
#include <cstdint>

#include "../../tracy_amd/csrc/stream_plan.h"

using namespace tracyhip;

extern "C" {

void pr_consts(int64_t* out) {
  out[0] = kFrontRows;
  out[1] = kFrontK;
  out[2] = kFrontHalfW;
}

// in: ri risize n trim_left trim_right forward -> ri len pos pad
void pr_trim_finish(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 6, out += 4) {
    const TrimRec r = s_trim_finish((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], in[5] != 0);
    out[0] = r.ri; out[1] = r.len; out[2] = r.pos; out[3] = r.pad;
  }
}

static tracyhip_params params(const int64_t* in) {
  tracyhip_params p;
  p.match = (int32_t)in[0]; p.mismatch = (int32_t)in[1]; p.go = (int32_t)in[2]; p.ge = (int32_t)in[3];
  p.hfree = (int32_t)in[4]; p.vfree = (int32_t)in[5];
  return p;
}

// in: match mismatch go ge hfree vfree m n -> origin16_ok(m, n), b16_origin_ok(m, n), s_front_ok(m, n)
void pr_front_ok(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 8, out += 3) {
    const tracyhip_params p = params(in);
    out[0] = origin16_ok(&p, (uint32_t)in[6], (uint32_t)in[7]);
    out[1] = b16_origin_ok(p.match, p.mismatch, p.go, p.ge, (uint32_t)in[6], (uint32_t)in[7]);
    out[2] = s_front_ok(&p, (uint32_t)in[6], (uint32_t)in[7]);
  }
}

// in: vf vr m front_ok exact -> g both cls
void pr_orient_class(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 5, out += 3) {
    const SOrient o = s_orient_class((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], in[3] != 0, in[4] != 0);
    out[0] = o.g; out[1] = o.both; out[2] = o.cls;
  }
}

// in: vf vr -> g clear; orient -> vote_skips_checkpoints (the sweep kernels' use of the same vote)
void pr_clear_vote(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 3, out += 3) {
    const ClearVote v = s_clear_vote((uint32_t)in[0], (uint32_t)in[1]);
    out[0] = v.g; out[1] = v.clear;
    out[2] = vote_skips_checkpoints((uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2]);
  }
}

// in: g prefix ub s_g -> certified bound
void pr_strand_by_bound(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 4, out += 2) {
    const SStrand c = s_strand_by_bound((uint32_t)in[0], (int32_t)in[1], (int32_t)in[2], in[3]);
    out[0] = c.certified; out[1] = c.bound;
  }
}

// in: m ce g -> dlo dhi K
void pr_end_band(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 3, out += 3) {
    const SBand b = s_end_band((uint32_t)in[0], in[1], in[2]);
    out[0] = b.dlo; out[1] = b.dhi; out[2] = b.K;
  }
}

// in: m ce top sstar ge -> g a n dlo dhi K
void pr_sub_window(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 5, out += 6) {
    const SubWindow s = s_sub_window((uint32_t)in[0], (uint32_t)in[1], in[2], in[3], (int32_t)in[4]);
    out[0] = s.g; out[1] = s.a; out[2] = s.n; out[3] = s.dlo; out[4] = s.dhi; out[5] = s.K;
  }
}

// in: n K -> fits
void pr_fits_lds(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 2, out += 1) out[0] = s_fits_lds((uint32_t)in[0], (int)in[1]);
}

// in: gap -> w
void pr_final_width(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = s_final_width((uint32_t)in[i]);
}

// in: m n want -> w dlo dhi K
void pr_final_band(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 3, out += 4) {
    const SFinalBand f = s_final_band((uint32_t)in[0], (uint32_t)in[1], in[2]);
    out[0] = f.w; out[1] = f.dlo; out[2] = f.dhi; out[3] = f.K;
  }
}

// in: sb top ge w ops_len -> certified
void pr_final_certified(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 5, out += 1)
    out[0] = s_final_certified((int32_t)in[0], (int32_t)in[1], (int32_t)in[2], in[3], (uint32_t)in[4]);
}

// in: m n ce g narrow lead ri -> dlo dhi K
void pr_slice_band(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 7, out += 3) {
    const SBand b = s_slice_band((uint32_t)in[0], (uint32_t)in[1], in[2], in[3], in[4] != 0, (uint32_t)in[5], (uint32_t)in[6]);
    out[0] = b.dlo; out[1] = b.dhi; out[2] = b.K;
  }
}

// in: len best go ge sc1 sc2 -> dlo dhi K bound
void pr_a12_band(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 6, out += 4) {
    const SA12Band b = s_a12_band((uint32_t)in[0], in[1], (int32_t)in[2], (int32_t)in[3], (int32_t)in[4], (int32_t)in[5]);
    out[0] = b.dlo; out[1] = b.dhi; out[2] = b.K; out[3] = b.bound;
  }
}

// in: sb sstar ops_len -> certified
void pr_exact_certified(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 3, out += 1) out[0] = s_exact_certified((int32_t)in[0], (int32_t)in[1], (uint32_t)in[2]);
}

// in: sb bound ops_len -> certified (sb: an int32 score, as both callers hold it; the bound is 64-bit)
void pr_a12_certified(uint64_t n, const int64_t* in, int64_t* out) {
  for (uint64_t i = 0; i < n; ++i, in += 3, out += 1) out[0] = s_a12_certified((int32_t)in[0], in[1], (uint32_t)in[2]);
}

}  // extern "C"
