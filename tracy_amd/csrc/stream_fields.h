// stream_fields.h -- the per-trace result arrays of tracyhip_align_traces and tracyhip_decompose_traces, each list written ONCE.
//
// A result array with one element (fractions: two) per trace is carved from the call's arena, pointed at the caller's device array,
// handed to the host-planned pipeline for the dead traces, scattered back through the dead list, copied to host memory and rebased
// for a lane (pipeline.hip AlignChunk / DecomposeChunk).  Every one of those walks the list below: each(a, b, fn) calls
// fn(a.X, b.X, per) for every array X, `per` its elements per trace.  a and b are any two of the structs that hold the arrays
// (stream.hip AlignOutDev / DecompResDev, tracyhip_align_result / tracyhip_decompose_result; the same struct twice where one suffices).
// The order is the order the scatters are queued in.  A new per-trace output is added here and to the structs, nowhere else.
//
// NOT in the lists: what is laid out by offsets instead of by trace (ops, dcp_indel, dcp_err, secdecomp, the basecalls) -- those keep
// their explicit handling where they are sized.
#ifndef TRACY_AMD_STREAM_FIELDS_H
#define TRACY_AMD_STREAM_FIELDS_H

#include <cstdint>

namespace tracyhip {

struct AlignFields {
  template <class A, class B, class Fn>
  static void each(A& a, B& b, Fn fn) {
    const uint32_t one = 1;
    fn(a.score_fwd, b.score_fwd, one);
    fn(a.score_rev, b.score_rev, one);
    fn(a.forward, b.forward, one);
    fn(a.score_prelim, b.score_prelim, one);  // (the caller's may be NULL)
    fn(a.slice_begin, b.slice_begin, one);
    fn(a.slice_len, b.slice_len, one);
    fn(a.ref_pos, b.ref_pos, one);
    fn(a.score_final, b.score_final, one);
    fn(a.ops_len, b.ops_len, one);
  }
};

struct DecompFields {
  template <class A, class B, class Fn>
  static void each(A& a, B& b, Fn fn) {
    const uint32_t one = 1;
    fn(a.bp, b.bp, one);
    fn(a.dstatus, b.dstatus, one);
    fn(a.fractions, b.fractions, 2u);  // allelicFraction: two doubles per trace
    fn(a.status, b.status, one);
    fn(a.score_fwd, b.score_fwd, one);
    fn(a.score_rev, b.score_rev, one);
    fn(a.forward, b.forward, one);
    fn(a.score_trim, b.score_trim, one);
    for (int k = 0; k < 2; ++k) {
      fn(a.slice_begin[k], b.slice_begin[k], one);
      fn(a.slice_len[k], b.slice_len[k], one);
      fn(a.ref_pos[k], b.ref_pos[k], one);
    }
    for (int k = 0; k < 3; ++k) {
      fn(a.score[k], b.score[k], one);
      fn(a.ops_len[k], b.ops_len[k], one);
    }
  }
};

}  // namespace tracyhip
#endif
