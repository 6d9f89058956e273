// pipe_internal.h -- what pipeline.hip (the pipelines planned by the host between launches) and stream.hip (the same stage orders
// planned on the device, one host synchronisation per call) know of each other.
#ifndef TRACY_AMD_PIPE_INTERNAL_H
#define TRACY_AMD_PIPE_INTERNAL_H

#include "capi_internal.h"

namespace tracyhip {

// internal status of stream_align / stream_decompose: the batch is outside what the stream-ordered pass is built for (an option
// selects another tier, caller-oriented windows, a wildtype-trace reference, scorings or shapes beyond the 16-bit / band forms) or
// a launch reported values outside its proven range; nothing was written, the host-planned pipeline takes the whole call
constexpr int kStreamNo = 3;

// the trims a job REQUESTS for trace t: its per-trace arrays (trim_left_each / trim_right_each) or, without them, the scalar pair for
// every trace.  Both pipelines read a job's trims through this alone, so the two forms share every line behind it.
struct TrimSrc {
  const uint32_t *l_each, *r_each;
  uint32_t l, r;
  uint32_t left(uint32_t t) const { return l_each ? l_each[t] : l; }
  uint32_t right(uint32_t t) const { return r_each ? r_each[t] : r; }
};
inline TrimSrc trims_of(const tracyhip_align_job* j) { return TrimSrc{j->trim_left_each, j->trim_right_each, j->trim_left, j->trim_right}; }
inline TrimSrc trims_of(const tracyhip_decompose_job* j) {
  return TrimSrc{j->trim_left_each, j->trim_right_each, (uint32_t)j->dprm.trim_left, (uint32_t)j->dprm.trim_right};
}

// sage.h:191-311 / indigo.h:190-388 for one context (no lanes), planned by the host between launches: every tier, every fallback
int align_traces_legacy(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm, int mem, const tracyhip_align_result* out);
int decompose_traces_legacy(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_params* prm, int mem,
                            const tracyhip_decompose_result* out);
// tracyhip_align_traces with a wildtype-trace reference (job->refs of kind PROFILE; wildtype.hip) for one context: stream-ordered, its own stages
int wildtype_align(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm, int mem, const tracyhip_align_result* out);
// the same stage orders with the planning on the device; traces whose tier the device cannot give them go through the functions
// above afterwards.  TRACYHIP_OK, an error, or kStreamNo.
int stream_align(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm, int mem, const tracyhip_align_result* out);
int stream_decompose(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_params* prm, int mem,
                     const tracyhip_decompose_result* out);

}  // namespace tracyhip
#endif
