// emu_sweep_diag.cpp -- the 16-bit query-profile sweeps in their offset form (dp_kernels.h gotoh_narrow_qp_body / gotoh_prefix_body,
// DIAG) on the host wave of the emulators (TEST INFRASTRUCTURE ONLY): one pair per call through the full sweep, with or without
// checkpoints and row m, or a wave of prefix groups with their kept rows -- in either form, so that a test can set the two side by
// side -- and the range rules of sweep_range.h.  Never linked into the product library.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../../tracy_amd/csrc/dp_kernels.h"
#include "../../tracy_amd/csrc/sweep_range.h"

using namespace tracyhip;

#include "host_wave.h"

namespace {
template <int K, int MODE, bool CKPT, bool DIAG>
void run_sweep(const DpArgs& a) {
  // both table forms, as the library launches them: exactly one of them takes the pair (DpArgs::special_blocks)
  for (int form = 0; form < 2; ++form) {
    WaveShared sh;
    sh.lds.assign(lds_bytes_sweep16(K, false) + 64, 0);
    sh.run([&](uint32_t l) {
      HostWave w{l, &sh};
      if (form == 0) gotoh_body<HostWave, K, MODE, false, true, CKPT, 0, true, DIAG>(w, a, 0);
      else gotoh_body<HostWave, K, MODE, false, true, CKPT, 0, false, DIAG>(w, a, 0);
    });
  }
}
template <int K>
void run_sweep_k(bool strings, bool ckpt, bool diag, const DpArgs& a) {
#define EMU_SD(MODE)                                                              \
  if (ckpt) { if (diag) run_sweep<K, MODE, true, true>(a); else run_sweep<K, MODE, true, false>(a); } \
  else { if (diag) run_sweep<K, MODE, false, true>(a); else run_sweep<K, MODE, false, false>(a); }
  if (strings) { EMU_SD(MODE_CQ) } else { EMU_SD(MODE_QP) }
#undef EMU_SD
}
template <int K, int GL, bool DIAG>
void run_prefix(const DpArgs& a, uint32_t npairs) {
  for (int form = 0; form < 2; ++form) {  // both table forms: every group is worked on in one of them
    WaveShared sh;
    sh.lds.assign(lds_bytes_prefix(K, false) + 64, 0);
    sh.run([&](uint32_t l) {
      HostWave w{l, &sh};
      if (form == 0) gotoh_prefix_body<HostWave, K, GL, true, false, DIAG>(w, a, 0, npairs);
      else gotoh_prefix_body<HostWave, K, GL, false, false, DIAG>(w, a, 0, npairs);
    });
  }
}
}  // namespace

extern "C" {

// The prefix rows of up to 64 / GL pairs on one wave: profiles a1 + a1_off[i] (float[6][m[i]]), reference characters a2 + a2_off[i]
// (n[i] bytes); flags[i] & 1 = reverse-complement view, & 2 = no pair in this group (skipped).  out[i]: the reported bound;
// kept + kept_off[i]: row R = GL x K of pair i, n[i] + 5 dwords ({F (high half), H + goe} at index column).
int emu_prefix_diag(int K, int GL, uint32_t period, uint32_t npairs, const float* a1, const uint64_t* a1_off, const uint32_t* m, const uint8_t* a2,
                    const uint64_t* a2_off, const uint32_t* n, const uint32_t* flags, const uint64_t* kept_off, int32_t match, int32_t mismatch,
                    int32_t go, int32_t ge, int32_t* out, int32_t* kept, int32_t* err_out) {
  std::vector<PairDesc> d(npairs);
  uint64_t extent = 0;
  for (uint32_t i = 0; i < npairs; ++i) {
    d[i] = PairDesc{};
    d[i].a1_off = a1_off[i]; d[i].a2_off = a2_off[i]; d[i].m = m[i]; d[i].n = n[i]; d[i].a1_stride = m[i]; d[i].a2_stride = n[i];
    d[i].flags = ((flags[i] & 1u) ? PAIR_A2_REVCOMP : 0u) | ((flags[i] & 2u) ? PAIR_SKIP : 0u) | PAIR_KEEP_ROW;
    d[i].out = i; d[i].lastrow_off = kept_off[i];
    extent = std::max<uint64_t>(extent, a2_off[i] + n[i]);
  }
  std::vector<uint8_t> codes((size_t)extent + 256, 5);
  for (uint64_t j = 0; j < extent; ++j) codes[128 + j] = (uint8_t)dp_code(a2[j]);
  std::vector<uint8_t> special(((size_t)extent >> 8) + 2, 0);
  for (uint64_t j = 0; j < extent; ++j) if (codes[128 + j] >= 4) special[j >> 8] = 1;
  int32_t errw[kErrWords] = {0};
  DpArgs a{};
  a.pairs = d.data(); a.a1 = a1; a.a2 = codes.data() + 128; a.special_blocks = special.data(); a.scores = out; a.err = errw; a.lastrow = kept;
  a.match = match; a.mismatch = mismatch; a.go = go; a.ge = ge; a.hfree = 1; a.vfree = 0;
  a.qlimit = std::max(std::abs(match), std::abs(mismatch));
  a.diag_period = period;
  if (K == 8 && GL == 16) { if (period) run_prefix<8, 16, true>(a, npairs); else run_prefix<8, 16, false>(a, npairs); }
  else if (K == 8 && GL == 8) { if (period) run_prefix<8, 8, true>(a, npairs); else run_prefix<8, 8, false>(a, npairs); }
  else if (K == 16 && GL == 8) { if (period) run_prefix<16, 8, true>(a, npairs); else run_prefix<16, 8, false>(a, npairs); }
  else if (K == 15 && GL == 8) { if (period) run_prefix<15, 8, true>(a, npairs); else run_prefix<15, 8, false>(a, npairs); }
  else return -1;
  if (err_out) { err_out[0] = errw[0]; err_out[1] = errw[1]; }
  return 0;
}

// One pair through the sweep.  a1: float[6][stride] profile, or (strings) m characters; a2: the n reference characters.
// period: 0 = values as they are, else the offset form with that many steps between re-bases.  ckpt: the checkpointed sweep, which
// leaves row m (lastrow: n + 2 dwords) and a frontier record every B steps (ckpt_out: nrec records of (K + 1) x 64 dwords).
int emu_sweep(int K, int strings, uint32_t period, int ckpt, uint32_t B, const void* a1, uint32_t m, uint32_t stride, const uint8_t* a2, uint32_t n,
              int revcomp, int32_t match, int32_t mismatch, int32_t go, int32_t ge, int32_t* score, int32_t* lastrow, int32_t* ckpt_out,
              uint32_t nrec, int32_t* err_out) {
  if (ckpt && (uint64_t)nrec * B < (uint64_t)n + 64) return -2;
  PairDesc d{};
  d.m = m; d.n = n; d.a1_stride = stride; d.a2_stride = n; d.flags = revcomp ? PAIR_A2_REVCOMP : 0u; d.out = 0;
  std::vector<uint8_t> codes((size_t)n + 256, 5);  // padded like the library's code buffers: the sweep looks ahead of and behind a window
  for (uint32_t j = 0; j < n; ++j) codes[128 + j] = (uint8_t)(strings ? cq_code(a2[j]) : dp_code(a2[j]));
  std::vector<uint8_t> special(((size_t)n >> 8) + 2, 0);
  for (uint32_t j = 0; j < n; ++j) if (codes[128 + j] >= 4) special[j >> 8] = 1;
  int32_t errw[kErrWords] = {0};
  DpArgs a{};
  a.pairs = &d; a.a1 = a1; a.a2 = codes.data() + 128; a.special_blocks = special.data(); a.scores = score; a.err = errw;
  a.match = match; a.mismatch = mismatch; a.go = go; a.ge = ge; a.hfree = 1; a.vfree = 0;
  a.qlimit = std::max(std::abs(match), std::abs(mismatch));
  a.diag_period = period;
  if (ckpt) { a.ckpt = ckpt_out; a.lastrow = lastrow; a.ckpt_B = B; a.ckpt_narrow = 1; }
  *score = 0x7fffffff;
  switch (K) {
    case 15: run_sweep_k<15>(strings != 0, ckpt != 0, period != 0, a); break;
    case 16: run_sweep_k<16>(strings != 0, ckpt != 0, period != 0, a); break;
    default: return -1;
  }
  if (err_out) { err_out[0] = errw[0]; err_out[1] = errw[1]; }
  return 0;
}

// the range rules (sweep_range.h): narrow_ok and the period of the offset form
int emu_narrow_ok(int32_t match, int32_t mismatch, int32_t go, int32_t ge, uint32_t maxm, int K, int64_t Q) {
  tracyhip_params p{};
  p.match = match; p.mismatch = mismatch; p.go = go; p.ge = ge; p.hfree = 1; p.vfree = 0;
  return narrow_ok_rule(&p, maxm, K, Q) ? 1 : 0;
}
uint32_t emu_diag_period(int32_t match, int32_t mismatch, int32_t go, int32_t ge, int K, int lanes, int64_t Q) {
  tracyhip_params p{};
  p.match = match; p.mismatch = mismatch; p.go = go; p.ge = ge; p.hfree = 1; p.vfree = 0;
  return sweep_diag_period_rule(&p, K, lanes, Q);
}
}
