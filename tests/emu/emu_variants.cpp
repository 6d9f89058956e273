// emu_variants.cpp -- host execution of the variant-calling wave body of `tracy decompose -v` (TEST INFRASTRUCTURE ONLY): the same
// tracy_amd/csrc/variants_wave.h text the HIP kernel runs, on the 64-fiber host wave, driven as variants_kernel drives it (one wave
// per trace, the two event lists in memory of its own).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/variants_wave.h"

using namespace tracyhip;

#include "host_wave.h"

extern "C" {

// one trace: alignment k is rows0[k] / rows1[k] of len[k] columns at rs.pos pos0[k].  var: max_variants records, text: max_text bytes.
int emu_variants(const uint8_t* row0a, const uint8_t* row1a, uint32_t lena, int32_t posa, const uint8_t* row0b, const uint8_t* row1b, uint32_t lenb,
                 int32_t posb, uint32_t forward, uint32_t bc_len, uint32_t trim_left, uint32_t trim_right, uint32_t max_variants, uint32_t max_text,
                 tracyhip_variant* var, uint8_t* text, uint32_t* var_n, uint32_t* var_flags) {
  VarTrace t{};
  t.row0[0] = row0a; t.row1[0] = row1a; t.len[0] = lena; t.pos0[0] = posa;
  t.row0[1] = row0b; t.row1[1] = row1b; t.len[1] = lenb; t.pos0[1] = posb;
  t.forward = forward; t.bc_len = bc_len;
  std::vector<VarEvent> ev(2 * (size_t)max_variants);  // exactly what the kernel hands a wave: a write past it is a sanitizer report
  WaveShared sh;
  sh.run([&](uint32_t lane) {
    HostWave w{lane, &sh};
    variants_wave(w, t, trim_left, trim_right, max_variants, max_text, ev.data(), var, text, var_n, var_flags);
  });
  return 0;
}

// callVariants of one alignment in push order: (pos, basenum, ref_len, alt_len) of the first min(n, cap) events into out; returns n
uint32_t emu_var_scan(const uint8_t* row0, const uint8_t* row1, uint32_t len, int32_t pos0, uint32_t cap, int32_t* out) {
  std::vector<VarEvent> ev(cap ? cap : 1);
  uint32_t n = 0;
  WaveShared sh;
  sh.run([&](uint32_t lane) {
    HostWave w{lane, &sh};
    const uint32_t k = var_scan_wave(w, row0, row1, len, pos0, ev.data(), cap);
    if (lane == 0) n = k;
  });
  for (uint32_t i = 0; i < n && i < cap; ++i) {
    out[4 * i] = ev[i].pos; out[4 * i + 1] = ev[i].basenum; out[4 * i + 2] = (int32_t)ev[i].ref_len; out[4 * i + 3] = (int32_t)ev[i].alt_len;
  }
  return n;
}
}
