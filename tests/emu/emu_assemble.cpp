// emu_assemble.cpp -- host execution of the row-block wave bodies of `tracy assemble` (TEST INFRASTRUCTURE ONLY): the same
// tracy_amd/csrc/assemble_wave.h code the HIP kernels run, on the 64-fiber host wave, driven as the kernels of assemble.hip drive it
// (one wave per merged row, per 64 columns of a profile, per consensus).
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/assemble_wave.h"

using namespace tracyhip;

#include "host_wave.h"

namespace {
MsaSide side(const uint8_t* rows, const float* prof, uint32_t n, uint32_t c) { return MsaSide{prof ? nullptr : rows, prof, prof ? 1u : n, c, c}; }
}  // namespace

extern "C" {

// ops: push order, L of them.  Each side: rows (n x c bytes) or, when prof is not null, one 6 x c profile shown as its consensus
// characters.  out: (n1 + n2) x L bytes; span: 2 per row of out.
int emu_msa_merge(const uint8_t* ops, uint32_t L, const uint8_t* rows1, const float* prof1, uint32_t n1, uint32_t c1, const uint8_t* rows2,
                  const float* prof2, uint32_t n2, uint32_t c2, uint8_t* out, int32_t* span) {
  const MsaSide l = side(rows1, prof1, n1, c1), r = side(rows2, prof2, n2, c2);
  for (uint32_t row = 0; row < l.n + r.n; ++row) {
    const bool left = row < l.n;
    WaveShared sh;
    sh.run([&](uint32_t lane) {
      HostWave w{lane, &sh};
      msa_merge_row_wave(w, ops, L, left ? l : r, left ? row : row - l.n, left, out + (uint64_t)row * L, span + 2 * row);
    });
  }
  return 0;
}

int emu_msa_span(const uint8_t* rows, uint32_t nrows, uint32_t ncol, int32_t* span) {
  for (uint32_t row = 0; row < nrows; ++row) {
    WaveShared sh;
    sh.run([&](uint32_t lane) { HostWave w{lane, &sh}; msa_span_wave(w, rows + (uint64_t)row * ncol, ncol, span + 2 * row); });
  }
  return 0;
}

// prof: 6 x ncol floats
int emu_msa_profile(const uint8_t* rows, uint32_t nrows, uint32_t ncol, float* prof) {
  std::vector<int32_t> span(2 * (size_t)nrows + 2, 0x5a5a5a5a);
  emu_msa_span(rows, nrows, ncol, span.data());
  for (uint32_t b = 0; b < ncol; b += 64) {
    WaveShared sh;
    sh.run([&](uint32_t lane) { HostWave w{lane, &sh}; msa_profile_wave(w, rows, nrows, ncol, span.data(), b, prof); });
  }
  return 0;
}

// gapped: ncol bytes; cons / qual: up to ncol bytes; returns cons_len through out_len
int emu_msa_consensus(const uint8_t* rows, uint32_t nrows, uint32_t ncol, float fraction_called, int ignore_last, uint8_t* gapped, uint8_t* cons,
                      uint8_t* qual, uint32_t* out_len) {
  std::vector<int32_t> span(2 * (size_t)nrows + 2, 0x5a5a5a5a);
  emu_msa_span(rows, nrows, ncol, span.data());
  const int64_t used = (int64_t)nrows - (ignore_last ? 1 : 0);
  const int32_t thr = (int32_t)(fraction_called * (float)(size_t)used);  // msa.h:196
  WaveShared sh;
  sh.run([&](uint32_t lane) {
    HostWave w{lane, &sh};
    msa_consensus_wave(w, rows, (uint32_t)used, ncol, span.data(), thr, gapped, cons, qual, out_len);
  });
  return 0;
}
}
