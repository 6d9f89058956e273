// emu_pad.cpp -- host execution of the trace padding wave body (TEST INFRASTRUCTURE ONLY): the same tracy_amd/csrc/pad_wave.h code the HIP
// kernel runs, on the 64-fiber host wave.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/pad_wave.h"

using namespace tracyhip;

#include "host_wave.h"

extern "C" {

uint32_t emu_pad_insert_tile() { return kPadTile; }        // inserts per LDS tile
uint32_t emu_pad_sample_tile() { return 64 * kPadVec; }    // output samples per step of the sample pass

// One trace.  signal: int32 (sample_bytes 4) or int16 (2), channels A C G T of nsamples each; the five basecall arrays hold n entries.  The
// result arrays may be null (all null: the sizes-only form); the padded signal is written from element out_sig_off of o_signal on.
// out6: status, nsamples_out, ncalls_out, leading, trailing, step.  Returns 1 when the body wrote past its scratch region.
int emu_pad(const void* signal, int sample_bytes, uint32_t nsamples, const int32_t* bcpos, const uint8_t* primary, const uint8_t* secondary,
            const uint8_t* consensus, const uint8_t* estqual, uint32_t n, const uint8_t* row, uint32_t row_len, uint32_t trim_l, uint32_t trim_r,
            uint32_t reverse, void* o_signal, uint64_t out_sig_off, uint32_t sample_cap, int32_t* o_bcpos, uint8_t* o_primary, uint8_t* o_secondary,
            uint8_t* o_consensus, uint8_t* o_estqual, uint32_t call_cap, int32_t* out6) {
  PadTrace tr{};
  tr.out_sig_off = out_sig_off;
  tr.nsamples = nsamples; tr.bc_len = n; tr.row_len = row_len;
  tr.trim_l = trim_l; tr.trim_r = trim_r; tr.reverse = reverse;
  tr.sample_cap = sample_cap; tr.call_cap = call_cap;
  PadOut out{-1, 0xdeadu, 0xdeadu, 0xdeadu, 0xdeadu, 0xdeadu};
  const bool payload = o_signal || o_bcpos || o_primary || o_secondary || o_consensus || o_estqual;
  const size_t words = pad_sizes_answerable(nsamples, n, trim_l, trim_r) ? (size_t)kPadInsWords * pad_max_inserts(n - trim_l - trim_r, row_len) : 0;
  const uint32_t stale = 0xa5a5a5a5u;  // (stale scratch: the body must write what it reads)
  std::vector<uint32_t> scratch(words + 16, stale);
  PadArgs a{};
  a.signal = signal; a.bcpos = bcpos; a.primary = primary; a.secondary = secondary; a.consensus = consensus; a.estqual = estqual;
  a.rows = row; a.tr = &tr; a.out = &out; a.scratch = payload ? scratch.data() : nullptr;
  a.o_signal = o_signal; a.o_bcpos = o_bcpos; a.o_primary = o_primary; a.o_secondary = o_secondary; a.o_consensus = o_consensus;
  a.o_estqual = o_estqual;
  a.ntraces = 1;
  WaveShared sh;
  sh.lds.assign(kPadLdsBytes, (char)0x5a);
  if (sample_bytes == 2) sh.run([&](uint32_t l) { HostWave w{l, &sh}; pad_wave_body<true>(w, a, 0); });
  else sh.run([&](uint32_t l) { HostWave w{l, &sh}; pad_wave_body<false>(w, a, 0); });
  out6[0] = out.status; out6[1] = (int32_t)out.nsamples_out; out6[2] = (int32_t)out.ncalls_out; out6[3] = (int32_t)out.leading;
  out6[4] = (int32_t)out.trailing; out6[5] = (int32_t)out.step;
  for (size_t i = words; i < scratch.size(); ++i)
    if (scratch[i] != stale) return 1;
  return 0;
}
}
