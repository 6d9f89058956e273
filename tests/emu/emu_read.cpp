// emu_read.cpp -- host execution of the file reading wave bodies (TEST INFRASTRUCTURE ONLY): the same tracy_amd/csrc/read_wave.h code the HIP
// kernels run, on the 64-fiber host wave.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/read_wave.h"

using namespace tracyhip;

#include "host_wave.h"

extern "C" {

uint32_t emu_read_tile() { return kReadTile; }          // samples per tile of an ABIF channel
uint32_t emu_read_scf_tile() { return kReadScfTile; }   // samples per step of an SCF channel
uint32_t emu_read_bound_samples(uint32_t file_len) { return read_bound_samples(file_len); }
uint32_t emu_read_bound_calls(uint32_t file_len) { return read_bound_calls(file_len); }

// One file image of file_len bytes at bytes + file_off.  The result arrays may be null (all null: the sizes-only form); the signal is
// written from element out_sig_off of o_signal on, the calls from element out_call_off.  out4: status, format, nsamples, ncalls.  The
// scan runs, then every tile the host would launch for a file of this length.
void emu_read(const uint8_t* bytes, uint64_t file_off, uint32_t file_len, int sample_bytes, void* o_signal, uint64_t out_sig_off, uint32_t sample_cap,
              int32_t* o_pos, uint8_t* o_b1, uint8_t* o_b2, uint8_t* o_qual, uint64_t out_call_off, uint32_t call_cap, int32_t* out4) {
  ReadFile fl{};
  fl.file_off = file_off; fl.file_len = file_len;
  fl.out_sig_off = out_sig_off; fl.out_call_off = out_call_off;
  fl.sample_cap = sample_cap; fl.call_cap = call_cap;
  fl.tile_first = 0; fl.tiles_per_channel = read_channel_tiles(file_len);
  ReadDesc d{};
  d.status = -1; d.nsamples = d.ncalls = 0xdeadu;
  ReadArgs a{};
  a.bytes = bytes; a.fl = &fl; a.desc = &d;
  a.o_signal = o_signal; a.o_pos = o_pos; a.o_b1 = o_b1; a.o_b2 = o_b2; a.o_qual = o_qual;
  a.ntraces = 1; a.ntiles = 1 + 4 * fl.tiles_per_channel; a.sample_bytes = (uint32_t)sample_bytes;
  WaveShared sh;
  sh.run([&](uint32_t l) { HostWave w{l, &sh}; read_scan_body(w, a, 0); });
  if (o_signal || o_pos || o_b1 || o_b2 || o_qual)
    for (uint32_t tile = 0; tile < a.ntiles; ++tile) {
      if (sample_bytes == 2) sh.run([&](uint32_t l) { HostWave w{l, &sh}; read_emit_body<true>(w, a, tile); });
      else sh.run([&](uint32_t l) { HostWave w{l, &sh}; read_emit_body<false>(w, a, tile); });
    }
  out4[0] = d.status; out4[1] = d.format; out4[2] = (int32_t)d.nsamples; out4[3] = (int32_t)d.ncalls;
}
}
