// emu_render.cpp -- host execution of the trace printing wave bodies (TEST INFRASTRUCTURE ONLY): the same tracy_amd/csrc/render_wave.h
// code the HIP kernels run, on the 64-fiber host wave, tile after tile.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/render_wave.h"

using namespace tracyhip;

#include "host_wave.h"

extern "C" {

uint32_t emu_render_tile() { return kRenderTile; }          // items per tile
uint32_t emu_render_max_item() { return kRenderMaxItem; }   // bytes the LDS image has per item

// One trace.  signal: int32 (sample_bytes 4) or int16 (2), channels A C G T of nsamples each; the five basecall arrays hold n entries
// (consensus may be null unless form is the TSV).  text null: the sizes-only form; else the text is written from byte text_off on.
// out2: status, text_len.  Returns 1 when an item was longer than the LDS image allows, 2 when a body wrote past the tile scratch.
int emu_render(uint32_t form, const void* signal, int sample_bytes, uint32_t nsamples, const int32_t* bcpos, const uint8_t* primary,
               const uint8_t* secondary, const uint8_t* consensus, const uint8_t* estqual, uint32_t n, uint32_t trim_l, uint32_t trim_r,
               uint8_t* text, uint64_t text_off, uint64_t text_cap, int32_t* out2) {
  RenderTrace tr{};
  tr.text_off = text_off; tr.text_cap = text_cap;
  tr.nsamples = nsamples; tr.bc_len = n; tr.trim_l = trim_l; tr.trim_r = trim_r;
  tr.answerable = render_answerable(nsamples, n) ? 1u : 0u;
  const uint32_t tiles = tr.answerable ? render_tiles(form, nsamples, n) : 0u;
  RenderOut out{-1, 0xdeadu};
  const uint32_t stale = 0xa5a5a5a5u;  // (stale scratch: the bodies must write what they read)
  std::vector<uint32_t> bytes(tiles + 16, stale), aux(tiles + 16, stale);
  RenderArgs a{};
  a.signal = signal; a.bcpos = bcpos; a.primary = primary; a.secondary = secondary; a.consensus = consensus; a.estqual = estqual;
  a.tr = &tr; a.out = &out; a.tile_bytes = bytes.data(); a.tile_aux = aux.data(); a.text = text;
  a.ntraces = 1; a.ntiles = tiles; a.form = form;
  WaveShared sh;
  constexpr size_t kGuard = 1024;  // behind the wave's LDS: an item longer than kRenderMaxItem lands here
  auto fresh = [&]() { sh.lds.assign(kRenderLdsBytes + kGuard, (char)0x5a); };
  auto guard_ok = [&]() {
    for (size_t i = kRenderLdsBytes; i < sh.lds.size(); ++i)
      if (sh.lds[i] != (char)0x5a) return false;
    return true;
  };
  for (uint32_t k = 0; k < tiles; ++k) {
    fresh();
    if (sample_bytes == 2) sh.run([&](uint32_t l) { HostWave w{l, &sh}; render_count_body<true>(w, a, k); });
    else sh.run([&](uint32_t l) { HostWave w{l, &sh}; render_count_body<false>(w, a, k); });
    const RenderTileAt at = render_locate(form, nsamples, n, k);
    if (bytes[k] > (at.i1 - at.i0) * kRenderMaxItem) return 1;
  }
  fresh();
  sh.run([&](uint32_t l) { HostWave w{l, &sh}; render_scan_body(w, a, 0); });
  if (text)
    for (uint32_t k = 0; k < tiles; ++k) {
      fresh();
      if (sample_bytes == 2) sh.run([&](uint32_t l) { HostWave w{l, &sh}; render_emit_body<true>(w, a, k); });
      else sh.run([&](uint32_t l) { HostWave w{l, &sh}; render_emit_body<false>(w, a, k); });
      if (!guard_ok()) return 1;
    }
  out2[0] = out.status; out2[1] = (int32_t)out.text_len;
  for (size_t i = tiles; i < bytes.size(); ++i)
    if (bytes[i] != stale || aux[i] != stale) return 2;
  return 0;
}
}
