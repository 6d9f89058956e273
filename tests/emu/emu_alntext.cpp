// emu_alntext.cpp -- host execution of the alignment printing wave bodies and of the reference slice body (TEST INFRASTRUCTURE ONLY): the
// same tracy_amd/csrc/alntext_wave.h code the HIP kernels run, on the 64-fiber host wave, tile after tile; the descriptors come from
// tracy_amd/csrc/alntext_plan.h as alntext.hip builds them.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/alntext_plan.h"
#include "../../tracy_amd/csrc/alntext_wave.h"

using namespace tracyhip;

#include "host_wave.h"

extern "C" {

uint32_t emu_alntext_tile() { return kAlnTile; }          // items per tile
uint32_t emu_alntext_max_item() { return kAlnMaxItem; }   // bytes the LDS image has per item
uint32_t emu_slice_tile() { return kSliceTile; }

// One alignment of a job of one.  text null: the sizes-only form; else the text is written from byte text_off on.  out2: status,
// text_len.  Returns 1 when an item was longer than the LDS image allows, 2 when a body wrote past the tile scratch, 3 when the job is
// refused by tracyhip_render_alignments_validate's rules.
int emu_alntext(uint32_t form, uint32_t key, uint32_t linelimit, const uint8_t* row0, const uint8_t* row1, uint32_t cols, const uint8_t* names,
                uint32_t name0_len, uint32_t name1_len, int32_t ref_pos, uint32_t ref_len, uint8_t forward, int32_t score, uint8_t* text,
                uint64_t text_off, uint64_t text_cap, int32_t* out2) {
  const uint64_t rows_off = 0, n0_off = 0, n1_off = name0_len;
  int32_t status = -1;
  uint32_t text_len = 0xdeadu;
  tracyhip_alntext_job job{};
  job.n = 1; job.form = form; job.key = key; job.linelimit = linelimit;
  job.rows0 = row0; job.rows1 = row1; job.rows_offset = &rows_off; job.cols = &cols;
  job.names = names; job.name0_offset = &n0_off; job.name0_len = &name0_len; job.name1_offset = &n1_off; job.name1_len = &name1_len;
  job.ref_pos = &ref_pos; job.ref_len = &ref_len; job.forward = &forward; job.score = &score;
  tracyhip_alntext_result res{};
  res.status = &status; res.text_len = &text_len; res.text = text; res.text_offset = &text_off; res.text_cap = &text_cap;
  if (alntext_validate(&job, TRACYHIP_MEM_DEVICE, &res)) return 3;
  std::vector<AlnChunk> chunks;
  uint32_t bad = 0;
  if (!alntext_cut_chunks(&job, &res, false, ~0ull, chunks, &bad) || chunks.size() != 1) return 3;
  const AlnDesc d = alntext_desc(&job, &res, chunks[0], false, 0, 0, 0);
  const uint32_t tiles = alntext_tiles(&job, 0), coltiles = alntext_coltiles(&job, 0);
  AlnOut out{-1, 0xdeadu};
  const uint32_t stale = 0xa5a5a5a5u;  // (stale scratch: the bodies must write what they read)
  std::vector<uint32_t> bytes(tiles + 16, stale), aux(2 * tiles + 16, stale), letters(2 * coltiles + 16, stale);
  AlnArgs a{};
  a.rows0 = row0; a.rows1 = row1; a.names = names;
  a.al = &d; a.out = &out; a.tile_bytes = bytes.data(); a.tile_aux = aux.data(); a.col_letters = letters.data(); a.text = text;
  a.n = 1; a.ntiles = tiles; a.ncoltiles = coltiles; a.form = form;
  a.key = form == kAlnPlot ? key : 0u; a.linelimit = form == kAlnPlot ? linelimit : 1u;
  WaveShared sh;
  constexpr size_t kGuard = 1024;  // behind the wave's LDS: an item longer than kAlnMaxItem lands here
  auto fresh = [&]() { sh.lds.assign(kAlnLdsBytes + kGuard, (char)0x5a); };
  auto guard_ok = [&]() {
    for (size_t i = kAlnLdsBytes; i < sh.lds.size(); ++i)
      if (sh.lds[i] != (char)0x5a) return false;
    return true;
  };
  const AlnShape shape = alntext_shape(&job, 0);
  for (uint32_t k = 0; k < coltiles; ++k) sh.run([&](uint32_t l) { HostWave w{l, &sh}; alntext_letters_body(w, a, k); });
  for (uint32_t k = 0; k < tiles; ++k) {
    fresh();
    sh.run([&](uint32_t l) { HostWave w{l, &sh}; alntext_count_body(w, a, k); });
    const AlnTileAt at = aln_locate(shape, k);
    if (at.sec != AS_CHECK && bytes[k] > (at.i1 - at.i0) * kAlnMaxItem) return 1;
  }
  fresh();
  sh.run([&](uint32_t l) { HostWave w{l, &sh}; alntext_scan_body(w, a, 0); });
  if (text)
    for (uint32_t k = 0; k < tiles; ++k) {
      fresh();
      sh.run([&](uint32_t l) { HostWave w{l, &sh}; alntext_emit_body(w, a, k); });
      if (!guard_ok()) return 1;
    }
  out2[0] = out.status; out2[1] = (int32_t)out.text_len;
  for (size_t i = tiles; i < bytes.size(); ++i)
    if (bytes[i] != stale) return 2;
  for (size_t i = 2 * (size_t)tiles; i < aux.size(); ++i)
    if (aux[i] != stale) return 2;
  for (size_t i = 2 * (size_t)coltiles; i < letters.size(); ++i)
    if (letters[i] != stale) return 2;
  return 0;
}

// One slice of `len` bytes from `begin` of the oriented reference, written at out.
void emu_slice(const uint8_t* ref, uint32_t ref_len, uint8_t forward, uint32_t begin, uint32_t len, uint8_t* out) {
  SliceDesc d{};
  d.ref_len = ref_len; d.begin = begin; d.len = len; d.forward = forward;
  SliceArgs a{};
  a.refs = ref; a.out = out; a.sl = &d; a.n = 1; a.ntiles = slice_tiles(len);
  WaveShared sh;
  for (uint32_t k = 0; k < a.ntiles; ++k) sh.run([&](uint32_t l) { HostWave w{l, &sh}; slice_body(w, a, k); });
}
}
