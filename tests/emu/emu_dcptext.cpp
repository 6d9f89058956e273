// emu_dcptext.cpp -- host execution of the decompose report printing wave bodies (TEST INFRASTRUCTURE ONLY): the same
// tracy_amd/csrc/dcptext_wave.h code the HIP kernels run, on the 64-fiber host wave, tile after tile; the descriptors come from
// tracy_amd/csrc/dcptext_plan.h as dcptext.hip builds them.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tracy_amd/csrc/dcptext_plan.h"
#include "../../tracy_amd/csrc/dcptext_wave.h"

using namespace tracyhip;

#include "host_wave.h"

extern "C" {

uint32_t emu_dcptext_tile() { return kDcpTile; }  // items per tile

// The traces of a job over host arrays, one chunk.  text null: the sizes-only form; else trace t writes from byte text_offset[t] on.
// status / text_len: per trace.  Returns 2 when a body wrote past the tile scratch, 3 when the job is refused by
// tracyhip_render_decompositions_validate's rules or does not make one chunk.
int emu_dcptext(const tracyhip_dcptext_job* job, uint8_t* text, const uint64_t* text_offset, const uint64_t* text_cap, int32_t* status, uint32_t* text_len) {
  tracyhip_dcptext_result res{};
  res.status = status; res.text_len = text_len; res.text = text; res.text_offset = text_offset; res.text_cap = text_cap;
  bool range = false;
  uint32_t bad = 0;
  if (dcptext_validate(job, TRACYHIP_MEM_DEVICE, &res, &range, &bad)) return 3;
  std::vector<DcpChunk> chunks;
  if (!dcptext_cut_chunks(job, &res, false, ~0ull, chunks, &bad) || chunks.size() != 1) return 3;
  const uint32_t n = job->n;
  std::vector<DcpDesc> desc(n);
  uint32_t tiles = 0;
  for (uint32_t t = 0; t < n; ++t) {
    desc[t] = dcptext_desc(job, &res, chunks[0], false, t, tiles);
    tiles += dcptext_tiles(job, t);
  }
  std::vector<DcpOut> out(n, DcpOut{-1, 0xdeadu});
  const uint32_t stale = 0xa5a5a5a5u;  // (stale scratch: the bodies must write what they read)
  std::vector<uint32_t> bytes(tiles + 16, stale), aux(tiles + 16, stale);
  const bool calls = dcptext_reads_calls(job->form);
  DcpArgs a{};
  a.dcp_indel = job->dcp_indel; a.dcp_err = job->dcp_err;
  for (int k = 0; k < 3; ++k) { a.rows0[k] = job->rows0[k]; a.rows1[k] = job->rows1[k]; }
  a.bcpos = job->bcpos; a.estqual = job->estqual;
  a.var = job->var; a.var_text = job->var_text; a.var_n = job->var_n; a.names = job->names;
  a.tr = desc.data(); a.out = out.data(); a.tile_bytes = bytes.data(); a.tile_aux = aux.data(); a.text = text;
  a.n = n; a.ntiles = tiles; a.form = job->form;
  a.qual_cut = job->qual_cut; a.max_variants = calls ? job->max_variants : 1u; a.max_text = calls ? job->max_text : 2u;
  WaveShared sh;
  for (uint32_t k = 0; k < tiles; ++k) sh.run([&](uint32_t l) { HostWave w{l, &sh}; dcptext_count_body(w, a, k); });
  for (uint32_t t = 0; t < n; ++t) sh.run([&](uint32_t l) { HostWave w{l, &sh}; dcptext_scan_body(w, a, t); });
  if (text)
    for (uint32_t k = 0; k < tiles; ++k) sh.run([&](uint32_t l) { HostWave w{l, &sh}; dcptext_emit_body(w, a, k); });
  for (uint32_t t = 0; t < n; ++t) { status[t] = out[t].status; text_len[t] = out[t].text_len; }
  for (size_t i = tiles; i < bytes.size(); ++i)
    if (bytes[i] != stale || aux[i] != stale) return 2;
  return 0;
}
}
