// alntext_plan.h -- the HIP-free part of the host side of tracyhip_render_alignments and tracyhip_reference_slices (alntext.hip): what is
// refused before a device is touched, the upper bound of an alignment's text, the cut of a batch into chunks of consecutive alignments
// whose staged bytes and tile scratch fit a limit, and the descriptors of a chunk.  The spans, the 64-bit test and the staging layout are
// ragged_plan.h's.  tests/cpp/alntext_plan.cpp runs it under the sanitizers.
#ifndef TRACY_AMD_ALNTEXT_PLAN_H
#define TRACY_AMD_ALNTEXT_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tracy_hip.h"
#include "alntext_wave.h"
#include "ragged_plan.h"

namespace tracyhip {

// null: the job may run; else why not (tracyhip_render_alignments_validate)
inline const char* alntext_validate(const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out) {
  if (!job || !out) return "null job / result";
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return "bad mem";
  if (job->form != TRACYHIP_ALNTEXT_PLOT && job->form != TRACYHIP_ALNTEXT_FASTA && job->form != TRACYHIP_ALNTEXT_JSON) return "bad form";
  if (job->form == TRACYHIP_ALNTEXT_PLOT) {
    if (job->key > 3) return "key must be 0 .. 3";
    if (job->linelimit < 1 || job->linelimit > kAlnMaxLine) return "linelimit must be 1 .. 65535";
  }
  if (job->n == 0) return nullptr;
  if (!job->rows0 || !job->rows1 || !job->rows_offset || !job->cols) return "null rows0 / rows1 / rows_offset / cols";
  if (!job->names || !job->name1_offset || !job->name1_len) return "null names / name1_offset / name1_len";
  if (job->form != TRACYHIP_ALNTEXT_JSON && (!job->name0_offset || !job->name0_len)) return "null name0_offset / name0_len";
  if (!job->ref_pos || !job->ref_len || !job->forward) return "null ref_pos / ref_len / forward";
  if (job->form == TRACYHIP_ALNTEXT_PLOT && !job->score) return "the plot prints the score: null score";
  if (!out->status || !out->text_len) return "null per-alignment result array (status, text_len)";
  if (out->text && (!out->text_offset || !out->text_cap)) return "result text without text_offset / text_cap";
  return nullptr;
}

// an upper bound of text_len of an alignment of these sizes, whatever its bytes and numbers (tracyhip_render_alignments_bound); 0 for
// a form that does not exist or a plot whose linelimit does.  Beyond the answered domain it is still a number, and means nothing.
inline uint64_t alntext_bound(uint32_t form, uint32_t linelimit, uint32_t cols, uint32_t name0_len, uint32_t name1_len) {
  const uint64_t c = cols, n0 = name0_len, n1 = name1_len;
  switch (form) {
    case kAlnPlot: {
      if (linelimit < 1 || linelimit > kAlnMaxLine) return 0;
      const uint64_t fald = (uint64_t)linelimit + 14, blocks = (c + linelimit - 1) / linelimit;
      const uint64_t ungapped = c + c / fald + 1;          // every column a letter, a break per full line, the closing one
      const uint64_t score = 18 + 11 + 1;                  // "\nAlignment score: " + "-2147483648" + '\n'
      const uint64_t per_block = 15 + 14 + 15 + 4;         // "Alt1" + ten digits + ' ', the bar indent, the same for "Alt2", four '\n'
      return n0 + 1 + n1 + 1 + 2 * ungapped + score + 3 * (fald + 1) + 1 + blocks * per_block + 3 * c + 24 + 2;
    }
    case kAlnFasta: return 1 + n0 + 1 + c + 1 + 1 + n1 + 11 + c + 1;
    case kAlnJson: return 14 + n1 + 13 + 10 + 15 + c + 17 + c + 19;
    default: return 0;
  }
}

struct AlnChunk {
  uint32_t t0 = 0, t1 = 0;
  Span rows, names, text;  // bytes of rows0 (and of rows1), of the names and of the result text
  uint64_t tiles = 0, coltiles = 0;
};
constexpr uint64_t kAlnMaxChunkTiles = 1ull << 30;  // tile numbers are 32-bit on the device

inline uint32_t alntext_name0_len(const tracyhip_alntext_job* job, uint32_t t) { return job->form == TRACYHIP_ALNTEXT_JSON ? 0u : job->name0_len[t]; }
inline uint64_t alntext_name0_off(const tracyhip_alntext_job* job, uint32_t t) { return job->form == TRACYHIP_ALNTEXT_JSON ? job->name1_offset[t] : job->name0_offset[t]; }
inline bool alntext_answerable(const tracyhip_alntext_job* job, uint32_t t) {
  return aln_answerable(job->cols[t], alntext_name0_len(job, t), job->name1_len[t], job->ref_pos[t], job->ref_len[t]);
}
inline AlnShape alntext_shape(const tracyhip_alntext_job* job, uint32_t t) {
  return AlnShape{job->form, job->form == TRACYHIP_ALNTEXT_PLOT ? job->linelimit : 1u, job->cols[t], alntext_name0_len(job, t), job->name1_len[t]};
}
inline uint32_t alntext_tiles(const tracyhip_alntext_job* job, uint32_t t) { return alntext_answerable(job, t) ? aln_tiles(alntext_shape(job, t)) : 0u; }
// column tiles: the letters of a plot's rows are counted per kAlnTile columns
inline uint32_t alntext_coltiles(const tracyhip_alntext_job* job, uint32_t t) {
  return job->form == TRACYHIP_ALNTEXT_PLOT && alntext_answerable(job, t) ? aln_tiles_of(job->cols[t]) : 0u;
}
// what a chunk stages (host payloads) and holds as scratch, in bytes
inline uint64_t alntext_chunk_bytes(const AlnChunk& c, bool host, bool payload) {
  uint64_t b = c.tiles * 12 + c.coltiles * 8;
  if (!host) return b;
  b += 2 * c.rows.size() + c.names.size();
  if (payload) b += c.text.size();
  return b;
}
// false: an offset + length of alignment *bad_t leaves 64 bits
inline bool alntext_cut_chunks(const tracyhip_alntext_job* job, const tracyhip_alntext_result* out, bool host, uint64_t limit,
                               std::vector<AlnChunk>& chunks, uint32_t* bad_t) {
  const bool payload = out->text != nullptr;
  return cut_spans(
      job->n, limit, chunks, bad_t,
      [=](uint32_t t) {
        return offset_fits(job->rows_offset[t], job->cols[t]) && offset_fits(alntext_name0_off(job, t), alntext_name0_len(job, t)) &&
               offset_fits(job->name1_offset[t], job->name1_len[t]) && (!payload || offset_fits(out->text_offset[t], out->text_cap[t]));
      },
      [=](AlnChunk& c, uint32_t t) {
        c.rows.add(job->rows_offset[t], job->cols[t]);
        c.names.add(alntext_name0_off(job, t), alntext_name0_len(job, t));
        c.names.add(job->name1_offset[t], job->name1_len[t]);
        if (payload) c.text.add(out->text_offset[t], out->text_cap[t]);
        c.tiles += alntext_tiles(job, t);
        c.coltiles += alntext_coltiles(job, t);
      },
      [=](const AlnChunk& c, uint64_t lim) { return alntext_chunk_bytes(c, host, payload) > lim || c.tiles > kAlnMaxChunkTiles; });
}

// the descriptor of alignment t of chunk c: host payloads are staged from each span's first byte, device payloads used in place
inline AlnDesc alntext_desc(const tracyhip_alntext_job* job, const tracyhip_alntext_result* out, const AlnChunk& c, bool host, uint32_t t,
                            uint32_t tile_first, uint32_t col_first) {
  AlnDesc d{};
  d.rows_off = job->rows_offset[t] - (host ? c.rows.lo : 0);
  d.name0_off = alntext_name0_off(job, t) - (host ? c.names.lo : 0);
  d.name1_off = job->name1_offset[t] - (host ? c.names.lo : 0);
  d.text_off = out->text ? out->text_offset[t] - (host ? c.text.lo : 0) : 0;
  d.text_cap = out->text ? out->text_cap[t] : 0;
  d.cols = job->cols[t]; d.name0_len = alntext_name0_len(job, t); d.name1_len = job->name1_len[t];
  d.ref_len = job->ref_len[t]; d.ref_pos = job->ref_pos[t]; d.score = job->score ? job->score[t] : 0;
  d.tile_first = tile_first; d.col_first = col_first;
  d.flags = (alntext_answerable(job, t) ? kAlnAnswerable : 0u) | (job->forward[t] ? kAlnForward : 0u);
  return d;
}

// ---- tracyhip_reference_slices ----
// null: the job may run; else why not.  *range: the reason is a slice beyond its reference (TRACYHIP_ERR_RANGE)
inline const char* slices_validate(const tracyhip_slices_job* job, int mem, const uint8_t* out, const uint64_t* out_offset, bool* range, uint32_t* bad_t) {
  *range = false;
  *bad_t = 0;
  if (!job) return "null job";
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return "bad mem";
  if (job->refs.kind != TRACYHIP_SEQ_CHAR) return "refs must be of kind CHAR";
  if (job->n == 0) return nullptr;
  if (!job->refs.data || !job->refs.offset || !job->refs.length) return "null refs.data / offset / length";
  if (!job->forward || !job->slice_begin || !job->slice_len) return "null forward / slice_begin / slice_len";
  if (!out || !out_offset) return "null out / out_offset";
  for (uint32_t t = 0; t < job->n; ++t) {
    const uint32_t r = job->ref_index ? job->ref_index[t] : t;
    *bad_t = t;
    if (r >= job->refs.count) return "a reference index beyond refs.count";
    if ((uint64_t)job->slice_begin[t] + job->slice_len[t] > job->refs.length[r]) { *range = true; return "slice_begin + slice_len beyond the reference"; }
    if (!offset_fits(job->refs.offset[r], job->refs.length[r]) || !offset_fits(out_offset[t], job->slice_len[t])) {
      *range = true;
      return "an offset + length leaves 64 bits";
    }
  }
  return nullptr;
}
inline uint32_t slice_tiles(uint32_t len) { return (len + kSliceTile - 1) / kSliceTile; }

}  // namespace tracyhip
#endif
