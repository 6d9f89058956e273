// dcptext_plan.h -- the HIP-free part of the host side of tracyhip_render_decompositions (dcptext.hip): what is refused before a device is
// touched, the upper bound of a trace's text, the cut of a batch into chunks of consecutive traces whose staged bytes and tile scratch
// fit a limit, and the descriptors of a chunk.  The spans, the 64-bit test and the staging layout are ragged_plan.h's.
// tests/cpp/dcptext_plan.cpp runs it under the sanitizers.
#ifndef TRACY_AMD_DCPTEXT_PLAN_H
#define TRACY_AMD_DCPTEXT_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/tracy_hip.h"
#include "dcptext_wave.h"
#include "ragged_plan.h"

namespace tracyhip {

inline bool dcptext_reads_table(uint32_t form) { return form != TRACYHIP_DCPTEXT_VCF; }
inline bool dcptext_reads_calls(uint32_t form) { return form != TRACYHIP_DCPTEXT_DECOMP; }  // basecalls, variants, names, strands, trims

// null: the job may run; else why not (tracyhip_render_decompositions_validate).  *range: the reason is a size out of range
// (TRACYHIP_ERR_RANGE), of trace *bad_t where it is a trace's
inline const char* dcptext_validate(const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out, bool* range, uint32_t* bad_t) {
  *range = false;
  *bad_t = 0;
  if (!job || !out) return "null job / result";
  if (mem != TRACYHIP_MEM_HOST && mem != TRACYHIP_MEM_DEVICE) return "bad mem";
  if (job->form != TRACYHIP_DCPTEXT_DECOMP && job->form != TRACYHIP_DCPTEXT_JSON && job->form != TRACYHIP_DCPTEXT_VCF) return "bad form";
  const bool table = dcptext_reads_table(job->form), calls = dcptext_reads_calls(job->form), json = job->form == TRACYHIP_DCPTEXT_JSON;
  if (calls) {
    *range = true;
    if (job->max_variants < 1 || job->max_variants > kDcpMaxVariants) return "max_variants must be 1 .. 1024";
    if (job->max_text < 2 || job->max_text > kDcpMaxText) return "max_text must be 2 .. 2^19";
    *range = false;
  }
  if (job->n == 0) return nullptr;
  if (table) {
    if (!job->dcp_indel || !job->dcp_err || !job->dcp_offset || !job->dcp_rows) return "null dcp_indel / dcp_err / dcp_offset / dcp_rows";
    if ((reinterpret_cast<uintptr_t>(job->dcp_indel) | reinterpret_cast<uintptr_t>(job->dcp_err)) & 3u) return "misaligned dcp_indel / dcp_err";
  }
  if (calls) {
    if (!job->bcpos || !job->estqual || !job->bc_offset || !job->bc_len) return "null bcpos / estqual / bc_offset / bc_len";
    if (!job->var || !job->var_text || !job->var_n) return "null var / var_text / var_n";
    if ((reinterpret_cast<uintptr_t>(job->bcpos) | reinterpret_cast<uintptr_t>(job->var) | reinterpret_cast<uintptr_t>(job->var_n)) & 3u)
      return "misaligned bcpos / var / var_n";
    if (!job->forward || !job->trim_left || !job->trim_right) return "null forward / trim_left / trim_right";
    if (!job->names || !job->chr_offset[0] || !job->chr_len[0]) return "null names / chr_offset[0] / chr_len[0]";
  }
  if (json) {
    for (int k = 0; k < 3; ++k)
      if (!job->rows0[k] || !job->rows1[k] || !job->rows_offset[k] || !job->cols[k] || !job->score[k]) return "null rows0 / rows1 / rows_offset / cols / score of an alignment";
    if (!job->ref_pos[0] || !job->ref_pos[1] || !job->breakpoint || !job->indelshift) return "null ref_pos / breakpoint / indelshift";
    if (!job->chr_offset[1] || !job->chr_len[1] || !job->frac_offset[0] || !job->frac_len[0] || !job->frac_offset[1] || !job->frac_len[1])
      return "null chr_offset[1] / chr_len[1] / frac_offset / frac_len";
  }
  if (!out->status || !out->text_len) return "null per-trace result array (status, text_len)";
  if (out->text && (!out->text_offset || !out->text_cap)) return "result text without text_offset / text_cap";
  if (table)
    for (uint32_t t = 0; t < job->n; ++t)
      if (job->dcp_rows[t] > kDcpMaxRows) { *range = true; *bad_t = t; return "a decomposition table of more than 2^22 rows"; }
  return nullptr;
}

// an upper bound of text_len of a trace of these sizes, whatever its bytes and numbers (tracyhip_render_decompositions_bound); 0 for a
// form that does not exist.  Beyond the answered domain it is still a number, and means nothing.
inline uint64_t dcptext_bound(uint32_t form, const tracyhip_dcptext_shape& h) {
  const uint64_t rows = h.dcp_rows, nv = h.max_variants, chr1 = h.chr_len[0];
  const uint64_t refalt = 2ull * h.max_text;  // of one record: each of the two stays inside the region
  switch (form) {
    case kDcpDecomp: return 13 + rows * (11 + 1 + 11 + 1);
    case kDcpVcf:  // chr \t pos \t . \t ref \t alt \t qual \t LowQual \t TYPE=Insertion;METHOD=EMBL.TRACYv0.9.1;BASEPOS=..;SIGNALPOS=.. \t GT:GQ \t 0/1:255 \n
      return nv * (chr1 + 1 + 11 + 3 + refalt + 2 + 3 + 1 + 8 + 5 + 9 + 32 + 10 + 11 + 11 + 7 + 3 + 1 + 3 + 1);
    case kDcpJson: {
      const uint64_t head = 2 + 50 + 11 + 2 + 11 + 9;                          // ",\n" chartConfig with two numbers
      const uint64_t allele = 11 + 3 + 11 + 10 + 3 + 14 + 3 + 14 + 3 + 15 + 1 + 3 + 15 + 11 + 3;  // the six lines of an allele without chr and rows
      const uint64_t fractions = 19 + 3 + 17 + 3 + 19 + 3 + 17 + 3 + 15 + 11 + 3 + 12 + 1 + 3;     // allele1fraction .. hetindel
      const uint64_t lists = 19 + 6 + 2 * rows * 13 + 10 + 2 + 3;              // "decomposition": {\n"x": [ .. ],\n"y": [ .. ]\n},\n
      const uint64_t vhead = 15 + 124 + 11;                                    // "variants": {\n, the columns line, "rows": [\n
      const uint64_t vrow = 2 + 2 + chr1 + 3 + 11 + 9 + refalt + 4 + 3 + 3 + 2 + 11 + 1 + 9 + 4 + 8 + 3 + 10 + 2 + 11 + 1;
      const uint64_t xrange = 2 + 1 + 11 + 2 + 11 + 1;
      return head + 2 * allele + chr1 + h.chr_len[1] + 2ull * h.cols[0] + 2ull * h.cols[1] + 2ull * h.cols[2] + fractions + h.frac_len[0] + h.frac_len[1] +
             lists + vhead + nv * (vrow + xrange) + 16 + 8;
    }
    default: return 0;
  }
}

struct DcpChunk {
  uint32_t t0 = 0, t1 = 0;
  Span dcp, rows[3], bc, names, text;  // elements of the tables and of the basecalls, bytes of rows0[k] (and rows1[k]), names and text
  Span var;                            // places of var / var_text / var_n
  uint64_t tiles = 0;
};
constexpr uint64_t kDcpMaxChunkTiles = 1ull << 30;  // tile numbers are 32-bit on the device

inline uint32_t dcptext_trim16(const uint32_t* a, uint32_t t) { return a[t] & 0xffffu; }
inline void dcptext_sizes(const tracyhip_dcptext_job* job, uint32_t t, uint32_t cols[3], uint32_t name_len[4]) {
  const bool json = job->form == TRACYHIP_DCPTEXT_JSON, calls = dcptext_reads_calls(job->form);
  for (int k = 0; k < 3; ++k) cols[k] = json ? job->cols[k][t] : 0u;
  name_len[DN_CHR1] = calls ? job->chr_len[0][t] : 0u;
  name_len[DN_CHR2] = json ? job->chr_len[1][t] : 0u;
  name_len[DN_FRAC1] = json ? job->frac_len[0][t] : 0u;
  name_len[DN_FRAC2] = json ? job->frac_len[1][t] : 0u;
}
inline uint64_t dcptext_name_off(const tracyhip_dcptext_job* job, uint32_t t, uint32_t k) {
  const bool json = job->form == TRACYHIP_DCPTEXT_JSON;
  if (k == DN_CHR1 || !json) return job->chr_offset[0][t];  // (a name that is not read: no bytes at a place that is)
  return k == DN_CHR2 ? job->chr_offset[1][t] : job->frac_offset[k - DN_FRAC1][t];
}
inline uint32_t dcptext_var_index(const tracyhip_dcptext_job* job, uint32_t t) { return job->var_index ? job->var_index[t] : t; }
inline uint32_t dcptext_bp_index(const tracyhip_dcptext_job* job, uint32_t t) {
  return job->form == TRACYHIP_DCPTEXT_JSON ? dcptext_trim16(job->trim_left, t) + job->breakpoint[t] : 0u;
}
inline bool dcptext_answerable(const tracyhip_dcptext_job* job, uint32_t t) {
  uint32_t cols[3], nl[4];
  dcptext_sizes(job, t, cols, nl);
  return dcp_answerable(job->form, cols, dcptext_reads_calls(job->form) ? job->bc_len[t] : 0u, nl, dcptext_bp_index(job, t));
}
inline DcpShape dcptext_shape(const tracyhip_dcptext_job* job, uint32_t t) {
  uint32_t cols[3], nl[4];
  dcptext_sizes(job, t, cols, nl);
  return DcpShape{job->form, dcptext_reads_table(job->form) ? job->dcp_rows[t] : 0u, {cols[0], cols[1], cols[2]}, job->max_variants};
}
inline uint32_t dcptext_tiles(const tracyhip_dcptext_job* job, uint32_t t) { return dcptext_answerable(job, t) ? dcp_tiles(dcptext_shape(job, t)) : 0u; }

// what a chunk stages (host payloads) and holds as scratch, in bytes
inline uint64_t dcptext_chunk_bytes(const tracyhip_dcptext_job* job, const DcpChunk& c, bool host, bool payload) {
  uint64_t b = c.tiles * 8;
  if (!host) return b;
  b += 8 * c.dcp.size() + 2 * (c.rows[0].size() + c.rows[1].size() + c.rows[2].size()) + 5 * c.bc.size() + c.names.size();
  if (dcptext_reads_calls(job->form)) b += c.var.size() * (sizeof(tracyhip_variant) * job->max_variants + job->max_text + 4ull);
  if (payload) b += c.text.size();
  return b;
}
// false: an offset + length of trace *bad_t leaves 64 bits
inline bool dcptext_cut_chunks(const tracyhip_dcptext_job* job, const tracyhip_dcptext_result* out, bool host, uint64_t limit,
                               std::vector<DcpChunk>& chunks, uint32_t* bad_t) {
  const bool payload = out->text != nullptr, table = dcptext_reads_table(job->form), calls = dcptext_reads_calls(job->form);
  const bool json = job->form == TRACYHIP_DCPTEXT_JSON;
  return cut_spans(
      job->n, limit, chunks, bad_t,
      [=](uint32_t t) {
        uint32_t cols[3], nl[4];
        dcptext_sizes(job, t, cols, nl);
        if (table && !offset_fits(job->dcp_offset[t], job->dcp_rows[t])) return false;
        if (calls && !offset_fits(job->bc_offset[t], job->bc_len[t])) return false;
        for (uint32_t k = 0; json && k < 3; ++k)
          if (!offset_fits(job->rows_offset[k][t], cols[k])) return false;
        for (uint32_t k = 0; calls && k < 4; ++k)
          if (!offset_fits(dcptext_name_off(job, t, k), nl[k])) return false;
        return !payload || offset_fits(out->text_offset[t], out->text_cap[t]);
      },
      [=](DcpChunk& c, uint32_t t) {
        uint32_t cols[3], nl[4];
        dcptext_sizes(job, t, cols, nl);
        if (table) c.dcp.add(job->dcp_offset[t], job->dcp_rows[t]);
        if (calls) c.bc.add(job->bc_offset[t], job->bc_len[t]);
        if (calls) c.var.add(dcptext_var_index(job, t), 1);
        for (uint32_t k = 0; json && k < 3; ++k) c.rows[k].add(job->rows_offset[k][t], cols[k]);
        for (uint32_t k = 0; calls && k < 4; ++k) c.names.add(dcptext_name_off(job, t, k), nl[k]);
        if (payload) c.text.add(out->text_offset[t], out->text_cap[t]);
        c.tiles += dcptext_tiles(job, t);
      },
      [=](const DcpChunk& c, uint64_t lim) { return dcptext_chunk_bytes(job, c, host, payload) > lim || c.tiles > kDcpMaxChunkTiles; });
}

// the descriptor of trace t of chunk c: host payloads are staged from each span's first element (the variants from the chunk's first
// place), device payloads used in place
inline DcpDesc dcptext_desc(const tracyhip_dcptext_job* job, const tracyhip_dcptext_result* out, const DcpChunk& c, bool host, uint32_t t,
                            uint32_t tile_first) {
  const bool table = dcptext_reads_table(job->form), calls = dcptext_reads_calls(job->form), json = job->form == TRACYHIP_DCPTEXT_JSON;
  DcpDesc d{};
  uint32_t cols[3], nl[4];
  dcptext_sizes(job, t, cols, nl);
  if (table) { d.dcp_off = job->dcp_offset[t] - (host ? c.dcp.lo : 0); d.dcp_rows = job->dcp_rows[t]; }
  for (uint32_t k = 0; k < 3; ++k) {
    d.cols[k] = cols[k];
    if (json) { d.rows_off[k] = job->rows_offset[k][t] - (host ? c.rows[k].lo : 0); d.score[k] = job->score[k][t]; }
  }
  for (uint32_t k = 0; k < 4; ++k) {
    d.name_len[k] = nl[k];
    if (calls) d.name_off[k] = dcptext_name_off(job, t, k) - (host ? c.names.lo : 0);
  }
  if (calls) {
    d.bc_off = job->bc_offset[t] - (host ? c.bc.lo : 0); d.bc_len = job->bc_len[t];
    d.trim_l = dcptext_trim16(job->trim_left, t); d.trim_r = dcptext_trim16(job->trim_right, t);
    d.var_slot = dcptext_var_index(job, t) - (host ? (uint32_t)c.var.lo : 0u);
  }
  if (json) { d.ref_pos[0] = job->ref_pos[0][t]; d.ref_pos[1] = job->ref_pos[1][t]; }
  d.bp_index = dcptext_bp_index(job, t);
  d.text_off = out->text ? out->text_offset[t] - (host ? c.text.lo : 0) : 0;
  d.text_cap = out->text ? out->text_cap[t] : 0;
  d.tile_first = tile_first;
  d.flags = (dcptext_answerable(job, t) ? kDcpAnswerable : 0u) | (calls && job->forward[t] ? kDcpForward : 0u) |
            (json && job->indelshift[t] ? kDcpIndelShift : 0u);
  return d;
}

}  // namespace tracyhip
#endif
