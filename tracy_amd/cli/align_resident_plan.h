// align_resident_plan.h -- the layout of one block of `align --batch --resident` (align_resident.inc), free of HIP and of the C ABI: which
// lines of the block the device chain may answer, the entries it reads (every line, then one more per distinct wildtype trace), where each
// entry's file bytes, chromatogram, calls and profile lie in their payloads, the split of the answered lines by reference kind with the
// shared references behind ref_index, the regions of the op strings / rows, reference slices, padded traces and names, and where every
// text fragment of every output file lies in the buffer that is copied back.  Offsets are 64-bit element offsets; a block whose totals
// leave 64 bits is refused (every layout_* returns false and leaves the plan unusable).  tests/cpp/align_resident_plan.cpp runs it plain
// and under the sanitizers.
//
// The order of use (one stage of the chain between two steps):
//   split_references   kind and path of every line's reference            -> the distinct FASTA files / wildtype traces, ref_of
//   layout_entries     file lengths and read capacities of the entries    -> file_off, sample_off, call_off (profiles: 6 * call_off)
//   open_rows          what read + basecall answered, the trims           -> rows: the lines still answered, by kind, compact ref_index
//   layout_ops         calls of a row and columns of its reference        -> ops_off / ops_cap (op strings and both alignment rows)
//   layout_slices      slice lengths of the FASTA rows
//   layout_pad         padded sizes                                       -> pad_sample_off / pad_call_off
//   layout_names       stem, the plot's second header line, rs.chr        -> names payload (the first header line is shared)
//   layout_text        the text lengths of a row                          -> text_off[f][k], fragments of a row in file order: a file is one span
// keep(ok) between the steps drops the rows a stage did not answer; a dropped row keeps its regions (they are never read again) and gets
// no text.
#ifndef TRACY_AMD_ALIGN_RESIDENT_PLAN_H
#define TRACY_AMD_ALIGN_RESIDENT_PLAN_H

#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace tracy_amd {
namespace resident {

constexpr uint32_t kBlockLines = 2048;  // lines whose files, chromatograms and text are resident together (the basecall chain's block)
constexpr uint32_t kNone = 0xffffffffu;

// genomeType's answers (sage_out.hpp)
enum RefKind : int32_t { REF_UNKNOWN = -1, REF_GENOME = 0, REF_FASTA = 1, REF_WILDTYPE = 2 };

// the text fragments of a row, in the order they lie in the copy-back buffer: <prefix>.abif, <prefix>.align.fa, <prefix>.txt, then
// <prefix>.json in its five parts -- the host's opening lines (up to trailingGaps), the device's gapped trace, the host's closing "}\n"
// of it, the device's tail.  The device renders its fragments where they lie and the host fills in its two after the copy back, so every
// file is one span of the buffer and is written from there.
enum Fragment : uint32_t { FRAG_ABIF = 0, FRAG_FASTA = 1, FRAG_PLOT = 2, FRAG_JSON_HEAD = 3, FRAG_GAPPED = 4, FRAG_JSON_CLOSE = 5, FRAG_TAIL = 6, FRAG_COUNT = 7 };
enum OutFile : uint32_t { FILE_ABIF = 0, FILE_FASTA = 1, FILE_PLOT = 2, FILE_JSON = 3, FILE_COUNT = 4 };
constexpr Fragment kFileFirst[FILE_COUNT] = {FRAG_ABIF, FRAG_FASTA, FRAG_PLOT, FRAG_JSON_HEAD};
constexpr Fragment kFileLast[FILE_COUNT] = {FRAG_ABIF, FRAG_FASTA, FRAG_PLOT, FRAG_TAIL};

// acc += by unless the sum leaves 64 bits
inline bool add64(uint64_t& acc, uint64_t by) {
  if (by > UINT64_MAX - acc) return false;
  acc += by;
  return true;
}
inline bool mul64(uint64_t a, uint64_t b, uint64_t& out) {
  if (a != 0 && b > UINT64_MAX / a) return false;
  out = a * b;
  return true;
}
// off[i] = sum of per[0 .. i) * scale, off[n] the total; false when a partial sum, or the total times `bytes`, leaves 64 bits
template <class Len>
inline bool prefix_offsets(std::vector<Len> const& per, uint64_t scale, uint64_t bytes, std::vector<uint64_t>& off) {
  off.assign(per.size() + 1, 0);
  for (std::size_t i = 0; i < per.size(); ++i) {
    uint64_t room = 0;
    if (!mul64((uint64_t)per[i], scale, room)) return false;
    off[i + 1] = off[i];
    if (!add64(off[i + 1], room)) return false;
  }
  uint64_t total = 0;
  return mul64(off[per.size()], bytes, total);
}

struct BlockPlan {
  // ---- split_references ----
  uint32_t nlines = 0;
  std::vector<int32_t> kind;           // [nlines] RefKind
  std::vector<uint32_t> ref_of;        // [nlines] the line's distinct FASTA (REF_FASTA) or distinct wildtype (REF_WILDTYPE) of the block, else kNone
  std::vector<uint32_t> fasta_line;    // [nfasta] the first line that names distinct FASTA f (its path)
  std::vector<uint32_t> wildtype_line; // [nwildtypes] likewise
  uint32_t nfasta() const { return (uint32_t)fasta_line.size(); }
  uint32_t nwildtypes() const { return (uint32_t)wildtype_line.size(); }
  // entries: line i is entry i, distinct wildtype w is entry nlines + w
  uint32_t nentries() const { return nlines + nwildtypes(); }
  uint32_t wildtype_entry(uint32_t w) const { return nlines + w; }

  void split_references(std::vector<int32_t> const& kinds, std::vector<std::string> const& ref_paths) {
    nlines = (uint32_t)kinds.size();
    kind = kinds;
    ref_of.assign(nlines, kNone);
    fasta_line.clear();
    wildtype_line.clear();
    std::map<std::string, uint32_t> seen[2];
    for (uint32_t i = 0; i < nlines; ++i) {
      if (kind[i] != REF_FASTA && kind[i] != REF_WILDTYPE) continue;
      const int w = kind[i] == REF_WILDTYPE;
      std::vector<uint32_t>& first = w ? wildtype_line : fasta_line;
      auto it = seen[w].find(ref_paths[i]);
      if (it == seen[w].end()) {
        it = seen[w].emplace(ref_paths[i], (uint32_t)first.size()).first;
        first.push_back(i);
      }
      ref_of[i] = it->second;
    }
  }

  // ---- layout_entries: lengths 0 for an entry the chain does not read (no usable reference, a file that could not be read) ----
  std::vector<uint32_t> file_len, sample_cap, call_cap;  // [nentries]
  std::vector<uint64_t> file_off, sample_off, call_off;  // [nentries + 1]: bytes; samples (four channels of sample_cap each); calls
  uint64_t profile_off(uint32_t e) const { return 6 * call_off[e]; }  // floats: tracyhip_basecall_result::profiles

  bool layout_entries(std::vector<uint32_t> const& flen, std::vector<uint32_t> const& scap, std::vector<uint32_t> const& ccap) {
    if (flen.size() != nentries() || scap.size() != flen.size() || ccap.size() != flen.size()) return false;
    file_len = flen; sample_cap = scap; call_cap = ccap;
    return prefix_offsets(file_len, 1, 1, file_off) && prefix_offsets(sample_cap, 4, 4, sample_off) &&
           prefix_offsets(call_cap, 1, 24, call_off);  // (24: a profile column, the widest per-call payload)
  }

  // ---- open_rows: row k is line row_line[k]; the rows keep manifest order ----
  std::vector<uint32_t> row_line;      // [nrows]
  std::vector<uint32_t> row_of_line;   // [nlines] or kNone
  std::vector<uint8_t> alive;          // [nrows] still answered by the chain
  std::vector<uint32_t> fasta_rows, wildtype_rows;  // rows by reference kind, ascending: the two align calls
  std::vector<uint32_t> fasta_used, wildtype_used;  // the distinct references those rows name, compact, in order of first use
  std::vector<uint32_t> fasta_ref_index, wildtype_ref_index;  // [fasta_rows.size()] / [wildtype_rows.size()]: into *_used
  uint32_t nrows() const { return (uint32_t)row_line.size(); }
  uint32_t nalive() const { uint32_t n = 0; for (uint8_t a : alive) n += a; return n; }

  // entry_ok: read and basecalled by the device (nentries); bc_len (nentries); trims (nlines); fasta_ok: loaded and short enough (nfasta)
  void open_rows(std::vector<uint8_t> const& entry_ok, std::vector<uint32_t> const& bc_len, std::vector<uint32_t> const& trim_l,
                 std::vector<uint32_t> const& trim_r, std::vector<uint8_t> const& fasta_ok) {
    row_line.clear(); fasta_rows.clear(); wildtype_rows.clear(); fasta_used.clear(); wildtype_used.clear();
    fasta_ref_index.clear(); wildtype_ref_index.clear();
    row_of_line.assign(nlines, kNone);
    std::vector<uint32_t> slot[2] = {std::vector<uint32_t>(nfasta(), kNone), std::vector<uint32_t>(nwildtypes(), kNone)};
    for (uint32_t i = 0; i < nlines; ++i) {
      if (ref_of[i] == kNone || !entry_ok[i] || bc_len[i] == 0) continue;
      if ((uint64_t)trim_l[i] + trim_r[i] >= bc_len[i]) continue;  // the trims take all of it
      const int w = kind[i] == REF_WILDTYPE;
      if (w) {
        const uint32_t e = wildtype_entry(ref_of[i]);
        if (!entry_ok[e] || bc_len[e] == 0) continue;
      } else if (!fasta_ok[ref_of[i]]) continue;
      const uint32_t k = nrows();
      row_line.push_back(i);
      row_of_line[i] = k;
      std::vector<uint32_t>& used = w ? wildtype_used : fasta_used;
      if (slot[w][ref_of[i]] == kNone) { slot[w][ref_of[i]] = (uint32_t)used.size(); used.push_back(ref_of[i]); }
      (w ? wildtype_rows : fasta_rows).push_back(k);
      (w ? wildtype_ref_index : fasta_ref_index).push_back(slot[w][ref_of[i]]);
    }
    alive.assign(nrows(), 1);
  }
  // a stage's verdicts: row k stays only where ok[k] != 0
  void keep(std::vector<uint8_t> const& ok) {
    for (uint32_t k = 0; k < nrows(); ++k) alive[k] = alive[k] && ok[k];
  }

  // ---- layout_ops: the op string of row k and each of its two alignment rows own ops_cap[k] bytes from ops_off[k] on ----
  std::vector<uint32_t> ops_cap;   // [nrows] calls + reference columns
  std::vector<uint64_t> ops_off;   // [nrows + 1]
  bool layout_ops(std::vector<uint32_t> const& calls, std::vector<uint32_t> const& ref_cols) {
    if (calls.size() != nrows() || ref_cols.size() != nrows()) return false;
    std::vector<uint64_t> cap(nrows());
    ops_cap.assign(nrows(), 0);
    for (uint32_t k = 0; k < nrows(); ++k) {
      cap[k] = (uint64_t)calls[k] + ref_cols[k];
      if (cap[k] > 0xffffffffull) return false;
      ops_cap[k] = (uint32_t)cap[k];
    }
    return prefix_offsets(cap, 1, 1, ops_off);
  }

  // ---- the distinct FASTA records in use, back to back; the slices of the FASTA rows, back to back ----
  std::vector<uint64_t> fasta_off;  // [fasta_used.size() + 1]
  template <class Len>
  bool layout_fasta(std::vector<Len> const& len_of_used) {
    return len_of_used.size() == fasta_used.size() && prefix_offsets(len_of_used, 1, 1, fasta_off);
  }
  std::vector<uint64_t> slice_off;  // [fasta_rows.size() + 1]
  template <class Len>
  bool layout_slices(std::vector<Len> const& slice_len) {
    return slice_len.size() == fasta_rows.size() && prefix_offsets(slice_len, 1, 1, slice_off);
  }

  // ---- layout_pad: the padded trace of row k (nothing for a row that is no longer answered) ----
  std::vector<uint32_t> pad_sample_cap, pad_call_cap;  // [nrows]
  std::vector<uint64_t> pad_sample_off, pad_call_off;  // [nrows + 1]: samples (four channels), calls
  bool layout_pad(std::vector<uint32_t> const& nsamples_out, std::vector<uint32_t> const& ncalls_out) {
    if (nsamples_out.size() != nrows() || ncalls_out.size() != nrows()) return false;
    pad_sample_cap.assign(nrows(), 0); pad_call_cap.assign(nrows(), 0);
    for (uint32_t k = 0; k < nrows(); ++k)
      if (alive[k]) { pad_sample_cap[k] = nsamples_out[k]; pad_call_cap[k] = ncalls_out[k]; }
    return prefix_offsets(pad_sample_cap, 4, 4, pad_sample_off) && prefix_offsets(pad_call_cap, 1, 4, pad_call_off);
  }

  // ---- layout_names: one payload: the plot's first header line once (shared by every row), then per row the trace stem, the plot's
  // second header line and rs.chr ----
  uint32_t head0_len = 0;
  std::vector<uint64_t> stem_off, head1_off, chr_off;  // [nrows]; the shared first header line lies at 0
  uint64_t names_bytes = 0;
  bool layout_names(uint32_t head0, std::vector<uint32_t> const& stem_len, std::vector<uint32_t> const& head1_len, std::vector<uint32_t> const& chr_len) {
    if (stem_len.size() != nrows() || head1_len.size() != nrows() || chr_len.size() != nrows()) return false;
    head0_len = head0;
    stem_off.assign(nrows(), 0); head1_off.assign(nrows(), 0); chr_off.assign(nrows(), 0);
    uint64_t at = head0;
    for (uint32_t k = 0; k < nrows(); ++k) {
      stem_off[k] = at;
      if (!add64(at, stem_len[k])) return false;
      head1_off[k] = at;
      if (!add64(at, head1_len[k])) return false;
      chr_off[k] = at;
      if (!add64(at, chr_len[k])) return false;
    }
    names_bytes = at;
    return true;
  }

  // ---- layout_text: fragment f of row k is text_cap[f][k] bytes from text_off[f][k] on; a row's fragments follow each other in Fragment
  // order, the rows in row order; a row that is no longer answered has no text ----
  std::vector<uint64_t> text_off[FRAG_COUNT], text_cap[FRAG_COUNT];  // [nrows]
  uint64_t text_bytes = 0;
  bool layout_text(std::vector<uint32_t> const (&len)[FRAG_COUNT]) {
    for (uint32_t f = 0; f < FRAG_COUNT; ++f) {
      if (len[f].size() != nrows()) return false;
      text_off[f].assign(nrows(), 0);
      text_cap[f].assign(nrows(), 0);
    }
    uint64_t at = 0;
    for (uint32_t k = 0; k < nrows(); ++k)
      for (uint32_t f = 0; f < FRAG_COUNT; ++f) {
        text_off[f][k] = at;
        text_cap[f][k] = alive[k] ? len[f][k] : 0;
        if (!add64(at, text_cap[f][k])) return false;
      }
    text_bytes = at;
    return true;
  }
  // file f of row k: out_len(f, k) bytes from out_off(f, k) on
  uint64_t out_off(uint32_t f, uint32_t k) const { return text_off[kFileFirst[f]][k]; }
  uint64_t out_len(uint32_t f, uint32_t k) const { return text_off[kFileLast[f]][k] + text_cap[kFileLast[f]][k] - text_off[kFileFirst[f]][k]; }
};

}  // namespace resident
}  // namespace tracy_amd
#endif
