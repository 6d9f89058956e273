// tracy_host_capi.cpp -- C wrappers over tracy_host.hpp + the seeded synthetic workload generator used
// by bench.py and the parity tests.  Host-only library (libtracy_host.so):
// basecalling / profile creation are host stages in the reference too.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/tracy_hip.h"  // tracyhip_dcptext_job, tracyhip_render_result, tracyhip_variant: declarations alone
#include "assemble_out.hpp"
#include "bcf_out.hpp"
#include "indigo_out.hpp"
#include "sage_out.hpp"
#include "seed.hpp"
#include "trace_io.hpp"
#include "tracy_host.hpp"

using namespace tracy_amd;

namespace {

struct SplitMix64 {
  uint64_t s;
  explicit SplitMix64(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return n ? (uint32_t)(next() % n) : 0; }
  double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

const char kBases[4] = {'A', 'C', 'G', 'T'};
inline int base_index(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }
inline char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }

// add a triangular peak (half-width 5 samples) of height amp centred at x
void add_peak(std::vector<int32_t>& ch, int32_t x, double amp) {
  for (int d = -5; d <= 5; ++d) {
    const int32_t i = x + d;
    if (i < 0 || i >= (int32_t)ch.size()) continue;
    ch[i] += (int32_t)(amp * (1.0 - std::abs(d) / 6.0));
  }
}

// One `tracy align` case: a uniform ACGT window of n bases, a trace of mf bases copied from it at a
// random offset (forward or reverse-complement, 1 % substitutions, 0.2 % 1-3 bp indels), rendered as a
// 4-channel chromatogram with 12 samples per base, primary amplitude U[400,1200] and a background peak
// of 5-15 % in another channel.  hetero > 0 adds a second allele (see synth_decompose_case).
void synth_sequence(SplitMix64& rng, uint32_t n, uint32_t mf, std::string& ref, std::string& seq, bool& reverse) {
  ref.resize(n);
  for (uint32_t i = 0; i < n; ++i) ref[i] = kBases[rng.below(4)];
  const uint32_t span = (n > mf + 40) ? n - mf - 40 : 0;
  uint32_t lo = std::min<uint32_t>(500, span / 2);
  const uint32_t start = lo + rng.below(span - 2 * lo + 1);
  reverse = (rng.next() & 1) != 0;
  std::string src = ref.substr(start, std::min<uint32_t>(n - start, mf + 40));
  if (reverse) {
    std::reverse(src.begin(), src.end());
    for (auto& c : src) c = complement(c);
  }
  seq.clear();
  for (size_t i = 0; i < src.size() && seq.size() < mf; ++i) {
    const double u = rng.unit();
    if (u < 0.001) { i += rng.below(3); continue; }                                                  // deletion
    if (u < 0.002) { const uint32_t k = 1 + rng.below(3); for (uint32_t j = 0; j < k; ++j) seq.push_back(kBases[rng.below(4)]); }  // insertion
    if (u > 0.99) seq.push_back(kBases[rng.below(4)]);                                               // substitution
    else seq.push_back(src[i]);
  }
  while (seq.size() < mf) seq.push_back(kBases[rng.below(4)]);
  seq.resize(mf);
}

void render_trace(SplitMix64& rng, std::string const& allele1, std::string const* allele2, double frac1, Trace& tr) {
  const size_t len = allele2 ? std::max(allele1.size(), allele2->size()) : allele1.size();
  const size_t samples = 12 * len + 12;
  tr.traceACGT.assign(4, std::vector<int32_t>(samples, 0));
  tr.basecallpos.resize(len);
  for (size_t j = 0; j < len; ++j) {
    const int32_t x = (int32_t)(6 + 12 * j);
    tr.basecallpos[j] = x;
    const double amp = 400.0 + 800.0 * rng.unit();
    const double bg = amp * (0.05 + 0.10 * rng.unit());
    int used[2] = {-1, -1};
    if (j < allele1.size()) { used[0] = base_index(allele1[j]); add_peak(tr.traceACGT[used[0]], x, allele2 ? amp * frac1 : amp); }
    if (allele2 && j < allele2->size()) { used[1] = base_index((*allele2)[j]); add_peak(tr.traceACGT[used[1]], x, amp * (1.0 - frac1)); }
    int b = (int)rng.below(4);
    while (b == used[0] || b == used[1]) b = (b + 1) & 3;
    add_peak(tr.traceACGT[b], x, bg);
  }
}

}  // namespace

extern "C" {

// flat-array wrappers -----------------------------------------------------------------------------------
size_t tracyhost_basecall(const int32_t* trace, size_t nsamples, const int32_t* basecallpos, size_t npos, float sigratio,
                          char* primary, char* secondary, char* consensus, int32_t* bcpos) {
  Trace tr;
  tr.traceACGT.resize(4);
  for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(trace + k * nsamples, trace + (k + 1) * nsamples);
  tr.basecallpos.assign(basecallpos, basecallpos + npos);
  BaseCalls bc;
  basecall(tr, bc, sigratio);
  const size_t n = bc.primary.size();
  std::memcpy(primary, bc.primary.data(), n);
  std::memcpy(secondary, bc.secondary.data(), n);
  std::memcpy(consensus, bc.consensus.data(), n);
  std::memcpy(bcpos, bc.bcPos.data(), n * sizeof(int32_t));
  return n;
}

int32_t tracyhost_create_profile(const int32_t* trace, size_t nsamples, const int32_t* bcpos, const char* primary,
                                 const char* secondary, size_t nbc, int32_t trimleft, int32_t trimright, float* out) {
  Trace tr;
  tr.traceACGT.resize(4);
  for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(trace + k * nsamples, trace + (k + 1) * nsamples);
  BaseCalls bc;
  bc.bcPos.assign(bcpos, bcpos + nbc);
  bc.primary.assign(primary, nbc);
  bc.secondary.assign(secondary, nbc);
  Profile p;
  createProfile(tr, bc, p, trimleft, trimright);
  std::memcpy(out, p.data(), sizeof(float) * 6 * p.cols);
  return (int32_t)p.cols;
}

char tracyhost_iupac(char a, char b) { return iupac(a, b); }

// basecall + the per-base quality estimate it ends with (abif.h:232-253, 510)
size_t tracyhost_basecall_qual(const int32_t* trace, size_t nsamples, const int32_t* basecallpos, size_t npos, float sigratio,
                               char* primary, char* secondary, char* consensus, int32_t* bcpos, uint8_t* estqual) {
  Trace tr;
  tr.traceACGT.resize(4);
  for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(trace + k * nsamples, trace + (k + 1) * nsamples);
  tr.basecallpos.assign(basecallpos, basecallpos + npos);
  BaseCalls bc;
  basecall(tr, bc, sigratio);
  const size_t n = bc.primary.size();
  std::memcpy(primary, bc.primary.data(), n);
  std::memcpy(secondary, bc.secondary.data(), n);
  std::memcpy(consensus, bc.consensus.data(), n);
  std::memcpy(bcpos, bc.bcPos.data(), n * sizeof(int32_t));
  std::memcpy(estqual, bc.estQual.data(), n);
  return n;
}

// chromatogram files: format 0 = ABIF, 1 = SCF (scf.h:18-34).  The handle owns a Trace.
void* tracyhost_trace_read(const char* path, int32_t* format) {
  const int32_t ft = traceFormat(path);
  if (format) *format = ft;
  Trace* tr = new Trace();
  const bool ok = ft == 0 ? readab(path, *tr) : ft == 1 ? readscf(path, *tr) : false;
  if (!ok) { delete tr; return nullptr; }
  return tr;
}
void tracyhost_trace_dims(const void* h, uint64_t* nsamples, uint64_t* ncalls) {
  const Trace* tr = static_cast<const Trace*>(h);
  size_t ns = 0;
  for (auto const& c : tr->traceACGT) ns = std::max(ns, c.size());
  *nsamples = ns;
  *ncalls = tr->basecallpos.size();
}
// signal: [4][nsamples] (channels shorter than nsamples are zero padded); text outputs have ncalls bytes
void tracyhost_trace_get(const void* h, int32_t* signal, int32_t* basecallpos, char* basecalls1, char* basecalls2, uint8_t* qual) {
  const Trace* tr = static_cast<const Trace*>(h);
  uint64_t ns, nc;
  tracyhost_trace_dims(h, &ns, &nc);
  for (size_t k = 0; k < 4; ++k)
    for (size_t i = 0; i < ns; ++i) signal[k * ns + i] = (k < tr->traceACGT.size() && i < tr->traceACGT[k].size()) ? tr->traceACGT[k][i] : 0;
  std::memcpy(basecallpos, tr->basecallpos.data(), nc * sizeof(int32_t));
  if (basecalls1) std::memcpy(basecalls1, tr->basecalls1.data(), std::min<size_t>(nc, tr->basecalls1.size()));
  if (basecalls2) std::memcpy(basecalls2, tr->basecalls2.data(), std::min<size_t>(nc, tr->basecalls2.size()));
  if (qual) std::memcpy(qual, tr->qual.data(), std::min<size_t>(nc, tr->qual.size()));
}
void tracyhost_trace_free(void* h) { delete static_cast<Trace*>(h); }

// the build's ABIF writer: signal [4][nsamples] in A,C,G,T order, written in dye order `order`
int32_t tracyhost_writeab(const char* path, const int32_t* signal, size_t nsamples, const int32_t* peaks, size_t npeaks,
                          const char* primary, size_t nprimary, const uint8_t* qual, size_t nqual, const char* secondary,
                          size_t nsecondary, const char* order) {
  Trace::TACGTMountains acgt(4);
  for (int k = 0; k < 4; ++k) acgt[k].assign(signal + k * nsamples, signal + (k + 1) * nsamples);
  return writeab(path, acgt, std::vector<int32_t>(peaks, peaks + npeaks), std::string(primary, nprimary),
                 std::vector<uint8_t>(qual, qual + nqual), secondary ? std::string(secondary, nsecondary) : std::string(),
                 order ? order : "GATC") ? 0 : -1;
}

// basecall + traceTxtOut (abif.h:513-533) into `outfile`
int32_t tracyhost_trace_txt(const char* outfile, const int32_t* trace, size_t nsamples, const int32_t* basecallpos, size_t npos,
                            float sigratio, uint32_t left_trim, uint32_t right_trim) {
  Trace tr;
  tr.traceACGT.resize(4);
  for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(trace + k * nsamples, trace + (k + 1) * nsamples);
  tr.basecallpos.assign(basecallpos, basecallpos + npos);
  BaseCalls bc;
  basecall(tr, bc, sigratio);
  if (bc.bcPos.empty()) return -1;
  traceTxtOut(std::string(outfile), bc, tr, left_trim, right_trim);
  return 0;
}

// the three alignment files of `tracy align` (sage.h:313-345) for a trace given as arrays and its final
// alignment rows: <prefix>.align.fa, <prefix>.txt, <prefix>.json
int32_t tracyhost_align_outputs(const char* prefix, const char* trace_stem, const int32_t* trace, size_t nsamples,
                                const int32_t* basecallpos, size_t npos, float sigratio, const char* row0, const char* row1,
                                size_t cols, const char* chr, const char* refslice, size_t nref, uint32_t pos, int32_t forward,
                                int32_t score, uint32_t linelimit) {
  Trace tr;
  tr.traceACGT.resize(4);
  for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(trace + k * nsamples, trace + (k + 1) * nsamples);
  tr.basecallpos.assign(basecallpos, basecallpos + npos);
  BaseCalls bc;
  basecall(tr, bc, sigratio);
  if (bc.bcPos.empty()) return -1;
  AlignRows rows;
  rows.row0.assign(row0, cols);
  rows.row1.assign(row1, cols);
  ReferenceSlice rs;
  rs.forward = forward != 0;
  rs.pos = pos;
  rs.chr = chr;
  rs.refslice.assign(refslice, nref);
  PaddedTrace padded;
  alignmentTracePadding(rows.row0, tr, bc, padded);
  const std::string pre(prefix);
  {
    std::ofstream f((pre + ".align.fa").c_str());
    alignFastaOut(f, trace_stem, rs, rows);
  }
  plotAlignment(pre + ".txt", rows, rs, score, linelimit);
  traceAlignJsonOut(pre + ".json", padded, rs, rows);
  return 0;
}

// the files `tracy decompose` writes after the device chain (indigo.h:340-442): <prefix>.decomp, .align1,
// .align2, .align3, .json and, with call_variants, <prefix>.vcf.  The trace is given as arrays (basecalled
// here, then overlaid with the decomposed calls); alignments as gapped rows.
struct tracyhost_decompose_report {
  const char* prefix;
  const char* genome_name;
  const char* input_name;
  const int32_t* trace;
  uint64_t nsamples;
  const int32_t* basecallpos;
  uint64_t npos;
  float pratio;
  uint32_t trim_left, trim_right, qual_cut, linelimit;
  const char* primary;    // decomposed calls, ncalls bytes each
  const char* secondary;
  const char* secdecomp;
  uint64_t ncalls;
  const char* rows[3][2]; // final1, final2, final3
  uint64_t cols[3];
  const char* var_rows[2][2];  // alignments variants are called on (the reverse-complement ones for reverse traces)
  uint64_t var_cols[2];
  int32_t call_variants;
  const char* chr;
  int32_t forward;
  uint32_t pos[2];        // allele1.pos, allele2.pos
  uint64_t slice_len[2];  // allele1/2 .refslice.size()
  uint64_t ref_len;       // rs.refslice.size()
  int32_t score[3];
  int32_t indelshift;
  uint32_t breakpoint;
  double a1, a2;
  const int32_t* dcp_indel;
  const int32_t* dcp_err;
  uint64_t dcp_n;
};

int32_t tracyhost_decompose_outputs(const tracyhost_decompose_report* rp) {
  Trace tr;
  tr.traceACGT.resize(4);
  for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(rp->trace + k * rp->nsamples, rp->trace + (k + 1) * rp->nsamples);
  tr.basecallpos.assign(rp->basecallpos, rp->basecallpos + rp->npos);
  BaseCalls bc;
  basecall(tr, bc, rp->pratio);
  if (bc.bcPos.size() != rp->ncalls) return -1;
  bc.primary.assign(rp->primary, rp->ncalls);
  bc.secondary.assign(rp->secondary, rp->ncalls);
  bc.secDecompose.assign(rp->secdecomp, rp->ncalls);
  AlleleReport r;
  AlignRows* al[3] = {&r.align1, &r.align2, &r.align3};
  for (int k = 0; k < 3; ++k) {
    al[k]->row0.assign(rp->rows[k][0], rp->cols[k]);
    al[k]->row1.assign(rp->rows[k][1], rp->cols[k]);
  }
  ReferenceSlice rs;
  rs.chr = rp->chr;
  rs.forward = rp->forward != 0;
  rs.filetype = 1;
  rs.refslice.assign(rp->ref_len, 'N');
  ReferenceSlice* slot[2] = {&r.rs1, &r.rs2};
  for (int k = 0; k < 2; ++k) {
    *slot[k] = rs;
    slot[k]->pos = rp->pos[k];
    slot[k]->refslice.assign(rp->slice_len[k], 'N');
  }
  r.a1Score = rp->score[0]; r.a2Score = rp->score[1]; r.a3Score = rp->score[2];
  r.bp.indelshift = rp->indelshift != 0;
  r.bp.breakpoint = rp->breakpoint;
  r.a1a2 = std::make_pair(rp->a1, rp->a2);
  for (uint64_t i = 0; i < rp->dcp_n; ++i) r.dcp.emplace_back(rp->dcp_indel[i], rp->dcp_err[i]);
  const std::string pre(rp->prefix);
  {
    std::ofstream f((pre + ".decomp").c_str());
    writeDecomposition(f, r.dcp);
  }
  ReferenceSlice secrs;
  secrs.refslice = trimmedSeq(bc.secDecompose, rp->trim_left, rp->trim_right);
  secrs.forward = true;
  secrs.chr = "Alt2";
  ReferenceSlice const* prs[3] = {&r.rs1, &r.rs2, &secrs};
  for (int k = 0; k < 3; ++k) {
    std::ofstream f((pre + ".align" + std::to_string(k + 1)).c_str());
    plotAlignment(f, *al[k], *prs[k], k + 1, rp->score[k], r.a1a2, rp->linelimit);
  }
  if (!r.bp.indelshift) r.bp.breakpoint = nearestSNP(rp->trim_left, rp->trim_right, bc, findBestTraceSection(bc));
  ReportConfig rc;
  rc.trimLeft = (uint16_t)rp->trim_left;
  rc.trimRight = (uint16_t)rp->trim_right;
  rc.qualCut = (uint16_t)rp->qual_cut;
  rc.pratio = rp->pratio;
  rc.genomeName = rp->genome_name;
  rc.inputName = rp->input_name;
  if (rp->call_variants) {
    for (int k = 0; k < 2; ++k) {
      AlignRows v;
      v.row0.assign(rp->var_rows[k][0], rp->var_cols[k]);
      v.row1.assign(rp->var_rows[k][1], rp->var_cols[k]);
      ReferenceSlice vrs = *slot[k];
      if (!rs.forward) reverseReferenceSlice(*slot[k], vrs);
      callVariants(v, vrs, r.var);
    }
    std::stable_sort(r.var.begin(), r.var.end());  // (ties by (pos, basenum) keep push order, as tracyhip_decompose_variants orders them)
    std::ofstream f((pre + ".vcf").c_str());
    vcfTextOutput(f, rc, bc, r.var, rs);
    if (!bcfOutput(pre + ".bcf", rc, bc, r.var, rs)) return -2;
  }
  std::ofstream f((pre + ".json").c_str());
  traceAlleleAlignJsonOut(f, rc, bc, tr, r);
  return 0;
}

// ---- k-mer seeding in an indexed genome (seed.hpp; fmindex.h:173-326) --------------------------------
// path: a (gzip-compressed) multi-FASTA -- the table is built in memory -- or an index file written by tracyhost_genome_save
// (`tracy_amd_cli index`), which is mapped read-only (kmer must be the index's)
void* tracyhost_genome_open(const char* path, uint32_t kmer, uint32_t nthreads) {
  GenomeIndex* g = new GenomeIndex();
  if (GenomeIndex::is_index_file(path)) {
    if (!g->open_index(path) || g->k != kmer) { delete g; return nullptr; }
    return g;
  }
  if (!g->load(path)) { delete g; return nullptr; }
  g->build(kmer, nthreads);
  return g;
}
int tracyhost_genome_save(const void* h, const char* path) { return static_cast<const GenomeIndex*>(h)->save(path) ? 0 : -1; }
void tracyhost_genome_free(void* h) { delete static_cast<GenomeIndex*>(h); }
uint32_t tracyhost_genome_contigs(const void* h) { return (uint32_t)static_cast<const GenomeIndex*>(h)->names.size(); }
uint64_t tracyhost_genome_count(const void* h, const char* pat, size_t n) { return static_cast<const GenomeIndex*>(h)->count(std::string(pat, n)); }
// the index's arrays (GenomeIndex::view) for a device upload: the layout of tracyhip_genome_desc (include/tracy_hip.h), pointers into the
// index (valid while it is open); an in-memory build and a mapped index file alike.  Returns -1 when the index has no table.
struct tracyhost_genome_view_t {
  uint32_t k, bucket_bits;
  const uint64_t* bkt;
  const uint64_t* tab;
  uint64_t ntab;
  const char* text;
  uint64_t text_len;
  const uint64_t* starts;
  const uint32_t* lengths;
  uint32_t ncontigs;
};
int tracyhost_genome_view(const void* h, tracyhost_genome_view_t* out) {
  const GenomeIndex* g = static_cast<const GenomeIndex*>(h);
  if (!g || !out || !g->has_table()) return -1;
  const GenomeIndex::View v = g->view();
  *out = tracyhost_genome_view_t{v.k, v.bucket_bits, v.bkt, v.tab, v.ntab, v.text, v.text_len, v.starts, v.lengths, v.ncontigs};
  return 0;
}
// A (gzip-compressed) multi-FASTA loaded WITHOUT a table: the text and contig table a device build starts from (tracyhost_genome_text,
// tracyhip_genome_build); tracyhost_genome_adopt then gives it the table.  An index file is refused (NULL).
void* tracyhost_genome_load(const char* path) {
  if (GenomeIndex::is_index_file(path) || GenomeIndex::is_stale_index_file(path)) return nullptr;
  GenomeIndex* g = new GenomeIndex();
  if (!g->load(path)) { delete g; return nullptr; }
  return g;
}
// the text and contig table of a loaded genome (the view's table fields NULL / 0 when it has no table), for tracyhip_genome_build
int tracyhost_genome_text(const void* h, tracyhost_genome_view_t* out) {
  const GenomeIndex* g = static_cast<const GenomeIndex*>(h);
  if (!g || !out || !g->text.p) return -1;
  const GenomeIndex::View v = g->view();
  const bool t = g->has_table();
  *out = tracyhost_genome_view_t{v.k, t ? v.bucket_bits : 0, t ? v.bkt : nullptr, t ? v.tab : nullptr, t ? v.ntab : 0, v.text, v.text_len,
                                 v.starts, v.lengths, v.ncontigs};
  return 0;
}
// GenomeIndex::adopt: a table built elsewhere (dir [2^bucket_bits + 1], tab [2 * ntab], the layout tracyhip_genome_download writes) copied
// into a genome loaded by tracyhost_genome_load.  -1: not a loaded FASTA, or k / bucket_bits / a directory that is not a table's.
int tracyhost_genome_adopt(void* h, uint32_t kmer, uint32_t bucket_bits, const uint64_t* dir, const uint64_t* tab, uint64_t ntab) {
  return h && static_cast<GenomeIndex*>(h)->adopt(kmer, bucket_bits, dir, tab, (std::size_t)ntab) ? 0 : -1;
}
// the bucket_bits an in-memory build picks for k (min(2k, 24), or the TRACY_AMD_SEED_BUCKET_BITS knob)
uint32_t tracyhost_default_bucket_bits(uint32_t kmer) { return GenomeIndex::default_bucket_bits(kmer); }
// name of contig i (NUL-terminated, valid while the index is open)
const char* tracyhost_genome_contig_name(const void* h, uint32_t i) {
  const GenomeIndex* g = static_cast<const GenomeIndex*>(h);
  return i < g->names.size() ? g->names[i].c_str() : nullptr;
}

// getReferenceSlice for a batch of consensus strings (trace t: consensus + cons_off[t], cons_len[t] bytes), one
// thread per stripe of traces.  Per trace: status 1 = anchored, 0 = not; forward, kmersupport, pos (window start
// in the contig), contig index, and the ORIENTED window at slices + t * slice_cap (slice_len[t] bytes).
void tracyhost_seed_batch(const void* h, uint32_t ntraces, const char* consensus, const uint64_t* cons_off, const uint32_t* cons_len,
                          uint32_t trim_left, uint32_t trim_right, uint32_t kmer, uint32_t min_support, uint32_t maxindel,
                          uint32_t nthreads, int32_t* status, uint8_t* forward, uint32_t* kmersupport, uint32_t* pos, uint32_t* contig,
                          char* slices, uint64_t slice_cap, uint32_t* slice_len) {
  const GenomeIndex* g = static_cast<const GenomeIndex*>(h);
  // seeding is a stream of dependent table look-ups (memory latency, not arithmetic): every hardware thread helps,
  // also under a CPU quota (measured on the 256-thread / 16-CPU GPU box: 256 threads 171 k traces/s, 16 threads 99 k)
  if (nthreads == 0) nthreads = std::max(1u, std::thread::hardware_concurrency());
  SeedConfig sc;
  sc.trimLeft = (uint16_t)trim_left; sc.trimRight = (uint16_t)trim_right; sc.kmer = (uint16_t)kmer;
  sc.minKmerSupport = (uint16_t)min_support; sc.maxindel = (uint16_t)maxindel;
  auto work = [&](uint32_t tid) {
    for (uint32_t t = tid; t < ntraces; t += nthreads) {
      ReferenceSlice rs;
      rs.filetype = 0;
      const bool ok = getReferenceSlice(sc, *g, std::string(consensus + cons_off[t], cons_len[t]), rs);
      status[t] = ok ? 1 : 0;
      slice_len[t] = 0;
      if (!ok) continue;
      forward[t] = rs.forward ? 1 : 0;
      kmersupport[t] = rs.kmersupport;
      pos[t] = rs.pos;
      uint32_t ci = 0;
      while (ci < g->names.size() && g->names[ci] != rs.chr) ++ci;
      contig[t] = ci;
      const size_t n = std::min<size_t>(rs.refslice.size(), slice_cap);
      std::memcpy(slices + (size_t)t * slice_cap, rs.refslice.data(), n);
      slice_len[t] = (uint32_t)n;
    }
  };
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nthreads; ++t) th.emplace_back(work, t);
  for (auto& t : th) t.join();
}

// trimTrace (trim.h:35-73) of the basecalled trace
int32_t tracyhost_trim_trace(const int32_t* trace, size_t nsamples, const int32_t* basecallpos, size_t npos, float sigratio,
                             float stringency, uint32_t* left, uint32_t* right) {
  Trace tr;
  tr.traceACGT.resize(4);
  for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(trace + k * nsamples, trace + (k + 1) * nsamples);
  tr.basecallpos.assign(basecallpos, basecallpos + npos);
  BaseCalls bc;
  basecall(tr, bc, sigratio);
  trimTrace(stringency, bc, *left, *right);
  return 0;
}

// loadSingleFasta (fasta.h:54-95): returns the sequence length, -1 on error; name/seq need capacity
int64_t tracyhost_load_fasta(const char* path, char* name, size_t name_cap, char* seq, size_t seq_cap) {
  std::string n, s;
  if (!loadSingleFasta(path, n, s)) return -1;
  if (n.size() + 1 > name_cap || s.size() > seq_cap) return -2;
  std::memcpy(name, n.c_str(), n.size() + 1);
  std::memcpy(seq, s.data(), s.size());
  return (int64_t)s.size();
}

// Seeded synthetic `tracy align` workload: ntraces cases, case i seeded with seed0 + i.  refs: ntraces x n
// bytes; profiles: ntraces x 6 x mf floats (createProfile of the basecalled synthetic chromatogram; when
// the basecaller drops a window the profile is padded with uniform 0.25 columns to keep mf columns).
// reverse[i] = 1 when the trace was copied from the reverse strand.  Multi-threaded over cases.
void tracyhost_synth_align(uint64_t seed0, uint32_t ntraces, uint32_t n, uint32_t mf, uint8_t* refs, float* profiles,
                           uint8_t* reverse, uint32_t nthreads) {
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  auto work = [&](uint32_t tid) {
    for (uint32_t i = tid; i < ntraces; i += nthreads) {
      SplitMix64 rng(seed0 + i);
      std::string ref, seq;
      bool rev;
      synth_sequence(rng, n, mf, ref, seq, rev);
      Trace tr;
      render_trace(rng, seq, nullptr, 1.0, tr);
      BaseCalls bc;
      basecall(tr, bc, 0.33f);
      Profile p;
      createProfile(tr, bc, p, 0, 0);
      std::memcpy(refs + (size_t)i * n, ref.data(), n);
      float* dst = profiles + (size_t)i * 6 * mf;
      for (int k = 0; k < 6; ++k)
        for (uint32_t j = 0; j < mf; ++j) dst[(size_t)k * mf + j] = (j < p.cols) ? p(k, j) : (k < 4 ? 0.25f : 0.0f);
      if (reverse) reverse[i] = rev ? 1 : 0;
    }
  };
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nthreads; ++t) th.emplace_back(work, t);
  for (auto& t : th) t.join();
}


// Seeded synthetic `tracy decompose` case: reference window of n bases; allele 1 =
// mf bases copied from it (forward strand), allele 2 = allele 1 with one heterozygous indel (length
// U[1,maxlen], insertion or deletion) at a position U[150, mf-300] plus 0.5 % heterozygous SNVs; the two
// alleles are mixed frac1 : 1-frac1 in the chromatogram.  kind & 3: 0 = het indel, 1 = het SNVs only (no indel), 2 = homozygous
// indel only (both alleles carry it, no het SNVs), 3 = no variant at all.  kind & 32: a low-complexity window.  kind & 16: the window handed out is the reverse
// complement of the one the trace was copied from (the trace reads the reverse strand of its reference).
// Outputs: ref[n]; signal[4][12*(mf+40)+12] (zero padded), basecallpos[npos]; returns npos.
uint32_t tracyhost_synth_decompose(uint64_t seed, uint32_t n, uint32_t mf, uint32_t maxlen, int kind, double frac1,
                                   uint8_t* ref_out, int32_t* signal, uint32_t nsamples_cap, int32_t* basecallpos,
                                   int32_t* indel_out) {
  SplitMix64 rng(seed);
  std::string ref(n, 'A');
  if (kind & 32) {  // low complexity: short units repeated a few times -- alignments with many co-optimal paths (gaps that can sit anywhere in a run)
    for (uint32_t i = 0; i < n;) {
      char unit[6];
      const uint32_t ul = 1 + rng.below(6), reps = 1 + rng.below(ul == 1 ? 8 : 5);
      for (uint32_t u = 0; u < ul; ++u) unit[u] = kBases[rng.below(4)];
      for (uint32_t r = 0; r < reps && i < n; ++r)
        for (uint32_t u = 0; u < ul && i < n; ++u) ref[i++] = unit[u];
    }
  } else {
    for (uint32_t i = 0; i < n; ++i) ref[i] = kBases[rng.below(4)];
  }
  const uint32_t start = (n > mf + 200) ? 100 + rng.below(n - mf - 200) : 0;
  std::string a1 = ref.substr(start, mf + 40);
  std::string a2 = a1;
  int32_t indel = 0;
  const bool reverse_strand = (kind & 16) != 0;
  kind &= 3;
  if (kind == 0 || kind == 2) {
    const uint32_t pos = 150 + rng.below(mf > 450 ? mf - 450 : 1);
    const uint32_t len = 1 + rng.below(maxlen);
    if (rng.next() & 1) {  // deletion in allele 2
      a2.erase(pos, len);
      indel = -(int32_t)len;
    } else {
      std::string ins(len, 'A');
      for (auto& c : ins) c = kBases[rng.below(4)];
      a2.insert(pos, ins);
      indel = (int32_t)len;
    }
    if (kind == 2) a1 = a2;  // homozygous: both alleles carry the indel
  }
  if (kind < 2)
    for (size_t i = 0; i < a2.size(); ++i)
      if (rng.unit() < 0.005) a2[i] = kBases[(base_index(a2[i]) + 1 + rng.below(3)) & 3];
  if (reverse_strand) {
    std::reverse(ref.begin(), ref.end());
    for (auto& c : ref) c = complement(c);
  }
  a1.resize(mf);
  a2.resize(mf);
  Trace tr;
  render_trace(rng, a1, &a2, frac1, tr);
  const size_t ns = tr.traceACGT[0].size();
  for (int k = 0; k < 4; ++k)
    for (uint32_t i = 0; i < nsamples_cap; ++i) signal[(size_t)k * nsamples_cap + i] = i < ns ? tr.traceACGT[k][i] : 0;
  for (size_t i = 0; i < tr.basecallpos.size(); ++i) basecallpos[i] = tr.basecallpos[i];
  std::memcpy(ref_out, ref.data(), n);
  if (indel_out) *indel_out = indel;
  return (uint32_t)tr.basecallpos.size();
}


// Batch of synthetic `tracy decompose` inputs (config 3), multi-threaded: trace i is seeded with seed0 + i,
// 80 % heterozygous indels (kind 0), 20 % SNV-only (kind 1), allele mix 60/40.  Every trace is basecalled
// (0.33) and profiled here; traces whose basecaller dropped a window are regenerated with the next seed
// stride so that all traces have exactly mf basecalls.  Layouts: refs [nt][n]; signal [nt][4][ns] with
// ns = 12*mf+12; bcpos / primary / secondary [nt][mf]; profiles [nt][6][mf].
// mix 0: the round-1 batch above (all forward strand).  mix 1: BASELINE configs[2] as SURVEY.md 8d words it -- trace i with
// i % 10 == 8 carries a homozygous indel only, i % 10 == 9 no variant, the rest one het indel + 0.5 % het SNVs; odd traces
// read the reverse strand of their window.  mix 2: mix 1 in low-complexity windows (short tandem repeats: co-optimal alignments everywhere).
static void synth_decompose_batch_mix(uint64_t seed0, uint32_t nt, uint32_t n, uint32_t mf, uint8_t* refs, int32_t* signal,
                                      int32_t* bcpos, uint8_t* primary, uint8_t* secondary, float* profiles, uint32_t nthreads, int mix);
void tracyhost_synth_decompose_batch(uint64_t seed0, uint32_t nt, uint32_t n, uint32_t mf, uint8_t* refs, int32_t* signal,
                                     int32_t* bcpos, uint8_t* primary, uint8_t* secondary, float* profiles, uint32_t nthreads) {
  synth_decompose_batch_mix(seed0, nt, n, mf, refs, signal, bcpos, primary, secondary, profiles, nthreads, 0);
}
void tracyhost_synth_decompose_batch2(uint64_t seed0, uint32_t nt, uint32_t n, uint32_t mf, uint8_t* refs, int32_t* signal,
                                      int32_t* bcpos, uint8_t* primary, uint8_t* secondary, float* profiles, uint32_t nthreads, int mix) {
  synth_decompose_batch_mix(seed0, nt, n, mf, refs, signal, bcpos, primary, secondary, profiles, nthreads, mix);
}
static void synth_decompose_batch_mix(uint64_t seed0, uint32_t nt, uint32_t n, uint32_t mf, uint8_t* refs, int32_t* signal,
                                      int32_t* bcpos, uint8_t* primary, uint8_t* secondary, float* profiles, uint32_t nthreads, int mix) {
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  const uint32_t ns = 12 * mf + 12;
  auto work = [&](uint32_t tid) {
    std::vector<int32_t> pos(mf + 64);
    for (uint32_t i = tid; i < nt; i += nthreads) {
      for (uint64_t attempt = 0;; ++attempt) {
        const uint64_t seed = seed0 + i + attempt * 1000003ull * nt;
        int32_t indel = 0;
        int32_t* sig = signal + (size_t)i * 4 * ns;
        int kind = (i % 5 == 4) ? 1 : 0;
        if (mix >= 1) kind = ((i % 10 == 8) ? 2 : (i % 10 == 9) ? 3 : 0) | ((i & 1) ? 16 : 0);
        if (mix == 2) kind |= 32;  // ... in low-complexity windows
        const uint32_t npos = tracyhost_synth_decompose(seed, n, mf, 30, kind, 0.6, refs + (size_t)i * n, sig, ns,
                                                        pos.data(), &indel);
        Trace tr;
        tr.traceACGT.resize(4);
        for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(sig + (size_t)k * ns, sig + (size_t)(k + 1) * ns);
        tr.basecallpos.assign(pos.begin(), pos.begin() + npos);
        BaseCalls bc;
        basecall(tr, bc, 0.33f);
        if (bc.primary.size() != mf) continue;
        Profile p;
        createProfile(tr, bc, p, 0, 0);
        std::memcpy(bcpos + (size_t)i * mf, bc.bcPos.data(), sizeof(int32_t) * mf);
        std::memcpy(primary + (size_t)i * mf, bc.primary.data(), mf);
        std::memcpy(secondary + (size_t)i * mf, bc.secondary.data(), mf);
        std::memcpy(profiles + (size_t)i * 6 * mf, p.data(), sizeof(float) * 6 * mf);
        break;
      }
    }
  };
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nthreads; ++t) th.emplace_back(work, t);
  for (auto& t : th) t.join();
}

// The host chain in front of every command -- basecall (+ estimateQualities), trimTrace when stringency >= 1, createProfile -- for a batch
// of equally shaped traces on `nthreads` threads: signal [nt][4][ns], basecallpos [nt][np]; results [nt][np] (profiles [nt][6][np], the
// first 6 * bc_len[i] floats of a trace's region used), trims [nt][2].  Any result pointer may be null.  Returns the seconds the slowest
// thread spent in the chain itself: every thread first copies its traces into Trace objects (what a file reader leaves), untimed.
double tracyhost_basecall_batch(const int32_t* signal, uint32_t nt, uint32_t ns, const int32_t* basecallpos, uint32_t np, float sigratio,
                                float stringency, uint32_t nthreads, uint8_t* primary, uint8_t* secondary, int32_t* bcpos, uint8_t* estqual,
                                float* profiles, uint32_t* bc_len, uint32_t* trims) {
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  std::vector<double> spent(nthreads, 0.0);
  auto work = [&](uint32_t tid) {
    const uint32_t lo = (uint32_t)((uint64_t)nt * tid / nthreads), hi = (uint32_t)((uint64_t)nt * (tid + 1) / nthreads);
    std::vector<Trace> trs(hi - lo);
    for (uint32_t i = lo; i < hi; ++i) {
      Trace& tr = trs[i - lo];
      tr.traceACGT.resize(4);
      const int32_t* sig = signal + (size_t)i * 4 * ns;
      for (int k = 0; k < 4; ++k) tr.traceACGT[k].assign(sig + (size_t)k * ns, sig + (size_t)(k + 1) * ns);
      tr.basecallpos.assign(basecallpos + (size_t)i * np, basecallpos + (size_t)(i + 1) * np);
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = lo; i < hi; ++i) {
      Trace const& tr = trs[i - lo];
      BaseCalls bc;
      basecall(tr, bc, sigratio);
      uint32_t l = 0, r = 0;
      if (stringency >= 1) trimTrace(stringency, bc, l, r);
      Profile p;
      createProfile(tr, bc, p, 0, 0);
      const size_t n = bc.primary.size();
      if (primary) std::memcpy(primary + (size_t)i * np, bc.primary.data(), n);
      if (secondary) std::memcpy(secondary + (size_t)i * np, bc.secondary.data(), n);
      if (bcpos) std::memcpy(bcpos + (size_t)i * np, bc.bcPos.data(), n * sizeof(int32_t));
      if (estqual) std::memcpy(estqual + (size_t)i * np, bc.estQual.data(), n);
      if (profiles) std::memcpy(profiles + (size_t)i * 6 * np, p.data(), sizeof(float) * 6 * n);
      if (bc_len) bc_len[i] = (uint32_t)n;
      if (trims) { trims[2 * i] = (uint16_t)l; trims[2 * i + 1] = (uint16_t)r; }
    }
    spent[tid] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  std::vector<std::thread> th;
  for (uint32_t t = 0; t < nthreads; ++t) th.emplace_back(work, t);
  for (auto& t : th) t.join();
  double worst = 0;
  for (double v : spent) worst = std::max(worst, v);
  return worst;
}

// ---- the host side of the variant section of `tracy decompose -v` as tracy_amd_cli's call_variants runs it (the path behind
// tracyhip_decompose_variants' truncated traces; tools/variants_device_line.py times it beside the device call) ----
// reverseComplement of n strings: string i is src[off[i] .. + len[i]) and goes to dst + dst_off[i]
int tracyhost_revcomp_batch(const uint8_t* src, const uint64_t* off, const uint32_t* len, uint32_t n, uint8_t* dst, const uint64_t* dst_off, uint32_t nthreads) {
  if (n && (!src || !off || !len || !dst || !dst_off)) return -1;
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  std::vector<std::thread> th;
  for (uint32_t w = 0; w < nthreads; ++w)
    th.emplace_back([=]() {
      std::string s;
      for (uint32_t i = (uint32_t)((uint64_t)n * w / nthreads); i < (uint32_t)((uint64_t)n * (w + 1) / nthreads); ++i) {
        s.assign(reinterpret_cast<const char*>(src) + off[i], len[i]);
        reverseComplement(s);
        std::memcpy(dst + dst_off[i], s.data(), s.size());
      }
    });
  for (auto& t : th) t.join();
  return 0;
}
// callVariants of both allele alignments of every trace (alignments 2t and 2t + 1: rows0 / rows1 + off[i], len[i] columns, rs.pos pos[i]),
// std::stable_sort, variantCallIndex.  Results in the layout of tracyhip_call_variants: 8 words per record (pos, basenum, gt, call_index,
// ref_off, ref_len, alt_off, alt_len), max_variants records and max_text bytes per trace; a trace that does not fit: var_n 0, flag 1.
int tracyhost_call_variants_batch(uint32_t n, const uint8_t* rows0, const uint8_t* rows1, const uint64_t* off, const uint32_t* len, const int32_t* pos,
                                  const uint8_t* forward, const uint32_t* bc_len, uint32_t trim_left, uint32_t trim_right, uint32_t max_variants,
                                  uint32_t max_text, uint32_t* rec, uint8_t* text, uint32_t* var_n, uint32_t* var_flags, uint32_t nthreads) {
  if (n && (!rows0 || !rows1 || !off || !len || !pos || !forward || !bc_len || !rec || !text || !var_n || !var_flags)) return -1;
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  std::vector<std::thread> th;
  for (uint32_t w = 0; w < nthreads; ++w)
    th.emplace_back([=]() {
      std::vector<Variant> var;
      AlignRows al;
      ReferenceSlice rs;
      rs.chr = "chr";
      for (uint32_t t = (uint32_t)((uint64_t)n * w / nthreads); t < (uint32_t)((uint64_t)n * (w + 1) / nthreads); ++t) {
        var.clear();
        for (uint32_t k = 0; k < 2; ++k) {
          const std::size_t i = 2 * (std::size_t)t + k;
          al.row0.assign(reinterpret_cast<const char*>(rows0) + off[i], len[i]);
          al.row1.assign(reinterpret_cast<const char*>(rows1) + off[i], len[i]);
          rs.pos = pos[i];
          callVariants(al, rs, var);
        }
        std::stable_sort(var.begin(), var.end());
        std::size_t bytes = 0;
        for (Variant const& v : var) bytes += v.ref.size() + v.alt.size();
        var_n[t] = 0;
        var_flags[t] = (var.size() > max_variants || bytes > max_text) ? 1u : 0u;
        if (var_flags[t]) continue;
        uint32_t at = 0;
        uint32_t* r = rec + 8 * (std::size_t)t * max_variants;
        uint8_t* tx = text + (std::size_t)t * max_text;
        for (Variant const& v : var) {
          const uint32_t call = forward[t] ? trim_left + (uint32_t)v.basenum - 1u : bc_len[t] - (trim_right + (uint32_t)v.basenum);
          const uint32_t rl = (uint32_t)v.ref.size(), alen = (uint32_t)v.alt.size();
          const uint32_t w8[8] = {(uint32_t)v.pos, (uint32_t)v.basenum, (uint32_t)v.gt, call, at, rl, at + rl, alen};
          std::memcpy(r, w8, sizeof(w8));
          std::memcpy(tx + at, v.ref.data(), rl);
          std::memcpy(tx + at + rl, v.alt.data(), alen);
          at += rl + alen;
          r += 8;
        }
        var_n[t] = (uint32_t)var.size();
      }
    });
  for (auto& t : th) t.join();
  return 0;
}

// ---- the gapped chromatograms of a batch as the command line produces them, one trace after the other per thread: trimTrace(tr, bc, l,
// r, nbc), reverseComplementTrace, alignmentTracePadding (assemble_out.hpp, sage_out.hpp) over the flattened arrays of
// tracyhip_pad_traces (the fallback for its deferred traces; tools/pad_device_line.py times it beside the device call) ----
// status: 0 answered; 1 refused -- the reference's loops stall or read outside their arrays (no call, a position outside [0, nsamples)
// or not above its neighbour, trims that leave no call, more letters in the row than calls kept); 2 a capacity is too small (sizes
// reported).  Payload results may be null (all null: sizes only); trim_l / trim_r / reverse may be null.
int tracyhost_pad_batch(uint32_t n, const void* signal, const uint64_t* signal_offset, const uint32_t* nsamples, uint32_t sample_bytes,
                        const int32_t* bcpos, const uint8_t* primary, const uint8_t* secondary, const uint8_t* consensus, const uint8_t* estqual,
                        const uint64_t* bc_offset, const uint32_t* bc_len, const uint8_t* rows, const uint64_t* row_offset, const uint32_t* row_len,
                        const uint32_t* trim_l, const uint32_t* trim_r, const uint8_t* reverse, int32_t* status, uint32_t* nsamples_out,
                        uint32_t* ncalls_out, uint32_t* leading, uint32_t* trailing, uint32_t* step, void* o_signal, const uint64_t* sample_offset,
                        const uint32_t* sample_cap, int32_t* o_bcpos, uint8_t* o_primary, uint8_t* o_secondary, uint8_t* o_consensus, uint8_t* o_estqual,
                        const uint64_t* call_offset, const uint32_t* call_cap, uint32_t nthreads) {
  const bool want_calls = o_bcpos || o_primary || o_secondary || o_consensus || o_estqual;
  if (n && (!signal || !signal_offset || !nsamples || !bcpos || !primary || !secondary || !consensus || !estqual || !bc_offset || !bc_len || !rows ||
            !row_offset || !row_len || !status || !nsamples_out || !ncalls_out || !leading || !trailing || !step))
    return -1;
  if ((sample_bytes != 2 && sample_bytes != 4) || (o_signal && (!sample_offset || !sample_cap)) || (want_calls && (!call_offset || !call_cap))) return -1;
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  std::vector<std::thread> th;
  for (uint32_t w = 0; w < nthreads; ++w)
    th.emplace_back([=]() {
      for (uint32_t t = (uint32_t)((uint64_t)n * w / nthreads); t < (uint32_t)((uint64_t)n * (w + 1) / nthreads); ++t) {
        const uint32_t ns = nsamples[t], nc = bc_len[t], l = trim_l ? trim_l[t] : 0, r = trim_r ? trim_r[t] : 0;
        const int32_t* pos = bcpos + bc_offset[t];
        status[t] = 1;
        nsamples_out[t] = ncalls_out[t] = 0;
        bool ok = nc >= 1 && ns >= 1 && (uint64_t)l + r < nc;
        for (uint32_t i = 0; ok && i < nc; ++i) ok = pos[i] >= 0 && (uint32_t)pos[i] < ns && (i == 0 || pos[i] > pos[i - 1]);
        const std::string row(reinterpret_cast<const char*>(rows) + row_offset[t], row_len[t]);
        if (ok) ok = (uint64_t)(row.size() - (std::size_t)std::count(row.begin(), row.end(), '-')) <= (uint64_t)(nc - l - r);
        if (!ok) continue;
        Trace tr;
        BaseCalls bc;
        tr.traceACGT.resize(4);
        for (int k = 0; k < 4; ++k) {
          tr.traceACGT[k].resize(ns);
          const uint64_t at = signal_offset[t] + (uint64_t)k * ns;
          if (sample_bytes == 4) std::memcpy(tr.traceACGT[k].data(), static_cast<const int32_t*>(signal) + at, 4ull * ns);
          else
            for (uint32_t x = 0; x < ns; ++x) tr.traceACGT[k][x] = static_cast<const int16_t*>(signal)[at + x];
        }
        bc.bcPos.assign(pos, pos + nc);
        bc.primary.assign(reinterpret_cast<const char*>(primary) + bc_offset[t], nc);
        bc.secondary.assign(reinterpret_cast<const char*>(secondary) + bc_offset[t], nc);
        bc.consensus.assign(reinterpret_cast<const char*>(consensus) + bc_offset[t], nc);
        bc.estQual.assign(estqual + bc_offset[t], estqual + bc_offset[t] + nc);
        BaseCalls nbc;
        trimTrace(tr, bc, l, r, nbc);
        PaddedTrace padded;
        Trace ttr;
        BaseCalls tbc;
        const bool rev = reverse && reverse[t];
        if (rev) reverseComplementTrace(tr, nbc, ttr, tbc);
        BaseCalls const& used = rev ? tbc : nbc;
        alignmentTracePadding(row, rev ? ttr : tr, used, padded);
        const uint32_t nso = (uint32_t)padded.tr.traceACGT[0].size(), nco = (uint32_t)padded.bc.bcPos.size();
        nsamples_out[t] = nso; ncalls_out[t] = nco;
        leading[t] = padded.leadingGaps; trailing[t] = padded.trailingGaps;
        step[t] = 6;  // as alignmentTracePadding computes it (json.h:386-392)
        if (used.bcPos.size() > 1) {
          double avg = 0;
          for (uint32_t i = 1; i < used.bcPos.size(); ++i) avg += (used.bcPos[i] - used.bcPos[i - 1]);
          avg /= (used.bcPos.size() - 1);
          step[t] = (uint32_t)avg;
        }
        if ((o_signal && nso > sample_cap[t]) || (want_calls && nco > call_cap[t])) { status[t] = 2; continue; }
        status[t] = 0;
        if (o_signal)
          for (int k = 0; k < 4; ++k) {
            const uint64_t at = sample_offset[t] + (uint64_t)k * nso;
            if (sample_bytes == 4) std::memcpy(static_cast<int32_t*>(o_signal) + at, padded.tr.traceACGT[k].data(), 4ull * nso);
            else
              for (uint32_t x = 0; x < nso; ++x) static_cast<int16_t*>(o_signal)[at + x] = (int16_t)padded.tr.traceACGT[k][x];
          }
        if (!want_calls) continue;
        const uint64_t co = call_offset[t];
        if (o_bcpos) std::memcpy(o_bcpos + co, padded.bc.bcPos.data(), 4ull * nco);
        if (o_primary) std::memcpy(o_primary + co, padded.bc.primary.data(), nco);
        if (o_secondary) std::memcpy(o_secondary + co, padded.bc.secondary.data(), nco);
        if (o_consensus) std::memcpy(o_consensus + co, padded.bc.consensus.data(), nco);
        if (o_estqual) std::memcpy(o_estqual + co, padded.bc.estQual.data(), nco);
      }
    });
  for (auto& t : th) t.join();
  return 0;
}

// ---- the per-trace text of a batch as the command line prints it, one trace after the other per thread: traceTxtOut (trace_io.hpp),
// traceJsonBody (indigo_out.hpp) and assemblyTrace (sage_out.hpp) into a TextBuf over the flattened arrays of tracyhip_render_traces (the
// fallback for its deferred traces; tools/render_device_line.py times it beside the device call) ----
// form: 0 the .abif table, 1 the trace body of the decompose / basecall JSON, 2 the gapped trace from "peakA" through the "basecalls" line.
// status: 0 answered; 1 refused -- the reference's cursor loop stalls or reads outside its arrays (no call, no sample, a position outside
// [0, nsamples) or not above its neighbour) or the trace is beyond what the device answers (more than 131071 calls, more than 2^23
// samples); 2 text_cap is too small (text_len reported).  text may be null (sizes only); consensus is read by form 0 alone; trim_l / trim_r
// may be null.
int tracyhost_render_batch(uint32_t n, uint32_t form, const void* signal, const uint64_t* signal_offset, const uint32_t* nsamples, uint32_t sample_bytes,
                           const int32_t* bcpos, const uint8_t* primary, const uint8_t* secondary, const uint8_t* consensus, const uint8_t* estqual,
                           const uint64_t* bc_offset, const uint32_t* bc_len, const uint32_t* trim_l, const uint32_t* trim_r, int32_t* status,
                           uint32_t* text_len, uint8_t* text, const uint64_t* text_offset, const uint64_t* text_cap, uint32_t nthreads) {
  if (n && (!signal || !signal_offset || !nsamples || !bcpos || !primary || !secondary || !estqual || !bc_offset || !bc_len || !status || !text_len))
    return -1;
  if (form > 2 || (n && form == 0 && !consensus) || (sample_bytes != 2 && sample_bytes != 4) || (text && (!text_offset || !text_cap))) return -1;
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  std::vector<std::thread> th;
  for (uint32_t w = 0; w < nthreads; ++w)
    th.emplace_back([=]() {
      PaddedTrace p;  // (form 2 prints a padded trace; the other two its two members)
      Trace& tr = p.tr;
      BaseCalls& bc = p.bc;
      tr.traceACGT.resize(4);
      for (uint32_t t = (uint32_t)((uint64_t)n * w / nthreads); t < (uint32_t)((uint64_t)n * (w + 1) / nthreads); ++t) {
        const uint32_t ns = nsamples[t], nc = bc_len[t];
        const int32_t* pos = bcpos + bc_offset[t];
        status[t] = 1;
        text_len[t] = 0;
        bool ok = nc >= 1 && nc <= 131071u && ns >= 1 && ns <= (1u << 23);
        for (uint32_t i = 0; ok && i < nc; ++i) ok = pos[i] >= 0 && (uint32_t)pos[i] < ns && (i == 0 || pos[i] > pos[i - 1]);
        if (!ok) continue;
        for (int k = 0; k < 4; ++k) {
          tr.traceACGT[k].resize(ns);
          const uint64_t at = signal_offset[t] + (uint64_t)k * ns;
          if (sample_bytes == 4) std::memcpy(tr.traceACGT[k].data(), static_cast<const int32_t*>(signal) + at, 4ull * ns);
          else
            for (uint32_t x = 0; x < ns; ++x) tr.traceACGT[k][x] = static_cast<const int16_t*>(signal)[at + x];
        }
        bc.bcPos.assign(pos, pos + nc);
        bc.primary.assign(reinterpret_cast<const char*>(primary) + bc_offset[t], nc);
        bc.secondary.assign(reinterpret_cast<const char*>(secondary) + bc_offset[t], nc);
        if (form == 0) bc.consensus.assign(reinterpret_cast<const char*>(consensus) + bc_offset[t], nc);
        bc.estQual.assign(estqual + bc_offset[t], estqual + bc_offset[t] + nc);
        TextBuf out((std::size_t)48 * ns + 4096);
        std::size_t from = 0, to = 0;
        if (form == 0) {
          traceTxtOut(out, bc, tr, trim_l ? trim_l[t] : 0u, trim_r ? trim_r[t] : 0u);
          to = out.size();
        } else if (form == 1) {
          traceJsonBody(out, bc, tr);
          to = out.size();
        } else {
          p.leadingGaps = p.trailingGaps = 0;
          assemblyTrace(out, p, "");
          static const char head[] = "{\n\"traceFileName\": \"\",\n\"leadingGaps\": 0,\n\"trailingGaps\": 0,\n";
          from = sizeof(head) - 1;  // the lines in front of "peakA" ...
          to = out.size() - 2;      // ... and the closing "}\n" stay with the caller
        }
        if (to - from > 0x7fffffffull) continue;
        text_len[t] = (uint32_t)(to - from);
        if (text && to - from > text_cap[t]) { status[t] = 2; continue; }
        status[t] = 0;
        if (text) std::memcpy(text + text_offset[t], out.data() + from, to - from);
      }
    });
  for (auto& t : th) t.join();
  return 0;
}

// ---- the text printed from the two gapped rows of an alignment, one alignment after the other per thread: plotAlignmentLines,
// alignFastaOut and the tail of traceAlignJsonOut (sage_out.hpp) into a TextBuf over the flattened arrays of tracyhip_render_alignments
// (the fallback for its deferred alignments; tools/alntext_device_line.py times it beside the device call) ----
// form: 0 the plot (name0 / name1 are its two header lines), 1 the FASTA (name0 the trace stem, name1 rs.chr), 2 the JSON from
// ",\n\"refchr\"" through "}\n" (name1 rs.chr; name0 is not read).  Every alignment is printed, also those the device defers: ref_pos is
// rs.pos (taken as the uint32 it is there), ref_len rs.refslice.size().  status: 0 answered; 1 the text does not fit 32 bits; 2 text_cap
// is too small (text_len reported).  text may be null (sizes only).
int tracyhost_alntext_batch(uint32_t n, uint32_t form, uint32_t key, uint32_t linelimit, const uint8_t* rows0, const uint8_t* rows1,
                            const uint64_t* rows_offset, const uint32_t* cols, const uint8_t* names, const uint64_t* name0_offset,
                            const uint32_t* name0_len, const uint64_t* name1_offset, const uint32_t* name1_len, const int32_t* ref_pos,
                            const uint32_t* ref_len, const uint8_t* forward, const int32_t* score, int32_t* status, uint32_t* text_len, uint8_t* text,
                            const uint64_t* text_offset, const uint64_t* text_cap, uint32_t nthreads) {
  if (form > 2 || (form == 0 && (key > 3 || linelimit < 1 || linelimit > 65535u)) || (text && (!text_offset || !text_cap))) return -1;
  if (n && (!rows0 || !rows1 || !rows_offset || !cols || !names || !name1_offset || !name1_len || !ref_pos || !ref_len || !forward || !status || !text_len))
    return -1;
  if (n && ((form != 2 && (!name0_offset || !name0_len)) || (form == 0 && !score))) return -1;
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  std::vector<std::thread> th;
  for (uint32_t w = 0; w < nthreads; ++w)
    th.emplace_back([=]() {
      AlignRows al;
      ReferenceSlice rs;
      for (uint32_t t = (uint32_t)((uint64_t)n * w / nthreads); t < (uint32_t)((uint64_t)n * (w + 1) / nthreads); ++t) {
        status[t] = 1;
        text_len[t] = 0;
        al.row0.assign(reinterpret_cast<const char*>(rows0) + rows_offset[t], cols[t]);
        al.row1.assign(reinterpret_cast<const char*>(rows1) + rows_offset[t], cols[t]);
        const std::string name1(reinterpret_cast<const char*>(names) + name1_offset[t], name1_len[t]);
        std::string name0;
        if (form != 2) name0.assign(reinterpret_cast<const char*>(names) + name0_offset[t], name0_len[t]);
        rs.forward = forward[t] != 0;
        rs.pos = (uint32_t)ref_pos[t];
        rs.chr = name1;
        TextBuf out((std::size_t)8 * cols[t] + 4096);
        if (form == 0) {
          plotAlignmentLines(out, al, rs.pos, (std::size_t)ref_len[t], rs.forward, (int32_t)key, score[t], linelimit,
                             [&](TextBuf& o) { o << name0 << std::endl; },
                             [&](TextBuf& o, int32_t, int32_t, auto&&) { o << name1 << std::endl; });
        } else if (form == 1) {
          alignFastaOut(out, name0, rs, al);
        } else {
          traceAlignJsonTail(out, rs, al);
        }
        if (out.size() > 0xffffffffull) continue;
        text_len[t] = (uint32_t)out.size();
        if (text && out.size() > text_cap[t]) { status[t] = 2; continue; }
        status[t] = 0;
        if (text) std::memcpy(text + text_offset[t], out.data(), out.size());
      }
    });
  for (auto& t : th) t.join();
  return 0;
}

// ---- the readers over a batch of file images, one file after the other per thread: traceFormat, readab / readscf (trace_io.hpp) into the
// flattened arrays of tracyhip_read_traces (the fallback for its deferred traces; tools and the command line time it beside the device
// call) ----
// status: 0 read; 1 the reader refuses the image, or a sample does not fit sample_bytes = 2; 2 a capacity is too small (sizes reported).
// format is traceFormat's.  Channels shorter than the longest are zero padded, as tracyhost_trace_get does.  Payload results may be null
// (all null: sizes only).
int tracyhost_read_batch(uint32_t n, const uint8_t* bytes, const uint64_t* file_offset, const uint32_t* file_len, uint32_t sample_bytes, int32_t* status,
                         int32_t* format, uint32_t* nsamples, uint32_t* ncalls, void* o_signal, const uint64_t* sample_offset, const uint32_t* sample_cap,
                         int32_t* o_pos, uint8_t* o_b1, uint8_t* o_b2, uint8_t* o_qual, const uint64_t* call_offset, const uint32_t* call_cap,
                         uint32_t nthreads) {
  const bool want_calls = o_pos || o_b1 || o_b2 || o_qual;
  if (n && (!bytes || !file_offset || !file_len || !status || !format || !nsamples || !ncalls)) return -1;
  if ((sample_bytes != 2 && sample_bytes != 4) || (o_signal && (!sample_offset || !sample_cap)) || (want_calls && (!call_offset || !call_cap))) return -1;
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  std::vector<std::thread> th;
  for (uint32_t w = 0; w < nthreads; ++w)
    th.emplace_back([=]() {
      for (uint32_t t = (uint32_t)((uint64_t)n * w / nthreads); t < (uint32_t)((uint64_t)n * (w + 1) / nthreads); ++t) {
        detail::FileBytes f;
        f.view(bytes + file_offset[t], file_len[t]);
        status[t] = 1;
        nsamples[t] = ncalls[t] = 0;
        const int32_t ft = format[t] = traceFormat(f);
        Trace tr;
        if (!(ft == 0 ? readab(f, tr) : ft == 1 ? readscf(f, tr) : false)) continue;
        size_t ns = 0;
        for (auto const& c : tr.traceACGT) ns = std::max(ns, c.size());
        const size_t nc = tr.basecallpos.size();
        bool fits = ns <= 0xffffffffull && nc <= 0xffffffffull;
        if (fits && sample_bytes == 2)
          for (auto const& c : tr.traceACGT)
            for (int32_t v : c) fits = fits && v >= -32768 && v <= 32767;
        if (!fits) continue;
        nsamples[t] = (uint32_t)ns; ncalls[t] = (uint32_t)nc;
        if ((o_signal && ns > sample_cap[t]) || (want_calls && nc > call_cap[t])) { status[t] = 2; continue; }
        status[t] = 0;
        if (o_signal)
          for (size_t k = 0; k < 4; ++k) {
            const uint64_t at = sample_offset[t] + (uint64_t)k * ns;
            for (size_t x = 0; x < ns; ++x) {
              const int32_t v = (k < tr.traceACGT.size() && x < tr.traceACGT[k].size()) ? tr.traceACGT[k][x] : 0;
              if (sample_bytes == 4) static_cast<int32_t*>(o_signal)[at + x] = v;
              else static_cast<int16_t*>(o_signal)[at + x] = (int16_t)v;
            }
          }
        if (!want_calls) continue;
        const uint64_t co = call_offset[t];
        if (o_pos && nc) std::memcpy(o_pos + co, tr.basecallpos.data(), 4 * nc);
        auto put = [&](uint8_t* dst, const void* src, size_t have) {  // (nc bytes: what the Trace holds, zeros behind it)
          if (!dst) return;
          std::memset(dst + co, 0, nc);
          if (have) std::memcpy(dst + co, src, std::min(nc, have));
        };
        put(o_b1, tr.basecalls1.data(), tr.basecalls1.size());
        put(o_b2, tr.basecalls2.data(), tr.basecalls2.size());
        put(o_qual, tr.qual.data(), tr.qual.size());
      }
    });
  for (auto& t : th) t.join();
  return 0;
}

// ---- the text printed from the decompose results, one trace after the other per thread: writeDecomposition, traceAlleleAlignJsonTail
// and vcfRecordLines (indigo_out.hpp) into a TextBuf over the job of tracyhip_render_decompositions, host arrays throughout (the
// fallback for its deferred traces; tools/dcptext_device_line.py times it beside the device call) ----
// The forms and what each reads are the device call's (include/tracy_hip.h).  Long names, rows beyond 2^22 columns and any number of
// basecalls are printed.  status: 0 answered; 1 the writers would index outside an array (no basecall, trim_left + breakpoint or a
// variant's call index at or beyond bc_len, var_n > max_variants, a ref or alt outside the trace's text region) or the text does not
// fit 32 bits; 2 text_cap is too small (text_len reported).  out->text may be null (sizes only).
int tracyhost_dcptext_batch(const tracyhip_dcptext_job* job, const tracyhip_render_result* res, uint32_t nthreads) {
  if (!job || !res || job->form > 2 || (res->text && (!res->text_offset || !res->text_cap))) return -1;
  const uint32_t n = job->n, form = job->form;
  const bool table = form != TRACYHIP_DCPTEXT_VCF, calls = form != TRACYHIP_DCPTEXT_DECOMP, json = form == TRACYHIP_DCPTEXT_JSON;
  if (n && (!res->status || !res->text_len)) return -1;
  if (n && table && (!job->dcp_indel || !job->dcp_err || !job->dcp_offset || !job->dcp_rows)) return -1;
  if (n && calls && (!job->bcpos || !job->estqual || !job->bc_offset || !job->bc_len || !job->var || !job->var_text || !job->var_n || !job->forward ||
                     !job->trim_left || !job->trim_right || !job->names || !job->chr_offset[0] || !job->chr_len[0] || job->max_variants < 1 || job->max_text < 2))
    return -1;
  if (n && json) {
    for (int k = 0; k < 3; ++k)
      if (!job->rows0[k] || !job->rows1[k] || !job->rows_offset[k] || !job->cols[k] || !job->score[k]) return -1;
    if (!job->ref_pos[0] || !job->ref_pos[1] || !job->breakpoint || !job->indelshift || !job->chr_offset[1] || !job->chr_len[1] || !job->frac_offset[0] ||
        !job->frac_len[0] || !job->frac_offset[1] || !job->frac_len[1])
      return -1;
  }
  if (nthreads == 0) nthreads = tracy_amd::usable_threads();
  const tracyhip_dcptext_job j = *job;
  const tracyhip_render_result o = *res;
  std::vector<std::thread> th;
  for (uint32_t w = 0; w < nthreads; ++w)
    th.emplace_back([=]() {
      BaseCalls bc;
      AlleleReport r;
      ReportConfig c;
      c.qualCut = (uint16_t)j.qual_cut;
      auto name = [&](const uint64_t* off, const uint32_t* len, uint32_t t) { return std::string(reinterpret_cast<const char*>(j.names) + off[t], len[t]); };
      for (uint32_t t = (uint32_t)((uint64_t)n * w / nthreads); t < (uint32_t)((uint64_t)n * (w + 1) / nthreads); ++t) {
        o.status[t] = 1;
        o.text_len[t] = 0;
        std::size_t room = 4096;
        if (table) {
          r.dcp.clear();
          for (uint32_t i = 0; i < j.dcp_rows[t]; ++i) r.dcp.emplace_back(j.dcp_indel[j.dcp_offset[t] + i], j.dcp_err[j.dcp_offset[t] + i]);
          room += (std::size_t)48 * j.dcp_rows[t];
        }
        if (calls) {
          const uint32_t nc = j.bc_len[t];
          if (nc == 0) continue;
          c.trimLeft = (uint16_t)j.trim_left[t];
          c.trimRight = (uint16_t)j.trim_right[t];
          bc.bcPos.assign(j.bcpos + j.bc_offset[t], j.bcpos + j.bc_offset[t] + nc);
          bc.estQual.assign(j.estqual + j.bc_offset[t], j.estqual + j.bc_offset[t] + nc);
          bc.primary.assign(nc, 'N');  // (the writers read its size alone)
          r.rs1.forward = r.rs2.forward = j.forward[t] != 0;
          r.rs1.chr = name(j.chr_offset[0], j.chr_len[0], t);
          const uint32_t at = j.var_index ? j.var_index[t] : t;
          const uint32_t nv = j.var_n[at];
          if (nv > j.max_variants) continue;
          const tracyhip_variant* rec = j.var + (uint64_t)at * j.max_variants;
          const char* vt = reinterpret_cast<const char*>(j.var_text) + (uint64_t)at * j.max_text;
          r.var.clear();
          bool ok = true;
          for (uint32_t i = 0; ok && i < nv; ++i) {
            ok = variantCallIndex(c, bc, r.rs1.forward, rec[i].basenum) < nc && (uint64_t)rec[i].ref_off + rec[i].ref_len <= j.max_text &&
                 (uint64_t)rec[i].alt_off + rec[i].alt_len <= j.max_text;
            if (ok)
              r.var.push_back(Variant{rec[i].pos, rec[i].basenum, rec[i].gt, r.rs1.chr, std::string(vt + rec[i].ref_off, rec[i].ref_len),
                                      std::string(vt + rec[i].alt_off, rec[i].alt_len), "."});
            room += 256 + r.rs1.chr.size() + rec[i].ref_len + rec[i].alt_len;
          }
          if (!ok) continue;
        }
        std::string frac[2];
        if (json) {
          r.bp.breakpoint = j.breakpoint[t];
          r.bp.indelshift = j.indelshift[t] != 0;
          if ((uint32_t)(c.trimLeft + r.bp.breakpoint) >= j.bc_len[t]) continue;
          r.rs2.chr = name(j.chr_offset[1], j.chr_len[1], t);
          r.rs1.pos = j.ref_pos[0][t];
          r.rs2.pos = j.ref_pos[1][t];
          AlignRows* al[3] = {&r.align1, &r.align2, &r.align3};
          for (int k = 0; k < 3; ++k) {
            al[k]->row0.assign(reinterpret_cast<const char*>(j.rows0[k]) + j.rows_offset[k][t], j.cols[k][t]);
            al[k]->row1.assign(reinterpret_cast<const char*>(j.rows1[k]) + j.rows_offset[k][t], j.cols[k][t]);
            room += (std::size_t)2 * j.cols[k][t];
          }
          r.a1Score = j.score[0][t]; r.a2Score = j.score[1][t]; r.a3Score = j.score[2][t];
          for (int k = 0; k < 2; ++k) frac[k] = name(j.frac_offset[k], j.frac_len[k], t);
          room += r.rs1.chr.size() + r.rs2.chr.size() + frac[0].size() + frac[1].size();
        }
        TextBuf out(room);
        if (form == TRACYHIP_DCPTEXT_DECOMP) writeDecomposition(out, r.dcp);
        else if (json) traceAlleleAlignJsonTail(out, c, bc, r, [&](TextBuf& b, int k) { b << frac[k]; });
        else vcfRecordLines(out, c, bc, r.var, r.rs1.forward);
        if (out.size() > 0xffffffffull) continue;
        o.text_len[t] = (uint32_t)out.size();
        if (o.text && out.size() > o.text_cap[t]) { o.status[t] = 2; continue; }
        o.status[t] = 0;
        if (o.text) std::memcpy(o.text + o.text_offset[t], out.data(), out.size());
      }
    });
  for (auto& t : th) t.join();
  return 0;
}

// threads the batch entry points start when the caller passes nthreads = 0
uint32_t tracyhost_usable_threads() { return tracy_amd::usable_threads(); }

}  // extern "C"
