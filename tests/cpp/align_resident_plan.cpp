// align_resident_plan.cpp -- a stand-alone run of tracy_amd/cli/align_resident_plan.h (no HIP, no C ABI, its own main;
// tests/test_align_resident_plan.py builds it plain and with the sanitizers and runs it as a program):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o align_resident_plan tests/cpp/align_resident_plan.cpp
// It plans blocks of manifest lines of mixed reference kinds and checks: the regions of every payload are consecutive, disjoint and inside
// their buffers; lines that share a wildtype or a FASTA share one entry / one record through ref_index; blocks without FASTA lines,
// without wildtype lines and of host-path lines alone; the answered set narrows stage by stage and never grows; the text fragments of a
// row lie in file order and a dropped row has none; totals that leave 64 bits are refused.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../tracy_amd/cli/align_resident_plan.h"

using namespace tracy_amd::resident;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// off[0] = 0, off[i + 1] = off[i] + room[i] * scale: consecutive, disjoint, inside [0, off[n])
template <class Len>
static void check_regions(std::vector<uint64_t> const& off, std::vector<Len> const& room, uint64_t scale) {
  CHECK(off.size() == room.size() + 1);
  if (off.size() != room.size() + 1) return;
  CHECK(off[0] == 0);
  for (std::size_t i = 0; i < room.size(); ++i) {
    CHECK(off[i + 1] == off[i] + (uint64_t)room[i] * scale);
    CHECK(off[i + 1] <= off[room.size()]);
  }
}

struct Line {
  int32_t kind;
  std::string ref;
};

static BlockPlan split(std::vector<Line> const& lines) {
  std::vector<int32_t> kinds;
  std::vector<std::string> paths;
  for (Line const& l : lines) { kinds.push_back(l.kind); paths.push_back(l.ref); }
  BlockPlan p;
  p.split_references(kinds, paths);
  return p;
}

// a block as the command plans it, every entry of `len` file bytes but the ones in `unreadable`
static bool entries(BlockPlan& p, uint32_t len, std::vector<uint32_t> const& unreadable = {}) {
  const uint32_t ne = p.nentries();
  std::vector<uint32_t> flen(ne, 0), scap(ne, 0), ccap(ne, 0);
  for (uint32_t e = 0; e < ne; ++e) {
    if (e < p.nlines && p.ref_of[e] == kNone) continue;  // a host-path line is not read
    flen[e] = len + 3 * e;
    for (uint32_t u : unreadable) if (u == e) flen[e] = 0;
    scap[e] = flen[e] / 8; ccap[e] = flen[e] / 2;
  }
  return p.layout_entries(flen, scap, ccap);
}

static void mixed_block() {
  // 0 F:a  1 W:x  2 F:b  3 G  4 F:a  5 W:y  6 W:x  7 ?  8 F:c (too long)  9 W:x  10 F:b
  const std::vector<Line> lines = {{REF_FASTA, "a.fa"}, {REF_WILDTYPE, "x.ab1"}, {REF_FASTA, "b.fa"},   {REF_GENOME, "g.fa.gz"},
                                   {REF_FASTA, "a.fa"}, {REF_WILDTYPE, "y.ab1"}, {REF_WILDTYPE, "x.ab1"}, {REF_UNKNOWN, "junk"},
                                   {REF_FASTA, "c.fa"}, {REF_WILDTYPE, "x.ab1"}, {REF_FASTA, "b.fa"}};
  BlockPlan p = split(lines);
  CHECK(p.nlines == 11 && p.nfasta() == 3 && p.nwildtypes() == 2 && p.nentries() == 13);
  CHECK(p.fasta_line == (std::vector<uint32_t>{0, 2, 8}) && p.wildtype_line == (std::vector<uint32_t>{1, 5}));
  CHECK(p.ref_of == (std::vector<uint32_t>{0, 0, 1, kNone, 0, 1, 0, kNone, 2, 0, 1}));
  CHECK(p.wildtype_entry(0) == 11 && p.wildtype_entry(1) == 12);
  CHECK(entries(p, 1000));
  check_regions(p.file_off, p.file_len, 1);
  check_regions(p.sample_off, p.sample_cap, 4);
  check_regions(p.call_off, p.call_cap, 1);
  CHECK(p.file_len[3] == 0 && p.file_len[7] == 0 && p.file_len[11] != 0 && p.file_len[12] != 0);
  for (uint32_t e = 0; e < p.nentries(); ++e) CHECK(p.profile_off(e) == 6 * p.call_off[e] && p.profile_off(e) + 6ull * p.call_cap[e] <= 6 * p.call_off[p.nentries()]);

  // read + basecall: line 4's trims take all of it, line 5's wildtype (entry 12) was deferred, FASTA c is too long
  const uint32_t ne = p.nentries();
  std::vector<uint8_t> entry_ok(ne, 1);
  entry_ok[3] = entry_ok[7] = 0;
  entry_ok[12] = 0;
  std::vector<uint32_t> bc_len(ne, 500), tl(p.nlines, 50), tr(p.nlines, 50);
  tl[4] = 250; tr[4] = 250;
  p.open_rows(entry_ok, bc_len, tl, tr, {1, 1, 0});
  CHECK(p.row_line == (std::vector<uint32_t>{0, 1, 2, 6, 9, 10}));
  CHECK(p.nalive() == 6 && p.alive.size() == 6);
  CHECK(p.fasta_rows == (std::vector<uint32_t>{0, 2, 5}) && p.wildtype_rows == (std::vector<uint32_t>{1, 3, 4}));
  CHECK(p.fasta_used == (std::vector<uint32_t>{0, 1}) && p.fasta_ref_index == (std::vector<uint32_t>{0, 1, 1}));
  CHECK(p.wildtype_used == (std::vector<uint32_t>{0}) && p.wildtype_ref_index == (std::vector<uint32_t>{0, 0, 0}));  // three lines, one wildtype
  for (uint32_t i = 0; i < p.nlines; ++i) {
    const uint32_t k = p.row_of_line[i];
    CHECK((k == kNone) == (i == 3 || i == 4 || i == 5 || i == 7 || i == 8));
    if (k != kNone) CHECK(p.row_line[k] == i);
  }

  // op strings / rows, the FASTA records, the slices
  std::vector<uint32_t> calls(6, 500), refc = {2000, 480, 3000, 480, 480, 3000};
  CHECK(p.layout_ops(calls, refc));
  for (uint32_t k = 0; k < 6; ++k) CHECK(p.ops_cap[k] == calls[k] + refc[k]);
  check_regions(p.ops_off, p.ops_cap, 1);
  CHECK(p.layout_fasta(std::vector<uint32_t>{2000, 3000}) && p.fasta_off == (std::vector<uint64_t>{0, 2000, 5000}));
  CHECK(!p.layout_fasta(std::vector<uint32_t>{2000}));
  CHECK(p.layout_slices(std::vector<uint32_t>{700, 650, 0}) && p.slice_off == (std::vector<uint64_t>{0, 700, 1350, 1350}));
  CHECK(!p.layout_slices(std::vector<uint32_t>{700, 650}));

  // the answered set narrows: the pad defers row 3, a render defers row 0; nothing comes back
  std::vector<uint8_t> ok(6, 1);
  ok[3] = 0;
  p.keep(ok);
  CHECK(p.nalive() == 5 && !p.alive[3]);
  std::vector<uint32_t> nso = {6100, 6200, 6300, 6400, 6500, 6600}, nco = {510, 520, 530, 540, 550, 560};
  CHECK(p.layout_pad(nso, nco));
  CHECK(p.pad_sample_cap[3] == 0 && p.pad_call_cap[3] == 0 && p.pad_sample_cap[4] == 6500);
  check_regions(p.pad_sample_off, p.pad_sample_cap, 4);
  check_regions(p.pad_call_off, p.pad_call_cap, 1);
  ok.assign(6, 1);
  ok[0] = 0;
  p.keep(ok);
  CHECK(p.nalive() == 4 && !p.alive[0] && !p.alive[3]);
  ok.assign(6, 1);  // (a later stage that answers everything revives nothing)
  p.keep(ok);
  CHECK(p.nalive() == 4 && !p.alive[0] && !p.alive[3]);

  // names: the shared first header line at 0, then stem / second header line / chr of every row
  std::vector<uint32_t> sl = {3, 4, 5, 6, 7, 8}, hl = {30, 31, 32, 33, 34, 35}, cl = {6, 8, 6, 8, 8, 6};
  CHECK(p.layout_names(4, sl, hl, cl));
  uint64_t at = 4;
  for (uint32_t k = 0; k < 6; ++k) {
    CHECK(p.stem_off[k] == at && p.head1_off[k] == at + sl[k] && p.chr_off[k] == at + sl[k] + hl[k]);
    at += sl[k] + hl[k] + cl[k];
  }
  CHECK(p.names_bytes == at);

  // text: the fragments of a row in file order (.abif, .align.fa, .txt, the two parts of the .json), rows in row order, none for a dropped row
  std::vector<uint32_t> len[FRAG_COUNT];
  for (uint32_t f = 0; f < FRAG_COUNT; ++f)
    for (uint32_t k = 0; k < 6; ++k) len[f].push_back(1000 * (f + 1) + k);
  CHECK(p.layout_text(len));
  at = 0;
  for (uint32_t k = 0; k < 6; ++k)
    for (uint32_t f = 0; f < FRAG_COUNT; ++f) {
      CHECK(p.text_off[f][k] == at);
      CHECK(p.text_cap[f][k] == (p.alive[k] ? len[f][k] : 0));
      if (f) CHECK(p.text_off[f][k] == p.text_off[f - 1][k] + p.text_cap[f - 1][k]);
      at += p.text_cap[f][k];
      CHECK(at <= p.text_bytes);
    }
  CHECK(p.text_bytes == at);
  CHECK(FRAG_ABIF < FRAG_FASTA && FRAG_FASTA < FRAG_PLOT && FRAG_PLOT < FRAG_JSON_HEAD && FRAG_JSON_HEAD < FRAG_GAPPED &&
        FRAG_GAPPED < FRAG_JSON_CLOSE && FRAG_JSON_CLOSE < FRAG_TAIL && FRAG_TAIL + 1 == FRAG_COUNT);
  // every file is one span: .abif, .align.fa and .txt a fragment each, the .json its four parts in order; the files of a row follow each other
  for (uint32_t k = 0; k < 6; ++k) {
    CHECK(p.out_off(FILE_ABIF, k) == p.text_off[FRAG_ABIF][k] && p.out_len(FILE_ABIF, k) == p.text_cap[FRAG_ABIF][k]);
    CHECK(p.out_off(FILE_FASTA, k) == p.text_off[FRAG_FASTA][k] && p.out_len(FILE_FASTA, k) == p.text_cap[FRAG_FASTA][k]);
    CHECK(p.out_off(FILE_PLOT, k) == p.text_off[FRAG_PLOT][k] && p.out_len(FILE_PLOT, k) == p.text_cap[FRAG_PLOT][k]);
    CHECK(p.out_off(FILE_JSON, k) == p.text_off[FRAG_JSON_HEAD][k]);
    CHECK(p.out_len(FILE_JSON, k) == p.text_cap[FRAG_JSON_HEAD][k] + p.text_cap[FRAG_GAPPED][k] + p.text_cap[FRAG_JSON_CLOSE][k] + p.text_cap[FRAG_TAIL][k]);
    for (uint32_t f = 0; f + 1 < FILE_COUNT; ++f) CHECK(p.out_off(f + 1, k) == p.out_off(f, k) + p.out_len(f, k));
    CHECK(p.out_off(FILE_JSON, k) + p.out_len(FILE_JSON, k) == (k + 1 < 6 ? p.out_off(FILE_ABIF, k + 1) : p.text_bytes));
    if (!p.alive[k]) for (uint32_t f = 0; f < FILE_COUNT; ++f) CHECK(p.out_len(f, k) == 0);
  }
  len[2].pop_back();
  CHECK(!p.layout_text(len));
}

static void one_kind_blocks() {
  {  // no FASTA lines: two lines on one wildtype, one on another
    BlockPlan p = split({{REF_WILDTYPE, "x"}, {REF_WILDTYPE, "x"}, {REF_WILDTYPE, "y"}});
    CHECK(p.nfasta() == 0 && p.nwildtypes() == 2 && p.nentries() == 5);
    CHECK(entries(p, 800));
    p.open_rows(std::vector<uint8_t>(5, 1), std::vector<uint32_t>(5, 300), std::vector<uint32_t>(3, 0), std::vector<uint32_t>(3, 0), {});
    CHECK(p.nrows() == 3 && p.fasta_rows.empty() && p.wildtype_rows.size() == 3 && p.wildtype_ref_index == (std::vector<uint32_t>{0, 0, 1}));
    CHECK(p.layout_fasta(std::vector<uint32_t>{}) && p.fasta_off == std::vector<uint64_t>{0});
    CHECK(p.layout_slices(std::vector<uint32_t>{}) && p.slice_off == std::vector<uint64_t>{0});
  }
  {  // no wildtype lines: the entries are the lines
    BlockPlan p = split({{REF_FASTA, "a"}, {REF_FASTA, "b"}, {REF_FASTA, "a"}});
    CHECK(p.nfasta() == 2 && p.nwildtypes() == 0 && p.nentries() == 3);
    CHECK(entries(p, 800, {1}));  // (the second file could not be read)
    CHECK(p.file_len[1] == 0 && p.file_off[1] == p.file_off[2]);
    std::vector<uint8_t> entry_ok = {1, 0, 1};
    p.open_rows(entry_ok, {300, 0, 300}, {50, 50, 50}, {50, 50, 50}, {1, 1});
    CHECK(p.row_line == (std::vector<uint32_t>{0, 2}) && p.wildtype_rows.empty());
    CHECK(p.fasta_used == std::vector<uint32_t>{0} && p.fasta_ref_index == (std::vector<uint32_t>{0, 0}));  // two lines, one record
  }
  {  // host-path lines alone: nothing to read, no rows, every layout is empty and valid
    BlockPlan p = split({{REF_GENOME, "g"}, {REF_UNKNOWN, "u"}, {REF_GENOME, "g"}});
    CHECK(p.nfasta() == 0 && p.nwildtypes() == 0 && p.nentries() == 3);
    CHECK(entries(p, 800));
    CHECK(p.file_off[3] == 0 && p.sample_off[3] == 0 && p.call_off[3] == 0);
    p.open_rows(std::vector<uint8_t>(3, 0), std::vector<uint32_t>(3, 0), std::vector<uint32_t>(3, 0), std::vector<uint32_t>(3, 0), {});
    CHECK(p.nrows() == 0 && p.nalive() == 0);
    for (uint32_t i = 0; i < 3; ++i) CHECK(p.row_of_line[i] == kNone);
    CHECK(p.layout_ops({}, {}) && p.layout_pad({}, {}) && p.layout_names(4, {}, {}, {}) && p.names_bytes == 4);
    std::vector<uint32_t> len[FRAG_COUNT];
    CHECK(p.layout_text(len) && p.text_bytes == 0);
  }
  {  // an empty block
    BlockPlan p = split({});
    CHECK(p.nentries() == 0 && entries(p, 1) && p.file_off == std::vector<uint64_t>{0});
  }
  {  // a line without basecalls, and a wildtype line whose wildtype has none
    BlockPlan p = split({{REF_FASTA, "a"}, {REF_WILDTYPE, "x"}, {REF_FASTA, "a"}});
    CHECK(entries(p, 800));
    p.open_rows(std::vector<uint8_t>(4, 1), {0, 300, 300, 0}, {0, 0, 0}, {0, 0, 0}, {1});
    CHECK(p.row_line == std::vector<uint32_t>{2});
    p.open_rows(std::vector<uint8_t>(4, 1), {1, 300, 300, 10}, {0, 0, 299, 0}, {0, 0, 0, 0}, {1});  // (299 + 0 < 300: the trims just fit)
    CHECK(p.row_line == (std::vector<uint32_t>{0, 1, 2}));
    p.open_rows(std::vector<uint8_t>(4, 1), {1, 300, 300, 10}, {0, 0, 299, 0}, {0, 0, 1, 0}, {1});
    CHECK(p.row_line == (std::vector<uint32_t>{0, 1}));
    p.open_rows(std::vector<uint8_t>(4, 1), {1, 300, 300, 10}, {0xffffffffu, 0, 0, 0}, {0xffffffffu, 0, 0, 0}, {1});  // (the sum does not wrap)
    CHECK(p.row_line == (std::vector<uint32_t>{1, 2}));
  }
}

static void beyond_64_bits() {
  uint64_t acc = UINT64_MAX - 5;
  CHECK(add64(acc, 5) && acc == UINT64_MAX && !add64(acc, 1) && acc == UINT64_MAX);
  uint64_t prod = 0;
  CHECK(mul64(1ull << 32, 1ull << 31, prod) && prod == 1ull << 63 && !mul64(1ull << 32, 1ull << 32, prod) && mul64(0, UINT64_MAX, prod) && prod == 0);
  std::vector<uint64_t> off;
  CHECK(prefix_offsets(std::vector<uint64_t>{UINT64_MAX / 2, UINT64_MAX / 2}, 1, 1, off));
  CHECK(!prefix_offsets(std::vector<uint64_t>{UINT64_MAX / 2, UINT64_MAX / 2, 2}, 1, 1, off));  // a partial sum
  CHECK(!prefix_offsets(std::vector<uint64_t>{UINT64_MAX / 2}, 4, 1, off));                    // an element count
  CHECK(!prefix_offsets(std::vector<uint64_t>{UINT64_MAX / 8}, 1, 24, off));                   // the bytes of the total
  // the command's lengths are 32-bit, so its totals stay far below 64 bits; a block that does leave them is refused all the same
  BlockPlan p = split({{REF_FASTA, "a"}, {REF_FASTA, "a"}});
  p.open_rows(std::vector<uint8_t>(2, 1), {10, 10}, {0, 0}, {0, 0}, {1});
  CHECK(p.nrows() == 2);
  CHECK(!p.layout_ops({0xffffffffu, 1}, {1, 1}));  // a region beyond the 32-bit lengths of the calls
  CHECK(p.layout_ops({0xfffffffeu, 1}, {1, 1}) && p.ops_off[2] == 0x100000001ull);
  CHECK(!p.layout_ops({1}, {1, 1}) && !p.layout_pad({1}, {1, 1}) && !p.layout_names(4, {1}, {1, 1}, {1, 1}));
  CHECK(!p.layout_entries({1}, {1}, {1}));  // (two entries)
  // the plan's own layouts refuse totals that leave 64 bits (lengths wider than the command's, to get there with two rows)
  CHECK(p.layout_slices(std::vector<uint64_t>{UINT64_MAX - 1, 1}) && p.slice_off[2] == UINT64_MAX);
  CHECK(!p.layout_slices(std::vector<uint64_t>{UINT64_MAX - 1, 2}));
  CHECK(p.fasta_used.size() == 1 && p.layout_fasta(std::vector<uint64_t>{UINT64_MAX}) && !p.layout_fasta(std::vector<uint64_t>{UINT64_MAX, 1}));
}

int main() {
  mixed_block();
  one_kind_blocks();
  beyond_64_bits();
  if (failures) {
    std::printf("align_resident_plan: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("align_resident_plan: ok\n");
  return 0;
}
