// variants_wave_asan.cpp -- a stand-alone run of tracy_amd/csrc/variants_wave.h on the host wave under the sanitizers (not a pytest test):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o variants_wave_asan tests/cpp/variants_wave_asan.cpp
// The named cases of tests/variants_cases.py and seeded random alignment pairs with gap runs across the 64-column rounds, every buffer
// (rows, event lists, records, text) allocated at exactly the size the kernel is promised: a read or write past one is a report.
// Every result is checked for what must hold of it whatever the input (tests/test_emu_variants.py compares the values with the
// oracle).  Exit code 0 and "ok": no sanitizer report, no broken invariant.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../tracy_amd/csrc/variants_wave.h"

using namespace tracyhip;

#include "../emu/host_wave.h"

#define REQUIRE(x)                                                        \
  do {                                                                    \
    if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); return 1; } \
  } while (0)

namespace {
struct Aln { std::string row0, row1; int32_t pos; };
struct Result { std::vector<tracyhip_variant> var; std::vector<uint8_t> text; uint32_t n, flags; };

// rows in heap blocks of exactly their length
Result run(const Aln& a, const Aln& b, bool forward, uint32_t bc_len, uint32_t max_variants, uint32_t max_text) {
  std::unique_ptr<uint8_t[]> r[4];
  const std::string* s[4] = {&a.row0, &a.row1, &b.row0, &b.row1};
  for (int i = 0; i < 4; ++i) {
    r[i].reset(new uint8_t[s[i]->size()]);
    std::memcpy(r[i].get(), s[i]->data(), s[i]->size());
  }
  VarTrace t{};
  t.row0[0] = r[0].get(); t.row1[0] = r[1].get(); t.len[0] = (uint32_t)a.row0.size(); t.pos0[0] = a.pos;
  t.row0[1] = r[2].get(); t.row1[1] = r[3].get(); t.len[1] = (uint32_t)b.row0.size(); t.pos0[1] = b.pos;
  t.forward = forward; t.bc_len = bc_len;
  std::unique_ptr<VarEvent[]> ev(new VarEvent[2 * (size_t)max_variants]);
  Result res;
  res.var.resize(max_variants);
  res.text.assign(max_text, 0xA5);
  res.n = res.flags = 0x5a5a5a5a;
  WaveShared sh;
  sh.run([&](uint32_t lane) {
    HostWave w{lane, &sh};
    variants_wave(w, t, 20, 20, max_variants, max_text, ev.get(), res.var.data(), res.text.data(), &res.n, &res.flags);
  });
  return res;
}

// what holds of every result: sorted by (pos, basenum), text packed in record order inside max_text, gt 1 or 2, pos > 0, no N in ref
int check(const Result& r, uint32_t max_variants, uint32_t max_text) {
  REQUIRE(r.flags <= 1 && r.n <= max_variants && (r.flags == 0 || r.n == 0));
  uint32_t at = 0;
  for (uint32_t i = 0; i < r.n; ++i) {
    const tracyhip_variant& v = r.var[i];
    REQUIRE(v.pos > 0 && v.basenum >= 0 && (v.gt == 1 || v.gt == 2));
    REQUIRE(v.ref_len >= 1 && v.alt_len >= 1 && (v.ref_len == 1 || v.alt_len == 1));
    REQUIRE(v.ref_off == at && v.alt_off == at + v.ref_len);
    at += v.ref_len + v.alt_len;
    REQUIRE(at <= max_text);
    for (uint32_t k = 0; k < v.ref_len; ++k) REQUIRE(r.text[v.ref_off + k] != 'N' && r.text[v.ref_off + k] != 'n' && r.text[v.ref_off + k] != '-');
    for (uint32_t k = 0; k < v.alt_len; ++k) REQUIRE(r.text[v.alt_off + k] != '-' && r.text[v.alt_off + k] != 0xA5);
    if (v.ref_len > 1 || v.alt_len > 1) REQUIRE(r.text[v.ref_off] == r.text[v.alt_off]);  // the anchor
    if (i) REQUIRE(r.var[i - 1].pos < v.pos || (r.var[i - 1].pos == v.pos && r.var[i - 1].basenum <= v.basenum));
  }
  for (uint32_t k = at; k < max_text; ++k) REQUIRE(r.text[k] == 0xA5);
  return 0;
}

std::string reps(const char* unit, size_t n) { std::string s; while (s.size() < n) s += unit; return s.substr(0, n); }
}  // namespace

int main() {
  const Aln none{"", "", 0};
  std::vector<std::pair<Aln, Aln>> named = {
      {{"----", "ACGT", 5}, none}, {none, none},
      {{"--TACGG--", "AAAACGTAA", 10}, none}, {{"ACGTA", "--GTC", 10}, none}, {{"ACGTAA", "ACCT--", 10}, none},
      {{"---ACGT", "TTTACCT", 100}, none}, {{"ACGG--TA", "AC--TTTA", 10}, none}, {{"AC--GGTA", "ACTT--TA", 10}, none},
      {{"TC" + reps("GA", 80) + "---TA", "TC" + std::string(80, '-') + "ACGTA", 10}, none},
      {{"ACGTAC", "ANGnAG", 10}, none}, {{"AC--GT-A", "ACTNGTnA", 10}, none}, {{"AC-GT", "ANTGT", 10}, none},
      {{"ANGTNNCA", "ACGT--CA", 10}, none}, {{"A-CGT", "-TCGA", 0}, none}, {{"TC-GTA", "ACTGAA", -3}, none},
      {{"--TAC-GG-", "AAAACTGTA", 1 << 30}, {"TAC-GG", "AACTGT", (1 << 30) + 2}},
      {{"ACGTACGTAC--GTAC", "ACGTACCTACTTGTAC", 40}, {"ACTTGTACGTAC--GTAC", "AC--GTACCTACTTGTAC", 40}},
      {{"ACGTCCGT", "ACGTACGT", 40}, {"ACGTGCGT", "ACGTACGT", 40}},
  };
  for (uint32_t n : {1u, 64u, 65u, 130u}) {  // runs that start in column 63 / 3 / 61 and cross the rounds
    const std::string full = reps("ACGT", n + 70);
    std::string d = full, i = full;
    d.replace(63, n, std::string(n, '-'));
    i.replace(61, n, std::string(n, '-'));
    named.push_back({{d, full, 7}, {full, i, 7}});
  }
  for (uint32_t L : {1u, 63u, 64u, 65u, 127u, 128u, 129u, 200u}) {
    std::string r0(L, 'G'), r1(L, 'G');
    for (uint32_t j : {0u, L / 2, L - 1}) { r0[j] = 'C'; r1[j] = 'A'; }
    named.push_back({{r0, r1, 3}, {r1, r1, 3}});
  }
  uint64_t records = 0, flagged = 0;
  for (auto const& c : named)
    for (uint32_t maxv : {1u, 2u, 64u})
      for (uint32_t maxt : {2u, 13u, 1024u}) {
        const Result r = run(c.first, c.second, maxv & 1u, 321, maxv, maxt);
        if (check(r, maxv, maxt)) return 1;
        records += r.n; flagged += r.flags;
      }
  // seeded random pairs: up to 300 columns, gap runs up to 140, N among the letters
  std::mt19937 rng(20240519u);
  auto letter = [&]() { return "ACGTACGTACGTACGTN"[rng() % 17]; };
  auto random_aln = [&](int32_t pos) {
    Aln a{"", "", pos};
    const uint32_t want = 1 + rng() % 300;
    while (a.row0.size() < want) {
      const uint32_t u = rng() % 100;
      uint32_t n = u < 86 ? 1 + rng() % 30 : (rng() % 7 == 0 ? 1 + rng() % 140 : 1 + rng() % 4);
      n = std::min<uint32_t>(n, want - (uint32_t)a.row0.size());
      for (uint32_t k = 0; k < n; ++k) {
        const char r = letter();
        if (u < 86) { a.row0.push_back(rng() % 16 ? r : letter()); a.row1.push_back(r); }
        else if (u < 93) { a.row0.push_back('-'); a.row1.push_back(r); }
        else { a.row0.push_back(r); a.row1.push_back('-'); }
      }
    }
    return a;
  };
  for (int iter = 0; iter < 400; ++iter) {
    const int32_t pos = (int32_t)(rng() % 5000);
    const Aln a = random_aln(pos);
    Aln b = iter % 2 ? a : random_aln(pos);
    if (iter % 2 && !b.row0.empty()) {
      char& ch = b.row0[rng() % b.row0.size()];
      if (ch != '-') ch = "ACGT"[rng() % 4];
    }
    const uint32_t maxv = iter % 5 == 0 ? 3 : 128, maxt = iter % 7 == 0 ? 40 : 4096;
    const Result r = run(a, b, iter & 1, 600, maxv, maxt);
    if (check(r, maxv, maxt)) return 1;
    records += r.n; flagged += r.flags;
  }
  REQUIRE(records > 2000 && flagged > 50);
  std::printf("ok: %llu records, %llu truncated traces\n", (unsigned long long)records, (unsigned long long)flagged);
  return 0;
}
