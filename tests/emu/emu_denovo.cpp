// emu_denovo.cpp -- host execution of what tracyhip_denovo_traces decides and counts between its dynamic programs (TEST
// INFRASTRUCTURE ONLY): the planning header tracy_amd/csrc/denovo_plan.h as denovo.hip calls it, and the 's' count body of
// assemble_wave.h on the 64-fiber host wave.  The merge / profile / consensus drivers are emu_assemble.cpp's, one copy.
#include "emu_assemble.cpp"

#include "../../tracy_amd/csrc/denovo_plan.h"

extern "C" {

// T: 4 K K entries (denovo_table_index); rev: K bytes; d: K x K, the matrix revSeqBasedOnDist ends with
int emu_denovo_strands(const int32_t* T, uint32_t K, uint8_t* rev, int32_t* d) {
  std::vector<uint8_t> r;
  std::vector<int32_t> m;
  denovo_strands(T, K, r, m);
  if (K) {
    std::memcpy(rev, r.data(), K);
    std::memcpy(d, m.data(), sizeof(int32_t) * (size_t)K * K);
  }
  return 0;
}

int emu_denovo_overlap_ok(int32_t num_aligned, int32_t gs, int32_t seq_size, float match_fraction, int32_t match, int32_t mismatch) {
  return denovo_overlap_ok(num_aligned, gs, seq_size, match_fraction, match, mismatch) ? 1 : 0;
}

// dist: num x num; p: 3 per node slot (2 num + 1 of them); height, below_root: one per slot; order: up to num leaves;
// out: {root, maxh, leaves in order}
int emu_denovo_tree(const int32_t* dist, int32_t num, int32_t* p, int32_t* height, uint8_t* below_root, uint32_t* order, int32_t* out) {
  DenovoTree t;
  denovo_tree(dist, num, t);
  for (size_t i = 0; i < t.p.size(); ++i) {
    for (int k = 0; k < 3; ++k) p[3 * i + k] = t.p[i][k];
    height[i] = t.height[i];
    below_root[i] = t.below_root[i];
  }
  for (size_t i = 0; i < t.order.size(); ++i) order[i] = t.order[i];
  out[0] = t.root;
  out[1] = t.maxh;
  out[2] = (int32_t)t.order.size();
  return 0;
}

// the 's' ops of an op string of L bytes, as denovo_count_kernel counts them; lanes: what each of the 64 lanes returned
int emu_count_aligned(const uint8_t* ops, uint32_t L, uint32_t* lanes) {
  WaveShared sh;
  sh.run([&](uint32_t lane) {
    HostWave w{lane, &sh};
    lanes[lane] = msa_count_aligned_wave(w, ops, L);
  });
  return 0;
}
}
