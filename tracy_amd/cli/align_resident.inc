// align_resident.inc -- `align --batch --resident`: the trace files of a block of manifest lines go to the device once and the text of the four
// output files comes back once; every intermediate stays where the stage before left it (included by tracy_amd_cli.cpp, inside its namespace).
//
//   tracyhip_read_traces -> tracyhip_basecall_traces -> tracyhip_render_traces (TSV: <prefix>.abif)
//   -> tracyhip_align_traces (one call per reference kind: FASTA records / wildtype profiles, shared through ref_index)
//   -> FASTA lines: tracyhip_reference_slices -> tracyhip_alignment_rows        (wildtype lines: rows0 / rows1 of the align call)
//   -> tracyhip_pad_traces along row 0 -> tracyhip_render_traces (GAPPED) -> tracyhip_render_alignments (PLOT, FASTA, JSON)
//   -> one copy of the text to the host
//
// The layout of a block is align_resident_plan.h's.  Every text is sized by the sizes-only form of its call and rendered into a buffer of
// exactly those sizes (DESIGN.md section 5, "The resident chain of `align --batch`").  What the device does not answer -- an indexed genome, a reference that does not load, a
// file a stage defers, trims that take the whole trace -- takes the host path of the command (prepare -> align_*_group -> write_outputs)
// with its messages and its exit code; the chain itself prints nothing about a line.

struct ResidentBlock {
  resident::BlockPlan plan;
  bool usable = false;                  // the chain has something to read
  std::unique_ptr<uint8_t[]> bytes;     // the file images of the entries (released once they are on the device)
  std::vector<std::string> fasta_name, fasta_seq;  // the distinct FASTA records of the block
  std::vector<uint8_t> fasta_ok;        // loaded and at most 50 kb
  std::vector<uint8_t> eligible;        // [lines] the chain may answer the line (the rest was prepared by the host already)
  std::vector<uint32_t> text_len[resident::FRAG_COUNT];  // [rows]
  std::vector<std::string> json_head;   // [rows] the host's opening lines of the .json, through trailingGaps
  std::unique_ptr<uint8_t[]> text;      // the copy-back buffer: every file of every answered row is one span of it
};

// the second header line of the plot (plotAlignment, key 0) without its newline
std::string resident_plot_head1(std::string const& chr, uint32_t pos, uint32_t reflen, bool forward) {
  TextBuf t(256);
  t << ">Ref " << chr << ":" << ((uint64_t)pos + 1) << "-" << ((uint64_t)pos + reflen) << (forward ? " forward" : " reversecomplement");
  return t.str();
}

// host threads: classify the references, load the distinct FASTA records, read the trace files (and every distinct wildtype once) into one buffer
void resident_prep(std::vector<Job>& jobs, uint32_t lo, uint32_t hi, ResidentBlock& b, uint32_t nthreads) {
  const uint32_t m = hi - lo;
  std::vector<int32_t> kinds(m);
  std::vector<std::string> paths(m);
  for_each_index(m, nthreads, [&](uint32_t i) { kinds[i] = genomeType(jobs[lo + i].ref_path); });
  for (uint32_t i = 0; i < m; ++i) paths[i] = jobs[lo + i].ref_path;
  resident::BlockPlan& P = b.plan;
  P.split_references(kinds, paths);
  const uint32_t nf = P.nfasta(), ne = P.nentries();
  b.fasta_name.assign(nf, std::string());
  b.fasta_seq.assign(nf, std::string());
  b.fasta_ok.assign(nf, 0);
  for_each_index(nf, nthreads, [&](uint32_t f) {  // (quiet: a line whose reference is refused is reported by the host path)
    b.fasta_ok[f] = loadSingleFasta(paths[P.fasta_line[f]], b.fasta_name[f], b.fasta_seq[f], true) && b.fasta_seq[f].size() <= kMaxSingleFasta;
  });
  b.eligible.assign(m, 0);
  for (uint32_t i = 0; i < m; ++i)
    b.eligible[i] = P.kind[i] == resident::REF_WILDTYPE || (P.kind[i] == resident::REF_FASTA && b.fasta_ok[P.ref_of[i]]);
  std::vector<uint32_t> file_len(ne, 0), sample_cap(ne, 0), call_cap(ne, 0);
  auto path_of = [&](uint32_t e) -> std::string const& { return e < m ? jobs[lo + e].trace_path : paths[P.wildtype_line[e - m]]; };
  for_each_index(ne, nthreads, [&](uint32_t e) {
    if (e < m && !b.eligible[e]) return;
    struct stat st;
    if (::stat(path_of(e).c_str(), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && (uint64_t)st.st_size <= 0x7fffffffull) file_len[e] = (uint32_t)st.st_size;
    tracyhip_read_bound(file_len[e], &sample_cap[e], &call_cap[e]);
  });
  b.usable = P.layout_entries(file_len, sample_cap, call_cap) && P.file_off[ne] > 0;  // (totals that leave 64 bits: the whole block takes the host path)
  if (!b.usable) return;
  b.bytes.reset(new uint8_t[P.file_off[ne] + 16]);
  for_each_index(ne, nthreads, [&](uint32_t e) {
    if (!P.file_len[e]) return;
    std::FILE* f = std::fopen(path_of(e).c_str(), "rb");
    const std::size_t got = f ? std::fread(b.bytes.get() + P.file_off[e], 1, P.file_len[e], f) : 0;
    if (f) std::fclose(f);
    if (got != P.file_len[e]) std::memset(b.bytes.get() + P.file_off[e], 0, P.file_len[e]);  // (no magic: neither format, the reader defers it)
  });
}

// the chain for one block.  false: a device call failed (the command ends); true: plan.alive says which rows the device answered, and their
// text lies in b.text
bool resident_chain(tracyhip_ctx* ctx, SageConfig const& c, tracyhip_params const& prm, std::vector<Job>& jobs, uint32_t lo, ResidentBlock& b,
                    StageTimes& times) {
  using namespace resident;
  BlockPlan& P = b.plan;
  const uint32_t m = P.nlines, ne = P.nentries();
  Stopwatch sw;
  // the wall seconds of the chain by stage (TRACY_AMD_CLI_TIMERS): what went by since the last lap
  struct Laps {
    StageTimes& times;
    Stopwatch w;
    void lap(const char* what) { times.add(what, w.seconds()); w = Stopwatch(); }
  } laps{times, Stopwatch()};
  DeviceBuffers dev(ctx);
  uint8_t* d_bytes;
  if (!dev.get(P.file_off[ne], d_bytes) || tracyhip_device_copy(ctx, d_bytes, b.bytes.get(), P.file_off[ne], 1) != TRACYHIP_OK) return gpu_fail("upload");
  b.bytes.reset();
  laps.lap("resident_upload_s");

  // 1. file bytes -> chromatograms (int16, what ABIF stores) and call positions, capacities from the bound
  std::vector<uint32_t> nsamples(ne), ncalls(ne);
  std::vector<int32_t> rstatus(ne), format(ne);
  int16_t* d_signal;
  int32_t* d_pos;
  if (!dev.get(P.sample_off[ne], d_signal) || !dev.get(P.call_off[ne], d_pos)) return gpu_fail("device memory");
  tracyhip_read_job rj{};
  rj.ntraces = ne; rj.bytes = d_bytes; rj.file_offset = P.file_off.data(); rj.file_len = P.file_len.data(); rj.sample_bytes = 2;
  tracyhip_read_result rr{};
  rr.status = rstatus.data(); rr.format = format.data(); rr.nsamples = nsamples.data(); rr.ncalls = ncalls.data();
  rr.signal = d_signal; rr.sample_offset = P.sample_off.data(); rr.sample_cap = P.sample_cap.data();
  rr.basecallpos = d_pos; rr.call_offset = P.call_off.data(); rr.call_cap = P.call_cap.data();
  if (tracyhip_read_traces(ctx, &rj, TRACYHIP_MEM_DEVICE, &rr) != TRACYHIP_OK) return gpu_fail("read");

  // 2. chromatograms -> basecalls, qualities, trims and the full profiles, where they lie
  std::vector<int32_t> bstatus(ne);
  std::vector<uint32_t> bc_len(ne), btrim_l(ne), btrim_r(ne), best(ne);
  uint8_t *d_pri, *d_sec, *d_con, *d_q;
  int32_t* d_bcpos;
  float* d_prof;
  const uint64_t nc = P.call_off[ne];
  if (!dev.get(nc, d_pri) || !dev.get(nc, d_sec) || !dev.get(nc, d_con) || !dev.get(nc, d_q) || !dev.get(nc, d_bcpos) || !dev.get(6 * nc, d_prof))
    return gpu_fail("device memory");
  tracyhip_basecall_job bj{};
  bj.ntraces = ne; bj.signal = d_signal; bj.signal_offset = P.sample_off.data(); bj.nsamples = nsamples.data(); bj.sample_bytes = 2;
  bj.basecallpos = d_pos; bj.pos_offset = P.call_off.data(); bj.npos = ncalls.data();
  bj.sigratio = c.pratio; bj.trim_stringency = c.trimStringency >= 1 ? c.trimStringency : 0;
  tracyhip_basecall_result br{};
  br.status = bstatus.data(); br.bc_len = bc_len.data(); br.trim_left = btrim_l.data(); br.trim_right = btrim_r.data(); br.best_section = best.data();
  br.primary = d_pri; br.secondary = d_sec; br.consensus = d_con; br.bcpos = d_bcpos; br.estqual = d_q; br.profiles = d_prof;
  if (tracyhip_basecall_traces(ctx, &bj, TRACYHIP_MEM_DEVICE, &br) != TRACYHIP_OK) return gpu_fail("basecall");

  std::vector<uint8_t> entry_ok(ne);
  for (uint32_t e = 0; e < ne; ++e) entry_ok[e] = P.file_len[e] != 0 && rstatus[e] == TRACYHIP_READ_OK && bstatus[e] == TRACYHIP_BASECALL_OK;
  std::vector<uint32_t> ltrim_l(m), ltrim_r(m);
  for (uint32_t i = 0; i < m; ++i) {
    ltrim_l[i] = c.trimStringency >= 1 ? btrim_l[i] : c.trimLeft;
    ltrim_r[i] = c.trimStringency >= 1 ? btrim_r[i] : c.trimRight;
  }
  P.open_rows(entry_ok, bc_len, ltrim_l, ltrim_r, b.fasta_ok);
  const uint32_t nr = P.nrows();
  laps.lap("resident_read_basecall_s");
  if (nr == 0) return true;

  // the rows' views of the entry payloads
  std::vector<uint64_t> sig_off(nr), bc_off(nr), prof_off(nr);
  std::vector<uint32_t> ns(nr), bcl(nr), trim_l(nr), trim_r(nr);
  for (uint32_t k = 0; k < nr; ++k) {
    const uint32_t i = P.row_line[k];
    sig_off[k] = P.sample_off[i]; bc_off[k] = P.call_off[i]; prof_off[k] = P.profile_off(i);
    ns[k] = nsamples[i]; bcl[k] = bc_len[i]; trim_l[k] = ltrim_l[i]; trim_r[k] = ltrim_r[i];
  }
  std::vector<int32_t> tstatus(nr);
  std::vector<uint8_t> ok(nr);
  std::vector<uint32_t> (&tlen)[FRAG_COUNT] = b.text_len;
  for (auto& v : tlen) v.assign(nr, 0);
  auto verdicts = [&](int32_t good) {
    for (uint32_t k = 0; k < nr; ++k) ok[k] = tstatus[k] == good;
    P.keep(ok);
  };

  // 3. the .abif table: sizes now, the text with the others
  tracyhip_render_job tj{};
  tj.ntraces = nr; tj.form = TRACYHIP_RENDER_TSV;
  tj.signal = d_signal; tj.signal_offset = sig_off.data(); tj.nsamples = ns.data(); tj.sample_bytes = 2;
  tj.bcpos = d_bcpos; tj.primary = d_pri; tj.secondary = d_sec; tj.consensus = d_con; tj.estqual = d_q;
  tj.bc_offset = bc_off.data(); tj.bc_len = bcl.data();
  tj.trim_left_each = trim_l.data(); tj.trim_right_each = trim_r.data();
  tracyhip_render_result tr{};
  tr.status = tstatus.data(); tr.text_len = tlen[FRAG_ABIF].data();
  if (tracyhip_render_traces(ctx, &tj, TRACYHIP_MEM_DEVICE, &tr) != TRACYHIP_OK) return gpu_fail("render");
  verdicts(TRACYHIP_RENDER_OK);
  laps.lap("resident_text_sizes_s");

  // 4. the alignments: one call per reference kind, op strings and rows of row k at ops_off[k]
  std::vector<uint32_t> ref_cols(nr);
  for (uint32_t k = 0; k < nr; ++k) {
    const uint32_t i = P.row_line[k];
    ref_cols[k] = P.kind[i] == REF_FASTA ? (uint32_t)b.fasta_seq[P.ref_of[i]].size() : bc_len[P.wildtype_entry(P.ref_of[i])];
  }
  if (!P.layout_ops(bcl, ref_cols)) { std::cerr << "tracy_amd: the block's alignments leave 64 bits" << std::endl; return false; }
  uint8_t *d_ops, *d_rows0, *d_rows1;
  if (!dev.get(P.ops_off[nr], d_ops) || !dev.get(P.ops_off[nr], d_rows0) || !dev.get(P.ops_off[nr], d_rows1)) return gpu_fail("device memory");
  std::vector<uint8_t> forward(nr, 0);
  std::vector<int32_t> ref_pos(nr, 0), score(nr, 0);
  std::vector<uint32_t> ref_len(nr, 0), cols(nr, 0);
  uint32_t device_calls = 0;
  // the per-trace result arrays of an align call live on the device under TRACYHIP_MEM_DEVICE (ops_len is read there by
  // tracyhip_alignment_rows); seven words and a byte per trace come back for the host's metadata
  struct AlignOut {
    uint32_t* d_words = nullptr;
    uint8_t* d_fwd = nullptr;
    std::vector<uint32_t> words;
    std::vector<uint8_t> fwd;
    uint32_t n = 0;
    enum { SF, SR, SFIN, SB, SL, RP, OLEN, COUNT };
    uint32_t* dev(int w) const { return d_words + (size_t)w * n; }
    const uint32_t* host(int w) const { return words.data() + (size_t)w * n; }
  };
  auto bind = [&](AlignOut& o, uint32_t n, tracyhip_align_result& res) -> bool {
    o.n = n;
    if (!dev.get((uint64_t)AlignOut::COUNT * n, o.d_words) || !dev.get(n, o.d_fwd)) return false;
    res.score_fwd = reinterpret_cast<int32_t*>(o.dev(AlignOut::SF)); res.score_rev = reinterpret_cast<int32_t*>(o.dev(AlignOut::SR));
    res.score_final = reinterpret_cast<int32_t*>(o.dev(AlignOut::SFIN)); res.forward = o.d_fwd;
    res.slice_begin = o.dev(AlignOut::SB); res.slice_len = o.dev(AlignOut::SL); res.ref_pos = o.dev(AlignOut::RP); res.ops_len = o.dev(AlignOut::OLEN);
    res.ops = d_ops;
    return true;
  };
  auto fetch = [&](AlignOut& o) -> bool {
    o.words.assign((size_t)AlignOut::COUNT * o.n + 1, 0);
    o.fwd.assign((size_t)o.n + 1, 0);
    return tracyhip_device_copy(ctx, o.words.data(), o.d_words, 4ull * AlignOut::COUNT * o.n, 0) == TRACYHIP_OK &&
           tracyhip_device_copy(ctx, o.fwd.data(), o.d_fwd, o.n, 0) == TRACYHIP_OK;
  };
  for (int wildtype = 0; wildtype < 2; ++wildtype) {
    std::vector<uint32_t> const& rows = wildtype ? P.wildtype_rows : P.fasta_rows;
    const uint32_t n = (uint32_t)rows.size();
    if (n == 0) continue;
    std::vector<uint64_t> poff(n), ooff(n);
    std::vector<uint32_t> plen(n), tl(n), trr(n);
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t k = rows[j];
      poff[j] = prof_off[k]; plen[j] = bcl[k]; tl[j] = trim_l[k]; trr[j] = trim_r[k]; ooff[j] = P.ops_off[k];
    }
    tracyhip_align_job job{};
    job.ntraces = n;
    job.profiles = tracyhip_seqset{TRACYHIP_SEQ_PROFILE, d_prof, poff.data(), plen.data(), n};
    job.trim_left_each = tl.data();
    job.trim_right_each = trr.data();
    tracyhip_align_result res{};
    AlignOut o;
    if (!bind(o, n, res)) return gpu_fail("device memory");
    res.ops_offset = ooff.data();
    std::vector<uint64_t> roff;
    std::vector<uint32_t> rlen;
    uint8_t* d_refs = nullptr;
    if (wildtype) {
      // the forward profiles of the distinct wildtypes, basecalled with the block: entries behind the lines
      for (uint32_t w : P.wildtype_used) { roff.push_back(P.profile_off(P.wildtype_entry(w))); rlen.push_back(bc_len[P.wildtype_entry(w)]); }
      job.refs = tracyhip_seqset{TRACYHIP_SEQ_PROFILE, d_prof, roff.data(), rlen.data(), (uint32_t)rlen.size()};
      job.ref_index = P.wildtype_ref_index.data();
      res.rows0 = d_rows0; res.rows1 = d_rows1;
    } else {
      for (uint32_t f : P.fasta_used) rlen.push_back((uint32_t)b.fasta_seq[f].size());
      if (!P.layout_fasta(rlen)) { std::cerr << "tracy_amd: the block's references leave 64 bits" << std::endl; return false; }
      std::unique_ptr<uint8_t[]> refs(new uint8_t[P.fasta_off[rlen.size()] + 1]);
      for (std::size_t u = 0; u < rlen.size(); ++u) std::memcpy(refs.get() + P.fasta_off[u], b.fasta_seq[P.fasta_used[u]].data(), rlen[u]);
      if (!dev.get(P.fasta_off[rlen.size()], d_refs) || tracyhip_device_copy(ctx, d_refs, refs.get(), P.fasta_off[rlen.size()], 1) != TRACYHIP_OK)
        return gpu_fail("upload");
      job.refs = tracyhip_seqset{TRACYHIP_SEQ_CHAR, d_refs, P.fasta_off.data(), rlen.data(), (uint32_t)rlen.size()};
      job.ref_index = P.fasta_ref_index.data();
      job.strand_by_certificate = 1;  // (as the host path: only the decision is part of an output file)
    }
    if (tracyhip_align_traces(ctx, &job, &prm, TRACYHIP_MEM_DEVICE, &res) != TRACYHIP_OK) return gpu_fail("align");
    ++device_calls;
    if (!fetch(o)) return gpu_fail("copy back");
    if (!wildtype) {
      // the slices the final alignments ran against, then both rows from the op strings where they lie (ops_len read on the device)
      std::vector<uint32_t> sl(o.host(AlignOut::SL), o.host(AlignOut::SL) + n);
      if (!P.layout_slices(sl)) { std::cerr << "tracy_amd: the block's slices leave 64 bits" << std::endl; return false; }
      uint8_t* d_slices;
      if (!dev.get(P.slice_off[n], d_slices)) return gpu_fail("device memory");
      tracyhip_slices_job sj{};
      sj.n = n; sj.refs = job.refs; sj.ref_index = job.ref_index;
      sj.forward = o.fwd.data(); sj.slice_begin = o.host(AlignOut::SB); sj.slice_len = o.host(AlignOut::SL);
      if (tracyhip_reference_slices(ctx, &sj, TRACYHIP_MEM_DEVICE, d_slices, P.slice_off.data()) != TRACYHIP_OK) return gpu_fail("reference slices");
      tracyhip_pairs pr{};
      pr.npairs = n;
      pr.a1 = job.profiles;
      pr.a2 = tracyhip_seqset{TRACYHIP_SEQ_CHAR, d_slices, P.slice_off.data(), o.host(AlignOut::SL), n};
      if (tracyhip_alignment_rows(ctx, &pr, TRACYHIP_MEM_DEVICE, d_ops, ooff.data(), o.dev(AlignOut::OLEN), d_rows0, d_rows1) != TRACYHIP_OK)
        return gpu_fail("alignment rows");
    }
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t k = rows[j];
      forward[k] = o.fwd[j];
      ref_pos[k] = (int32_t)o.host(AlignOut::RP)[j];
      ref_len[k] = wildtype ? rlen[P.wildtype_ref_index[j]] : o.host(AlignOut::SL)[j];  // (wildtype: the length of its primary basecalls)
      score[k] = (int32_t)o.host(AlignOut::SFIN)[j];
      cols[k] = o.host(AlignOut::OLEN)[j];
    }
  }
  times.add("device_calls", (double)device_calls);
  laps.lap("resident_align_s");

  // 5. the trace padded along row 0 (no hard trim, no reverse: the trace as read): sizes, then the payloads
  std::vector<uint32_t> ns_out(nr), nc_out(nr), step(nr), leading(nr), trailing(nr);
  tracyhip_pad_job pj{};
  pj.ntraces = nr; pj.signal = d_signal; pj.signal_offset = sig_off.data(); pj.nsamples = ns.data(); pj.sample_bytes = 2;
  pj.bcpos = d_bcpos; pj.primary = d_pri; pj.secondary = d_sec; pj.consensus = d_con; pj.estqual = d_q;
  pj.bc_offset = bc_off.data(); pj.bc_len = bcl.data();
  pj.rows = d_rows0; pj.row_offset = P.ops_off.data(); pj.row_len = cols.data();
  tracyhip_pad_result po{};
  po.status = tstatus.data(); po.nsamples_out = ns_out.data(); po.ncalls_out = nc_out.data();
  po.leading_gaps = leading.data(); po.trailing_gaps = trailing.data(); po.step = step.data();
  if (tracyhip_pad_traces(ctx, &pj, TRACYHIP_MEM_DEVICE, &po) != TRACYHIP_OK) return gpu_fail("pad");
  verdicts(TRACYHIP_PAD_OK);
  if (!P.layout_pad(ns_out, nc_out)) { std::cerr << "tracy_amd: the block's padded traces leave 64 bits" << std::endl; return false; }
  int16_t* d_psignal;
  int32_t* d_pbcpos;
  uint8_t *d_ppri, *d_psec, *d_pq;
  if (!dev.get(P.pad_sample_off[nr], d_psignal) || !dev.get(P.pad_call_off[nr], d_pbcpos) || !dev.get(P.pad_call_off[nr], d_ppri) ||
      !dev.get(P.pad_call_off[nr], d_psec) || !dev.get(P.pad_call_off[nr], d_pq))
    return gpu_fail("device memory");
  po.signal = d_psignal; po.sample_offset = P.pad_sample_off.data(); po.sample_cap = P.pad_sample_cap.data();
  po.bcpos = d_pbcpos; po.primary = d_ppri; po.secondary = d_psec; po.estqual = d_pq;
  po.call_offset = P.pad_call_off.data(); po.call_cap = P.pad_call_cap.data();
  if (tracyhip_pad_traces(ctx, &pj, TRACYHIP_MEM_DEVICE, &po) != TRACYHIP_OK) return gpu_fail("pad");
  verdicts(TRACYHIP_PAD_OK);
  laps.lap("resident_pad_s");

  // 6. the gapped trace of the .json: the pad result as it stands (a row that is no longer answered has no padded trace: no sizes either)
  std::vector<uint32_t> gns(nr), gbl(nr);
  for (uint32_t k = 0; k < nr; ++k) { gns[k] = P.alive[k] ? ns_out[k] : 0; gbl[k] = P.alive[k] ? nc_out[k] : 0; }
  tracyhip_render_job gj{};
  gj.ntraces = nr; gj.form = TRACYHIP_RENDER_GAPPED;
  gj.signal = d_psignal; gj.signal_offset = P.pad_sample_off.data(); gj.nsamples = gns.data(); gj.sample_bytes = 2;
  gj.bcpos = d_pbcpos; gj.primary = d_ppri; gj.secondary = d_psec; gj.estqual = d_pq;
  gj.bc_offset = P.pad_call_off.data(); gj.bc_len = gbl.data();
  tracyhip_render_result gr{};
  gr.status = tstatus.data(); gr.text_len = tlen[FRAG_GAPPED].data();
  if (tracyhip_render_traces(ctx, &gj, TRACYHIP_MEM_DEVICE, &gr) != TRACYHIP_OK) return gpu_fail("render");
  verdicts(TRACYHIP_RENDER_OK);

  // 7. the names of the three alignment texts: the plot's first header line once, then stem, second header line and rs.chr of every row
  static const std::string head0 = ">Alt", wt_chr = "wildtype";
  std::vector<std::string> stems(nr), head1(nr);
  std::vector<std::string const*> chr(nr);
  std::vector<uint32_t> stem_len(nr), head1_len(nr), chr_len(nr);
  for (uint32_t k = 0; k < nr; ++k) {
    const uint32_t i = P.row_line[k];
    chr[k] = P.kind[i] == REF_FASTA ? &b.fasta_name[P.ref_of[i]] : &wt_chr;
    stems[k] = stem(jobs[lo + i].trace_path);
    head1[k] = resident_plot_head1(*chr[k], (uint32_t)ref_pos[k], ref_len[k], forward[k] != 0);
    stem_len[k] = (uint32_t)stems[k].size(); head1_len[k] = (uint32_t)head1[k].size(); chr_len[k] = (uint32_t)chr[k]->size();
  }
  if (!P.layout_names((uint32_t)head0.size(), stem_len, head1_len, chr_len)) { std::cerr << "tracy_amd: the block's names leave 64 bits" << std::endl; return false; }
  std::unique_ptr<uint8_t[]> names(new uint8_t[P.names_bytes + 1]);
  std::memcpy(names.get(), head0.data(), head0.size());
  for (uint32_t k = 0; k < nr; ++k) {
    std::memcpy(names.get() + P.stem_off[k], stems[k].data(), stem_len[k]);
    std::memcpy(names.get() + P.head1_off[k], head1[k].data(), head1_len[k]);
    std::memcpy(names.get() + P.chr_off[k], chr[k]->data(), chr_len[k]);
  }
  uint8_t* d_names;
  if (!dev.get(P.names_bytes, d_names) || tracyhip_device_copy(ctx, d_names, names.get(), P.names_bytes, 1) != TRACYHIP_OK) return gpu_fail("upload");
  const std::vector<uint64_t> head0_off(nr, 0);
  const std::vector<uint32_t> head0_len(nr, (uint32_t)head0.size());
  tracyhip_alntext_job aj[3];
  tracyhip_alntext_result ar[3];
  static const uint32_t aform[3] = {TRACYHIP_ALNTEXT_PLOT, TRACYHIP_ALNTEXT_FASTA, TRACYHIP_ALNTEXT_JSON};
  static const uint32_t afrag[3] = {FRAG_PLOT, FRAG_FASTA, FRAG_TAIL};
  for (int f = 0; f < 3; ++f) {
    tracyhip_alntext_job& j = aj[f];
    j = tracyhip_alntext_job{};
    j.n = nr; j.form = aform[f]; j.key = 0; j.linelimit = c.linelimit;
    j.rows0 = d_rows0; j.rows1 = d_rows1; j.rows_offset = P.ops_off.data(); j.cols = cols.data();
    j.names = d_names;
    j.name0_offset = f == 0 ? head0_off.data() : P.stem_off.data();
    j.name0_len = f == 0 ? head0_len.data() : stem_len.data();
    j.name1_offset = f == 0 ? P.head1_off.data() : P.chr_off.data();
    j.name1_len = f == 0 ? head1_len.data() : chr_len.data();
    j.ref_pos = ref_pos.data(); j.ref_len = ref_len.data(); j.forward = forward.data(); j.score = score.data();
    ar[f] = tracyhip_alntext_result{};
    ar[f].status = tstatus.data(); ar[f].text_len = tlen[afrag[f]].data();
    if (tracyhip_render_alignments(ctx, &j, TRACYHIP_MEM_DEVICE, &ar[f]) != TRACYHIP_OK) return gpu_fail("render alignments");
    verdicts(TRACYHIP_ALNTEXT_OK);
  }

  // 8. every text into one buffer of exactly the sizes, the fragments of a row in file order; the host's two parts of the .json get their
  // room between the device's (they are filled in after the copy back)
  b.json_head.assign(nr, std::string());
  for (uint32_t k = 0; k < nr; ++k) {
    TextBuf t(256);
    t << "{" << std::endl << "\"gappedTrace\":" << std::endl << "{" << std::endl << "\"traceFileName\": \"trace\"," << std::endl;
    t << "\"leadingGaps\": " << leading[k] << "," << std::endl << "\"trailingGaps\": " << trailing[k] << "," << std::endl;
    b.json_head[k] = t.str();
    tlen[FRAG_JSON_HEAD][k] = (uint32_t)b.json_head[k].size();
    tlen[FRAG_JSON_CLOSE][k] = 2;  // "}\n"
  }
  laps.lap("resident_text_sizes_s");
  if (!P.layout_text(tlen)) { std::cerr << "tracy_amd: the block's text leaves 64 bits" << std::endl; return false; }
  uint8_t* d_text;
  if (!dev.get(P.text_bytes, d_text)) return gpu_fail("device memory");
  std::vector<uint32_t> again(nr);  // (the sizes were reported by the first pass; a row without capacity reports TOO_SMALL here)
  auto emit = [&](tracyhip_render_result& r, Fragment f) {
    r.text = d_text; r.text_offset = P.text_off[f].data(); r.text_cap = P.text_cap[f].data(); r.text_len = again.data();
  };
  emit(tr, FRAG_ABIF);
  if (tracyhip_render_traces(ctx, &tj, TRACYHIP_MEM_DEVICE, &tr) != TRACYHIP_OK) return gpu_fail("render");
  verdicts(TRACYHIP_RENDER_OK);
  emit(gr, FRAG_GAPPED);
  if (tracyhip_render_traces(ctx, &gj, TRACYHIP_MEM_DEVICE, &gr) != TRACYHIP_OK) return gpu_fail("render");
  verdicts(TRACYHIP_RENDER_OK);
  for (int f = 0; f < 3; ++f) {
    emit(ar[f], (Fragment)afrag[f]);
    if (tracyhip_render_alignments(ctx, &aj[f], TRACYHIP_MEM_DEVICE, &ar[f]) != TRACYHIP_OK) return gpu_fail("render alignments");
    verdicts(TRACYHIP_ALNTEXT_OK);
  }
  laps.lap("resident_text_emit_s");

  // 9. one copy back
  b.text.reset(new uint8_t[P.text_bytes + 1]);
  if (P.text_bytes && tracyhip_device_copy(ctx, b.text.get(), d_text, P.text_bytes, 0) != TRACYHIP_OK) return gpu_fail("copy back");
  laps.lap("resident_copy_back_s");
  times.add("resident_chain_s", sw.seconds());  // (the whole chain but the release of its device buffers)
  return true;
}

// the four files of an answered row, byte for byte what prepare() and write_outputs() write: each is one span of the copy-back buffer,
// once the host's two parts of the .json are in their places
void resident_write(std::string const& prefix, ResidentBlock& b, uint32_t k) {
  using namespace resident;
  BlockPlan const& P = b.plan;
  char* const text = reinterpret_cast<char*>(b.text.get());
  std::memcpy(text + P.text_off[FRAG_JSON_HEAD][k], b.json_head[k].data(), b.json_head[k].size());
  std::memcpy(text + P.text_off[FRAG_JSON_CLOSE][k], "}\n", 2);
  static const char* ext[FILE_COUNT] = {".abif", ".align.fa", ".txt", ".json"};
  for (uint32_t f = 0; f < FILE_COUNT; ++f) TextBuf::write_bytes(prefix + ext[f], text + P.out_off(f, k), (std::size_t)P.out_len(f, k));
}

// `align --batch --resident` behind the checks of align_main: the block loop of the host path with the chain as its device stage
int align_resident_main(SageConfig const& c, std::vector<Job>& jobs, int argc, char** argv) {
  echo_command(argc, argv);
  std::cout << stamp() << "Load ab1 file" << std::endl;
  // one device: sharding the chain over a device group is not built
  std::string first = c.devices == "all" ? std::string("0") : c.devices.substr(0, c.devices.find(','));
  if (first != c.devices) std::cout << stamp() << "--resident runs on one GPU: device " << first << " of -d " << c.devices << std::endl;
  std::atomic<int> failed(0);
  const uint32_t nthreads = c.threads ? c.threads : usable_cores();
  const uint32_t njobs = (uint32_t)jobs.size();
  StageTimes times;
  const char* blk_env = getenv("TRACY_AMD_CLI_BLOCK");
  const uint32_t blk = (blk_env && std::atol(blk_env) >= 1) ? block_size() : resident::kBlockLines;
  std::vector<ResidentBlock> blocks((njobs + blk - 1) / blk + 1);
  std::vector<int> rcs(njobs, 0);
  // the host path's prepare for the lines the chain does not answer, with its messages
  std::mutex host_mutex;  // (the stage that reads block k + 1 and the device stage of block k both come here: their messages stay whole lines)
  auto host_prepare = [&](std::vector<uint32_t> const& lines) {
    std::lock_guard<std::mutex> lk(host_mutex);
    Stopwatch sw;
    for_each_index((uint32_t)lines.size(), lines.size() <= 64 ? 1 : nthreads, [&](uint32_t x) { rcs[lines[x]] = prepare(c, jobs[lines[x]]); });
    for (uint32_t i : lines) {
      if (rcs[i] != 0) {
        std::cerr << "skipping " << jobs[i].trace_path << std::endl;
        ++failed;
      } else {
        jobs[i].ok = true;
      }
    }
    times.add("read_basecall_profile_s", sw.seconds());
  };
  auto prep = [&](uint32_t lo, uint32_t hi) {
    Stopwatch sw;
    ResidentBlock& b = blocks[lo / blk];
    resident_prep(jobs, lo, hi, b, nthreads);
    times.add("resident_read_files_s", sw.seconds());
    std::vector<uint32_t> host_lines;
    for (uint32_t i = lo; i < hi; ++i)
      if (!b.usable || !b.eligible[i - lo]) host_lines.push_back(i);
    if (!host_lines.empty()) host_prepare(host_lines);
  };
  Device dev;
  bool dev_open = false, said = false;
  std::future<int> dev_ready = std::async(std::launch::async, [&]() {
    Stopwatch sw;
    const int rc = dev.open(first, 2);
    times.add("gpu_init_s", sw.seconds());
    return rc;
  });
  tracyhip_params prm{c.match, c.mismatch, c.gapopen, c.gapext, 1, 0};
  std::vector<uint8_t> answered(njobs, 0);
  uint32_t resident_traces = 0;
  auto device = [&](uint32_t lo, uint32_t hi) -> bool {
    if (!said) std::cout << stamp() << "Find reference match" << std::endl;
    if (!dev_open) {
      if (dev_ready.get() != 0) return gpu_fail("no usable GPU");
      dev_open = true;
    }
    Stopwatch sw;
    if (!said) std::cout << stamp() << "Alignment" << std::endl;
    said = true;
    ResidentBlock& b = blocks[lo / blk];
    if (b.usable) {
      if (!resident_chain(dev.ctx, c, prm, jobs, lo, b, times)) return false;
      for (uint32_t k = 0; k < b.plan.nrows(); ++k)
        if (b.plan.alive[k]) { answered[lo + b.plan.row_line[k]] = 1; ++resident_traces; }
      // what the chain left, on the host path
      std::vector<uint32_t> late;
      for (uint32_t i = lo; i < hi; ++i)
        if (b.eligible[i - lo] && !answered[i]) late.push_back(i);
      if (!late.empty()) host_prepare(late);
    }
    std::vector<Job*> fasta_group, seeded_group, wildtype;
    for (uint32_t i = lo; i < hi; ++i) {
      Job& j = jobs[i];
      if (!j.ok) continue;
      if (j.rs.filetype == 1) fasta_group.push_back(&j);
      else if (j.rs.filetype == 0) seeded_group.push_back(&j);
      else wildtype.push_back(&j);
    }
    uint32_t device_calls = 0;
    for (auto* g : {&fasta_group, &seeded_group}) {
      if (g->empty()) continue;
      if (!align_fasta_group(dev, prm, *g, nthreads)) return false;
      ++device_calls;
    }
    times.add("device_calls", (double)device_calls);
    if (!wildtype.empty() && !align_wildtype_group(dev, prm, wildtype)) return false;
    times.add("device_s", sw.seconds());
    return true;
  };
  bool said_out = false;
  auto write = [&](uint32_t lo, uint32_t hi) {
    Stopwatch sw;
    if (!said_out) std::cout << stamp() << "Output" << std::endl;
    said_out = true;
    ResidentBlock& b = blocks[lo / blk];
    for_each_index(hi - lo, nthreads, [&](uint32_t i) {
      Job& j = jobs[lo + i];
      if (answered[lo + i]) resident_write(j.outprefix, b, b.plan.row_of_line[i]);
      else if (j.ok) write_outputs(c, j);
      Job done; done.trace_path.swap(j.trace_path); done.ok = j.ok; j = std::move(done);  // the block's traces are released here
    });
    b = ResidentBlock();  // ... and its text
    times.add("writers_s", sw.seconds());
  };
  if (!run_blocks(njobs, blk, prep, device, write)) return -1;
  times.add("resident_traces", (double)resident_traces);
  times.report(njobs, nthreads);
  std::cout << stamp() << "Device: " << resident_traces << " of " << njobs << " traces read, basecalled, aligned and written" << std::endl;
  std::cout << stamp() << "Done." << std::endl;
  end_process((failed || TextBuf::write_errors()) ? 2 : 0);
}
