// assemble_cli.inc -- `tracy assemble` (assemble.h:56-589) on the C ABI; included by tracy_amd_cli.cpp inside its
// anonymous namespace (uses stamp(), stem(), regular_nonempty(), load_trace(), Device, gpu_fail()).
//
//   tracy_amd_cli assemble [options] [-r reference.fa] trace1.ab1 trace2.ab1 ...
//   tracy_amd_cli assemble [options] -r reference.fa --batch manifest.tsv
//   tracy_amd_cli assemble [options] --denovo --batch manifest.tsv
//
// Reference-guided: every trace is scored in both strands against the reference (one device batch), the matching
// traces join the alignment one by one, best first (each step one profile x profile Gotoh on the device).
// De novo: strand assignment (revSeqBasedOnDist), removal of traces that overlap nothing, msa() (distance matrix,
// UPGMA, progressive alignment -- msa.hpp), consensus.  Outputs: .align.fa, .json, .vertical, .cons.fa|.cons.fq.

struct AssembleConfig {  // assemble.h:12-30
  bool hasReference = false, incCons = false, incRef = false;
  int32_t gapopen = -10, gapext = -4, match = 3, mismatch = -5;
  float pratio = 0.33f, trimStringency = 4, matchFraction = 0.5f, fractionCalled = 0.1f;
  std::string outprefix = "out", format = "fasta", reference;
  std::vector<std::string> ab;
  int device = 0;
  std::string batch;     // --batch: manifest of trace <TAB> reference <TAB> outprefix lines
  bool denovo = false;   // --denovo: the groups of the manifest are assembled de novo (no reference anywhere)
  uint32_t threads = 0;  // --threads: host threads of the --batch stages; 0 = every core this process may use
};

struct TraceScore {  // assemble.h:32-41
  int32_t score, idx, newidx;
  bool forward;
  bool operator<(TraceScore const& o) const { return score > o.score || (score == o.score && idx < o.idx); }
};

int parse_assemble(int argc, char** argv, AssembleConfig& c) {
  static const std::map<std::string, char> longs = {{"help", '?'}, {"reference", 'r'}, {"pratio", 'p'}, {"trim", 't'}, {"fracmatch", 'f'},
                                                    {"gapopen", 'g'}, {"gapext", 'e'}, {"match", 'm'}, {"mismatch", 'n'}, {"called", 'd'},
                                                    {"outprefix", 'o'}, {"format", 'a'}, {"inccons", 'i'}, {"incref", 'j'}, {"device", 'D'},
                                                    {"batch", 'B'}, {"threads", 'T'}, {"denovo", 'N'}};
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i], val;
    char opt = 0;
    bool has_val = false;
    if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
      std::string name = a.substr(2);
      const std::size_t eq = name.find('=');
      if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
      auto it = longs.find(name);
      if (it == longs.end()) { std::cerr << "unrecognised option '" << a << "'" << std::endl; return 1; }
      opt = it->second;
    } else if (a.size() >= 2 && a[0] == '-' && !(a[1] >= '0' && a[1] <= '9')) {
      opt = a[1];
      if (a.size() > 2) { val = a.substr(2); has_val = true; }
    } else {
      c.ab.push_back(a);
      continue;
    }
    if (opt == '?') return 1;
    if (opt == 'i') { c.incCons = true; continue; }
    if (opt == 'j') { c.incRef = true; continue; }
    if (opt == 'N' && a == "--denovo") { c.denovo = true; continue; }
    if (!has_val) {
      if (i + 1 >= argc) { std::cerr << "the required argument for option '" << a << "' is missing" << std::endl; return 1; }
      val = argv[++i];
    }
    switch (opt) {
      case 'r': c.reference = val; c.hasReference = true; break;
      case 'p': c.pratio = std::strtof(val.c_str(), nullptr); break;
      case 't': c.trimStringency = std::strtof(val.c_str(), nullptr); break;
      case 'f': c.matchFraction = std::strtof(val.c_str(), nullptr); break;
      case 'g': c.gapopen = std::atoi(val.c_str()); break;
      case 'e': c.gapext = std::atoi(val.c_str()); break;
      case 'm': c.match = std::atoi(val.c_str()); break;
      case 'n': c.mismatch = std::atoi(val.c_str()); break;
      case 'd': c.fractionCalled = std::strtof(val.c_str(), nullptr); break;
      case 'o': c.outprefix = val; break;
      case 'a': c.format = val; break;
      case 'D': c.device = std::atoi(val.c_str()); break;
      case 'B': c.batch = val; break;
      case 'T': c.threads = (uint32_t)std::max(0, std::atoi(val.c_str())); break;
      default: std::cerr << "unrecognised option '" << a << "'" << std::endl; return 1;
    }
  }
  return (c.ab.empty() == c.batch.empty()) ? 1 : 0;  // trace files, or a manifest
}

struct AsmTrace {  // one input trace: what the alignment stage and the output stage need
  Trace tr;
  BaseCalls bc;
  uint32_t trimLeft = 0, trimRight = 0;
  Profile prof;  // createProfile(tr, bc, trimLeft, trimRight)
};

// load + basecall + trimming estimate + profile (assemble.h:184-214 / 384-417); returns the CLI exit code
int load_asm_trace(AssembleConfig const& c, std::string const& path, AsmTrace& t) {
  if (!load_trace(path, t.tr)) return -1;
  basecall(t.tr, t.bc, c.pratio);
  if (t.bc.bcPos.empty()) {
    std::cerr << "Trace file lacks basecalls!" << std::endl;
    return -1;
  }
  if (c.trimStringency) {
    trimTrace(c.trimStringency, t.bc, t.trimLeft, t.trimRight);
    if (t.trimLeft + t.trimRight >= t.bc.bcPos.size()) {
      std::cerr << "Too stringent trimming parameters!" << std::endl;
      std::cerr << path << " has no peaks left!" << std::endl;
      return -1;
    }
  }
  createProfile(t.tr, t.bc, t.prof, (int32_t)t.trimLeft, (int32_t)t.trimRight);
  return 0;
}

// gotoh(a1[k], a2[k]) for all k in one device call: scores and op strings (push order)
bool align_profiles(tracyhip_ctx* ctx, tracyhip_params const& prm, std::vector<Profile const*> const& a1, std::vector<Profile const*> const& a2,
                    std::vector<int32_t>& scores, std::vector<std::string>& ops_out) {
  const uint32_t np = (uint32_t)a1.size();
  scores.assign(np, 0);
  ops_out.assign(np, std::string());
  if (np == 0) return true;
  detail::ProfilePack p1, p2;
  std::vector<uint64_t> ooff(np);
  uint64_t cap = 0;
  for (uint32_t i = 0; i < np; ++i) {
    p1.add(*a1[i]);
    p2.add(*a2[i]);
    ooff[i] = cap;
    cap += a1[i]->cols + a2[i]->cols;
  }
  tracyhip_pairs pr{};
  pr.npairs = np;
  pr.a1 = p1.set();
  pr.a2 = p2.set();
  std::vector<uint8_t> ops(cap ? cap : 1);
  std::vector<uint32_t> olen(np);
  if (tracyhip_gotoh_align(ctx, &pr, &prm, TRACYHIP_MEM_HOST, scores.data(), ops.data(), ooff.data(), olen.data()) != TRACYHIP_OK)
    return gpu_fail("alignment");
  for (uint32_t i = 0; i < np; ++i) {
    ops_out[i].assign(reinterpret_cast<char*>(ops.data()) + ooff[i], olen[i]);
    std::reverse(ops_out[i].begin(), ops_out[i].end());  // forward order
  }
  return true;
}

// the gapped consensus-character row of a profile along an op string (forward order); row 0 takes 'h' as gap
std::string profile_row(Profile const& p, std::string const& ops, bool first_row) {
  std::string row;
  std::size_t at = 0;
  for (char op : ops) {
    const bool gap = first_row ? op == 'h' : op == 'v';
    row.push_back(gap ? '-' : profileConsChar(p, at));
    if (!gap) ++at;
  }
  return row;
}

void write_assembly_outputs(AssembleConfig const& c, CharAlign const& align, std::string const& gapped, std::string const& cs,
                            std::string const& qstr) {
  {
    std::ofstream v((c.outprefix + ".vertical").c_str());
    const std::size_t ncol = align.empty() ? 0 : align[0].size();
    for (std::size_t j = 0; j < ncol; ++j) {
      for (auto const& r : align) v << r[j];
      v << '|' << gapped[j] << std::endl;
    }
  }
  if (c.format == "fasta") {
    std::ofstream f((c.outprefix + ".cons.fa").c_str());
    f << ">Consensus" << std::endl << cs << std::endl;
  } else if (c.format == "fastq") {
    std::ofstream f((c.outprefix + ".cons.fq").c_str());
    f << "@Consensus" << std::endl << cs << std::endl << "+" << std::endl << qstr << std::endl;
  }
}

// the gapped chromatogram of alignment row `row` (assemble.h:330-372 / 506-545)
void gapped_trace_json(std::ostream& out, AsmTrace const& t, bool forward, std::string const& row, std::string const& name) {
  BaseCalls nbc;
  trimTrace(t.tr, t.bc, t.trimLeft, t.trimRight, nbc);
  PaddedTrace padded;
  if (forward) {
    alignmentTracePadding(row, t.tr, nbc, padded);
  } else {
    Trace ttr;
    BaseCalls tbc;
    reverseComplementTrace(t.tr, nbc, ttr, tbc);
    alignmentTracePadding(row, ttr, tbc, padded);
  }
  assemblyTrace(out, padded, name);
}

// .align.fa and .json of a reference-guided assembly (assemble.h:290-372); scoreIdx in TraceScore order, the trace of rank i is row n - 1 - i
void write_ref_guided_outputs(AssembleConfig const& c, std::vector<AsmTrace> const& traces, std::vector<TraceScore> const& scoreIdx,
                              CharAlign const& align, std::string const& gapped, std::string const& cs) {
  const std::size_t n = scoreIdx.size();
  {
    std::ofstream v((c.outprefix + ".align.fa").c_str());
    for (std::size_t i = 0; i < n; ++i) {
      v << ">" << stem(c.ab[scoreIdx[i].idx]) << (scoreIdx[i].forward ? " (forward)" : " (reverse)") << std::endl;
      v << align[n - i - 1] << std::endl;
    }
    v << ">Reference" << std::endl << align[n] << std::endl;
    if (c.incCons) v << ">Consensus" << std::endl << gapped << std::endl;
  }
  std::ofstream r((c.outprefix + ".json").c_str());
  r << "{" << std::endl;
  r << "\"gapFreeConsensus\": \"" << cs << "\"," << std::endl;
  r << "\"gappedConsensus\": \"" << gapped << "\"," << std::endl;
  r << "\"msa\": " << std::endl << "[" << std::endl;
  for (std::size_t i = 0; i < n; ++i) {
    if (i) r << ',' << std::endl;
    alignedTraceByRow(r, align, (uint32_t)(n - i - 1), stem(c.ab[scoreIdx[i].idx]), scoreIdx[i].forward, false);
  }
  r << ',' << std::endl;
  alignedTraceByRow(r, align, (uint32_t)n, "", true, true);
  r << "]," << std::endl;
  r << "\"gappedTraces\": " << std::endl << "[" << std::endl;
  for (std::size_t i = 0; i < n; ++i) {
    if (i) r << ", ";
    gapped_trace_json(r, traces[scoreIdx[i].idx], scoreIdx[i].forward, align[n - i - 1], stem(c.ab[scoreIdx[i].idx]));
  }
  r << "]" << std::endl << "}" << std::endl;
}

// .align.fa and .json of a de novo assembly (assemble.h:473-545): row i of the alignment is trace idxMap[seqidx[i]] of the input
void write_denovo_outputs(AssembleConfig const& c, std::vector<AsmTrace> const& traces, std::vector<uint32_t> const& idxMap, std::vector<bool> const& fwd,
                          std::vector<uint32_t> const& seqidx, CharAlign const& align, std::string const& gapped, std::string const& cs) {
  {
    std::ofstream v((c.outprefix + ".align.fa").c_str());
    for (std::size_t i = 0; i < align.size(); ++i) {
      v << ">" << stem(c.ab[idxMap[seqidx[i]]]) << (fwd[seqidx[i]] ? " (forward)" : " (reverse)") << std::endl;
      v << align[i] << std::endl;
    }
    if (c.incCons) v << ">Consensus" << std::endl << gapped << std::endl;
  }
  std::ofstream r((c.outprefix + ".json").c_str());
  r << "{" << std::endl;
  r << "\"gapFreeConsensus\": \"" << cs << "\"," << std::endl;
  r << "\"gappedConsensus\": \"" << gapped << "\"," << std::endl;
  r << "\"msa\": " << std::endl << "[" << std::endl;
  for (std::size_t i = 0; i < align.size(); ++i) {
    if (i) r << ',' << std::endl;
    alignedTraceByRow(r, align, (uint32_t)i, stem(c.ab[idxMap[seqidx[i]]]), fwd[seqidx[i]], false);
  }
  r << "]," << std::endl;
  r << "\"gappedTraces\": " << std::endl << "[" << std::endl;
  for (std::size_t i = 0; i < align.size(); ++i) {
    if (i) r << ", ";
    gapped_trace_json(r, traces[idxMap[seqidx[i]]], fwd[seqidx[i]], align[i], stem(c.ab[idxMap[seqidx[i]]]));
  }
  r << "]" << std::endl << "}" << std::endl;
}

// ---- --batch: many assemblies, every chain (-r) or tree (--denovo) on the device in one call per block ---------------------------------
struct AsmGroup {  // the manifest lines of one outprefix, in manifest order
  AssembleConfig c;  // the command's options with this group's outprefix and trace files
  uint32_t ref = 0;  // index into the loaded references
  std::vector<AsmTrace> traces;
  bool ok = false;
  std::vector<TraceScore> scoreIdx;
  std::vector<uint32_t> excluded;  // input indices of the traces that do not match
  std::vector<uint32_t> idxMap, seqidx;  // --denovo: the traces that stay, and which of them each row of the alignment is
  std::vector<bool> fwd;                 // ... their strands, indexed like idxMap
  CharAlign align;
  std::string gapped, cs, qstr;
};

// What both device calls take and give per group: the traces of `gs` in one pack with group_first, and the per-group result arrays
// with every group's offset.  bound(group, summed columns of its traces): the columns tracy_hip.h asks for it, over K + more_rows rows.
struct GroupPack {
  detail::ProfilePack tp;
  std::vector<uint32_t> first, nrows, ncol, clen;
  std::vector<uint64_t> roff, coff;
  std::vector<uint8_t> rows, gapped, cons, qual;
  template <class Bound>
  GroupPack(std::vector<AsmGroup*> const& gs, uint64_t more_rows, Bound bound) : first(1, 0), nrows(gs.size()), ncol(gs.size()), clen(gs.size()) {
    uint64_t rtot = 0, ctot = 0;
    for (AsmGroup const* a : gs) {
      uint64_t sum = 0;
      for (AsmTrace const& t : a->traces) { tp.add(t.prof); sum += t.prof.cols; }
      first.push_back((uint32_t)tp.off.size());
      roff.push_back(rtot);
      coff.push_back(ctot);
      rtot += (a->traces.size() + more_rows) * bound(*a, sum);
      ctot += bound(*a, sum);
    }
    rows.resize(std::max<uint64_t>(rtot, 1));
    gapped = cons = qual = std::vector<uint8_t>(std::max<uint64_t>(ctot, 1));
  }
  // align / gapped / cs / qstr of every group from the arrays; the profiles of its traces are released
  void unpack(std::vector<AsmGroup*> const& gs) const {
    for (std::size_t g = 0; g < gs.size(); ++g) {
      AsmGroup& a = *gs[g];
      a.align.assign(nrows[g], std::string());
      for (uint32_t r = 0; r < nrows[g]; ++r)
        a.align[r].assign(reinterpret_cast<const char*>(rows.data() + roff[g] + (uint64_t)r * ncol[g]), ncol[g]);
      if (nrows[g]) {
        a.gapped.assign(reinterpret_cast<const char*>(gapped.data() + coff[g]), ncol[g]);
        a.cs.assign(reinterpret_cast<const char*>(cons.data() + coff[g]), clen[g]);
        a.qstr.assign(reinterpret_cast<const char*>(qual.data() + coff[g]), clen[g]);
      }
      for (AsmTrace& t : a.traces) t.prof = Profile();
    }
  }
};

// all chains of `gs` (every one loaded) through one device call; fills scoreIdx / excluded / align / gapped / cs / qstr
bool assemble_device(tracyhip_ctx* ctx, AssembleConfig const& c, detail::ProfilePack& refs, std::vector<AsmGroup*> const& gs) {
  const uint32_t ng = (uint32_t)gs.size();
  if (ng == 0) return true;
  GroupPack p(gs, 1, [&](AsmGroup const& a, uint64_t sum) { return (uint64_t)refs.len[a.ref] + sum; });  // (K + 1) x (n_ref + sum len)
  std::vector<uint32_t> ridx(ng);
  for (uint32_t g = 0; g < ng; ++g) ridx[g] = gs[g]->ref;
  const uint32_t nt = p.first[ng];
  tracyhip_assemble_job job{};
  job.ngroups = ng;
  job.traces = p.tp.set();
  job.group_first = p.first.data();
  job.references = refs.set();
  job.ref_index = ridx.data();
  job.match_fraction = c.matchFraction;
  job.fraction_called = c.fractionCalled;
  job.include_reference = c.incRef ? 1u : 0u;
  std::vector<int32_t> sf(nt), sr(nt);
  std::vector<uint8_t> fwd(nt);
  std::vector<uint32_t> rank(nt);
  tracyhip_assemble_result res{sf.data(), sr.data(), fwd.data(), rank.data(), p.nrows.data(), p.ncol.data(), p.rows.data(), p.gapped.data(),
                               p.cons.data(), p.qual.data(), p.clen.data(), p.roff.data(), p.coff.data()};
  tracyhip_params semi{c.match, c.mismatch, c.gapopen, c.gapext, 1, 0};  // AlignConfig<true,false>
  if (tracyhip_assemble_traces(ctx, &job, &semi, TRACYHIP_MEM_HOST, &res) != TRACYHIP_OK) {
    gpu_fail("assembly");
    return false;
  }
  for (uint32_t g = 0; g < ng; ++g) {
    AsmGroup& a = *gs[g];
    a.scoreIdx.assign(p.nrows[g] ? p.nrows[g] - 1 : 0, TraceScore{0, 0, 0, true});
    for (uint32_t t = p.first[g]; t < p.first[g + 1]; ++t) {
      const uint32_t i = t - p.first[g];
      if (rank[t] == UINT32_MAX) a.excluded.push_back(i);
      else a.scoreIdx[rank[t]] = TraceScore{std::max(sf[t], sr[t]), (int32_t)i, (int32_t)rank[t], fwd[t] != 0};
    }
  }
  p.unpack(gs);
  return true;
}

// all trees of `gs` (every one loaded) through one device call; fills excluded / idxMap / fwd / seqidx / align / gapped / cs / qstr
bool denovo_device(tracyhip_ctx* ctx, AssembleConfig const& c, std::vector<AsmGroup*> const& gs) {
  const uint32_t ng = (uint32_t)gs.size();
  if (ng == 0) return true;
  GroupPack p(gs, 0, [](AsmGroup const&, uint64_t sum) { return sum; });  // K x sum len
  const uint32_t nt = p.first[ng];
  tracyhip_denovo_job job{};
  job.ngroups = ng;
  job.traces = p.tp.set();
  job.group_first = p.first.data();
  job.match_fraction = c.matchFraction;
  job.fraction_called = c.fractionCalled;
  std::vector<uint8_t> fwd(nt);
  std::vector<uint32_t> partner(nt), row(nt);
  tracyhip_denovo_result res{fwd.data(), partner.data(), row.data(), p.nrows.data(), p.ncol.data(), p.rows.data(), p.gapped.data(),
                             p.cons.data(), p.qual.data(), p.clen.data(), p.roff.data(), p.coff.data()};
  tracyhip_params endfree{c.match, c.mismatch, c.gapopen, c.gapext, 1, 1};  // AlignConfig<true,true>
  if (tracyhip_denovo_traces(ctx, &job, &endfree, TRACYHIP_MEM_HOST, &res) != TRACYHIP_OK) {
    gpu_fail("assembly");
    return false;
  }
  for (uint32_t g = 0; g < ng; ++g) {
    AsmGroup& a = *gs[g];
    a.seqidx.assign(p.nrows[g], 0);
    for (uint32_t t = p.first[g]; t < p.first[g + 1]; ++t) {
      const uint32_t i = t - p.first[g];
      if (partner[t] == UINT32_MAX) { a.excluded.push_back(i); continue; }
      if (row[t] != UINT32_MAX && row[t] < p.nrows[g]) a.seqidx[row[t]] = (uint32_t)a.idxMap.size();
      a.idxMap.push_back(i);
      a.fwd.push_back(fwd[t] != 0);
    }
  }
  p.unpack(gs);
  return true;
}

int assemble_batch(AssembleConfig const& c, int argc, char** argv) {
  std::vector<AsmGroup> groups;
  std::vector<std::string> ref_paths;
  {
    std::ifstream mf(c.batch.c_str());
    if (!mf) {
      std::cerr << "Manifest is missing: " << c.batch << std::endl;
      return 1;
    }
    std::map<std::string, uint32_t> by_prefix, by_ref;
    std::string line;
    uint32_t lineno = 0;
    while (std::getline(mf, line)) {
      ++lineno;
      if (line.empty() || line[0] == '#') continue;
      std::istringstream ss(line);
      std::string trace, ref, prefix;
      if (!std::getline(ss, trace, '\t') || !std::getline(ss, ref, '\t') || !std::getline(ss, prefix, '\t') || trace.empty() || prefix.empty()) {
        std::cerr << "Malformed manifest line " << lineno << ": " << line << std::endl;
        return 1;
      }
      if (c.denovo && !ref.empty() && ref != "-") {
        std::cerr << "Manifest line " << lineno << ": --denovo takes no reference, the line names " << ref << std::endl;
        return 1;
      }
      if (ref.empty() || ref == "-") ref = c.reference;
      auto r = by_ref.find(ref);
      if (r == by_ref.end()) {
        r = by_ref.emplace(ref, (uint32_t)ref_paths.size()).first;
        ref_paths.push_back(ref);
      }
      auto it = by_prefix.find(prefix);
      if (it == by_prefix.end()) {
        it = by_prefix.emplace(prefix, (uint32_t)groups.size()).first;
        groups.emplace_back();
        groups.back().c = c;
        groups.back().c.outprefix = prefix;
        groups.back().c.ab.clear();
        groups.back().ref = r->second;
      } else if (groups[it->second].ref != r->second) {
        std::cerr << "Manifest line " << lineno << ": outprefix " << prefix << " already has the reference " << ref_paths[groups[it->second].ref]
                  << ", not " << ref << std::endl;
        return 1;
      }
      groups[it->second].c.ab.push_back(trace);
    }
  }
  for (AsmGroup const& g : groups)
    for (auto const& p : g.c.ab)
      if (!regular_nonempty(p)) {
        std::cerr << "Trace file is missing: " << p << std::endl;
        return 1;
      }
  echo_command(argc, argv);
  detail::ProfilePack refs;
  for (std::string const& path : ref_paths) {
    if (c.denovo) break;  // (one entry: the empty path every line stands for)
    std::string faname, seq;
    if (!loadSingleFasta(path, faname, seq)) return -1;
    if (seq.size() > kMaxSingleFasta) {
      std::cerr << "Reference is larger than 50Kbp. Please use a smaller reference slice!" << std::endl;
      return -1;
    }
    Profile p;
    createProfile(seq, p);
    refs.add(p);
  }
  std::cout << stamp() << "Load ab1 files" << std::endl;
  const uint32_t nthreads = c.threads ? c.threads : usable_cores();
  StageTimes times;
  std::atomic<int> failed(0);
  auto prep = [&](uint32_t lo, uint32_t hi) {
    Stopwatch sw;
    std::vector<std::pair<uint32_t, uint32_t>> work;  // (group, trace)
    for (uint32_t g = lo; g < hi; ++g) {
      groups[g].traces.assign(groups[g].c.ab.size(), AsmTrace());
      for (uint32_t i = 0; i < groups[g].c.ab.size(); ++i) work.emplace_back(g, i);
    }
    std::vector<int> rcs(work.size(), 0);
    for_each_index((uint32_t)work.size(), nthreads, [&](uint32_t w) {
      AsmGroup& g = groups[work[w].first];
      rcs[w] = load_asm_trace(g.c, g.c.ab[work[w].second], g.traces[work[w].second]);
    });
    for (uint32_t g = lo; g < hi; ++g) groups[g].ok = true;
    for (std::size_t w = 0; w < work.size(); ++w)
      if (rcs[w] != 0) groups[work[w].first].ok = false;
    for (uint32_t g = lo; g < hi; ++g)
      if (!groups[g].ok) {  // (too stringent trimming, no basecalls, unreadable: what ends the one-group command)
        std::cerr << "skipping " << groups[g].c.outprefix << std::endl;
        groups[g].traces.clear();
        ++failed;
      }
    times.add("read_basecall_profile_s", sw.seconds());
  };
  Device dev;
  std::future<int> dev_ready = std::async(std::launch::async, [&]() {
    Stopwatch sw;
    const int rc = tracyhip_create(c.device, &dev.ctx) == TRACYHIP_OK ? 0 : -1;
    times.add("gpu_init_s", sw.seconds());
    return rc;
  });
  bool dev_open = false;
  auto device = [&](uint32_t lo, uint32_t hi) -> bool {
    if (!dev_open) {
      if (dev_ready.get() != 0) {
        gpu_fail("no usable GPU");
        return false;
      }
      dev_open = true;
      std::cout << stamp() << "Align ab1 files" << std::endl;
    }
    Stopwatch sw;
    std::vector<AsmGroup*> gs;
    for (uint32_t g = lo; g < hi; ++g)
      if (groups[g].ok) gs.push_back(&groups[g]);
    const bool ok = c.denovo ? denovo_device(dev.ctx, c, gs) : assemble_device(dev.ctx, c, refs, gs);
    times.add("device_s", sw.seconds());
    return ok;
  };
  auto write = [&](uint32_t lo, uint32_t hi) {
    Stopwatch sw;
    for (uint32_t g = lo; g < hi; ++g) {  // (the warnings in manifest order)
      for (uint32_t i : groups[g].excluded)
        std::cerr << "Warning: " << stem(groups[g].c.ab[i]) << (c.denovo ? " is not matching to any of the other traces!" : " is not matching to the reference!")
                  << " Trace file will be excluded!" << std::endl;
      if (c.denovo && groups[g].ok && groups[g].align.empty()) {  // (what ends the one-group command, assemble.h:459-462)
        std::cerr << "At least 2 traces are required for de novo assembly!" << std::endl;
        std::cerr << "skipping " << groups[g].c.outprefix << std::endl;
        groups[g].ok = false;
        ++failed;
      }
    }
    for_each_index(hi - lo, nthreads, [&](uint32_t i) {
      AsmGroup& g = groups[lo + i];
      if (g.ok) {
        if (c.denovo) write_denovo_outputs(g.c, g.traces, g.idxMap, g.fwd, g.seqidx, g.align, g.gapped, g.cs);
        else if (!g.scoreIdx.empty()) write_ref_guided_outputs(g.c, g.traces, g.scoreIdx, g.align, g.gapped, g.cs);
        write_assembly_outputs(g.c, g.align, g.gapped, g.cs, g.qstr);
      }
      AsmGroup done;
      done.ok = g.ok;
      g = std::move(done);  // the block's traces and rows are released here
    });
    times.add("writers_s", sw.seconds());
  };
  if (!run_blocks((uint32_t)groups.size(), block_size(), prep, device, write)) return -1;
  times.report((uint32_t)groups.size(), nthreads);
  std::cout << stamp() << "Done." << std::endl;
  end_process(failed ? 2 : 0);
}

int assemble_main(int argc, char** argv) {
  AssembleConfig c;
  if (parse_assemble(argc, argv, c)) {
    std::cout << "Usage: tracy " << argv[0] << " [OPTIONS] trace1.ab1 trace2.ab1 ..." << std::endl;
    std::cout << "       tracy " << argv[0] << " [OPTIONS] -r reference.fa --batch manifest.tsv" << std::endl;
    std::cout << "       tracy " << argv[0] << " [OPTIONS] --denovo --batch manifest.tsv" << std::endl;
    std::cout << "Generic options:\n"
                 "  -? [ --help ]                    show help message\n"
                 "  -r [ --reference ] arg           reference-guided assembly (optional)\n"
                 "  -p [ --pratio ] arg (=0.33)      peak ratio to call base\n"
                 "  -t [ --trim ] arg (=4)           trimming stringency [1:9], 0: disable trimming\n"
                 "  -f [ --fracmatch ] arg (=0.5)    min. fraction of matches [0:1]\n"
                 "\nAlignment options:\n"
                 "  -g [ --gapopen ] arg (=-10)      gap open\n"
                 "  -e [ --gapext ] arg (=-4)        gap extension\n"
                 "  -m [ --match ] arg (=3)          match\n"
                 "  -n [ --mismatch ] arg (=-5)      mismatch\n"
                 "\nOutput options:\n"
                 "  -d [ --called ] arg (=0.1)       fraction of traces required for consensus\n"
                 "  -o [ --outprefix ] arg (=out)    output prefix\n"
                 "  -a [ --format ] arg (=fasta)     consensus output format [fasta|fastq]\n"
                 "  -i [ --inccons ]                 include consensus in FASTA align\n"
                 "  -j [ --incref ]                  include reference in consensus computation (req. --reference)\n"
                 "\nBatch options:\n"
                 "  --batch arg                      manifest: trace<TAB>reference<TAB>outprefix per line; the lines of one outprefix\n"
                 "                                   are one assembly (all of them on the GPU in one call; requires --reference,\n"
                 "                                   which an empty or '-' reference field stands for)\n"
                 "  --denovo                         with --batch: every assembly of the manifest is de novo (all of them on the GPU in\n"
                 "                                   one call; the reference field of every line is empty or '-', no --reference)\n"
                 "  --threads arg (=0)               host threads of the --batch stages (0 = all usable cores)\n\n";
    return -1;
  }
  if (c.denovo && c.batch.empty()) {
    std::cerr << "--denovo needs --batch: one de novo assembly per command is the default without -r" << std::endl;
    return 1;
  }
  if (c.denovo && c.hasReference) {
    std::cerr << "--denovo takes no reference (-r): a reference-guided batch is -r with --batch" << std::endl;
    return 1;
  }
  for (auto const& p : c.ab)
    if (!regular_nonempty(p)) {
      std::cerr << "Trace file is missing: " << p << std::endl;
      return 1;
    }
  if (c.trimStringency != 0) {
    if (c.trimStringency > 9) c.trimStringency = 9;
    else if (c.trimStringency < 1) c.trimStringency = 1;
  }
  if (c.matchFraction < 0) c.matchFraction = 0;
  else if (c.matchFraction > 1) c.matchFraction = 1;
  if (!c.batch.empty()) {
    if (!c.hasReference && !c.denovo) {
      std::cerr << "--batch needs a reference (-r): only reference-guided assemblies have a batch mode, de novo assembly runs one per command" << std::endl;
      return 1;
    }
    return assemble_batch(c, argc, argv);
  }
  echo_command(argc, argv);

  Device dev;
  if (tracyhip_create(c.device, &dev.ctx) != TRACYHIP_OK) {
    gpu_fail("no usable GPU");
    return -1;
  }
  tracyhip_params semi{c.match, c.mismatch, c.gapopen, c.gapext, 1, 0};   // AlignConfig<true,false>
  tracyhip_params endfree{c.match, c.mismatch, c.gapopen, c.gapext, 1, 1};  // AlignConfig<true,true>
  CharAlign align;
  std::string gapped, cs, qstr;
  const uint32_t ntr = (uint32_t)c.ab.size();
  std::vector<AsmTrace> traces(ntr);

  if (c.hasReference) {
    std::string faname, seq;
    if (!loadSingleFasta(c.reference, faname, seq)) return -1;
    if (seq.size() > kMaxSingleFasta) {
      std::cerr << "Reference is larger than 50Kbp. Please use a smaller reference slice!" << std::endl;
      return -1;
    }
    Profile prefslice;
    createProfile(seq, prefslice);
    std::cout << stamp() << "Align ab1 files" << std::endl;
    std::vector<Profile> rev(ntr);
    for (uint32_t i = 0; i < ntr; ++i) {
      std::cout << "Processing " << c.ab[i] << " [" << i << "]" << std::endl;
      if (int rc = load_asm_trace(c, c.ab[i], traces[i])) return rc;
      reverseComplementProfile(traces[i].prof, rev[i]);
    }
    // both strands of every trace against the reference: one device batch
    std::vector<int32_t> gs;
    {
      std::vector<Profile> a1;
      for (uint32_t i = 0; i < ntr; ++i) { a1.push_back(traces[i].prof); a1.push_back(rev[i]); }
      std::vector<Profile> a2(1, prefslice);
      std::vector<uint32_t> i1(2 * ntr), i2(2 * ntr, 0);
      for (uint32_t k = 0; k < 2 * ntr; ++k) i1[k] = k;
      tracyhip_params p = semi;
      detail::ProfilePack p1, p2;
      for (auto const& x : a1) p1.add(x);
      p2.add(prefslice);
      tracyhip_pairs pr{};
      pr.npairs = 2 * ntr;
      pr.a1 = p1.set();
      pr.a2 = p2.set();
      pr.a1_index = i1.data();
      pr.a2_index = i2.data();
      gs.assign(2 * ntr, 0);
      if (ntr && tracyhip_gotoh_score(dev.ctx, &pr, &p, TRACYHIP_MEM_HOST, gs.data()) != TRACYHIP_OK) return gpu_fail("scores"), -1;
    }
    std::vector<Profile> traceProfiles;
    std::vector<TraceScore> scoreIdx;
    for (uint32_t i = 0; i < ntr; ++i) {
      const int32_t gsFwd = gs[2 * i], gsRev = gs[2 * i + 1];
      const double seqsize = (double)traces[i].prof.cols;
      const double thr = seqsize * c.matchFraction * c.match + seqsize * (1 - c.matchFraction) * c.mismatch;
      if (gsFwd > thr || gsRev > thr) {
        const bool f = gsFwd >= gsRev;
        scoreIdx.push_back(TraceScore{std::max(gsFwd, gsRev), (int32_t)i, (int32_t)scoreIdx.size(), f});
        traceProfiles.push_back(f ? traces[i].prof : rev[i]);
      } else {
        std::cerr << "Warning: " << stem(c.ab[i]) << " is not matching to the reference! Trace file will be excluded!" << std::endl;
      }
    }
    std::sort(scoreIdx.begin(), scoreIdx.end());
    if (!scoreIdx.empty()) {
      // iterative alignment, best trace first (assemble.h:248-283)
      std::vector<int32_t> sc;
      std::vector<std::string> ops;
      {
        std::vector<Profile const*> a1(1, &traceProfiles[scoreIdx[0].newidx]), a2(1, &prefslice);
        if (!align_profiles(dev.ctx, semi, a1, a2, sc, ops)) return -1;
        align.assign(2, std::string());
        align[0] = profile_row(*a1[0], ops[0], true);
        align[1] = profile_row(prefslice, ops[0], false);
      }
      for (std::size_t i = 1; i < scoreIdx.size(); ++i) {
        Profile alignProfile;
        createProfile(align, alignProfile);
        std::vector<Profile const*> a1(1, &traceProfiles[scoreIdx[i].newidx]), a2(1, &alignProfile);
        if (!align_profiles(dev.ctx, semi, a1, a2, sc, ops)) return -1;
        CharAlign combined(align.size() + 1, std::string(ops[0].size(), '-'));
        combined[0] = profile_row(*a1[0], ops[0], true);
        std::size_t ap = 0;
        for (std::size_t j = 0; j < ops[0].size(); ++j) {
          if (ops[0][j] == 'v') continue;  // alignNew[1][j] == '-'
          for (std::size_t k = 1; k < combined.size(); ++k) combined[k][j] = align[k - 1][ap];
          ++ap;
        }
        align.swap(combined);
      }
      consensus(c.fractionCalled, align, gapped, cs, qstr, !c.incRef);
      write_ref_guided_outputs(c, traces, scoreIdx, align, gapped, cs);
    }
  } else {
    std::cout << stamp() << "Load ab1 files" << std::endl;
    std::vector<Profile> inputProfiles(ntr);
    std::vector<bool> fwdProfiles(ntr, true);
    for (uint32_t i = 0; i < ntr; ++i) {
      if (int rc = load_asm_trace(c, c.ab[i], traces[i])) return rc;
      inputProfiles[i] = traces[i].prof;
    }
    std::cout << stamp() << "Optimize layout" << std::endl;
    if (revSeqBasedOnDist(dev.ctx, endfree, inputProfiles, fwdProfiles) != TRACYHIP_OK) return gpu_fail("strand assignment"), -1;
    // a trace stays if it overlaps some other trace well enough (assemble.h:425-455).  The reference walks j = 0, 1, ...
    // and stops at the first hit; here every still-undecided trace tries its next partner per round, one batch per round.
    std::vector<int32_t> next(ntr, 0);
    std::vector<int8_t> state(ntr, 0);  // 0 undecided, 1 kept, -1 excluded
    for (;;) {
      std::vector<Profile const*> a1, a2;
      std::vector<uint32_t> who;
      for (uint32_t i = 0; i < ntr; ++i) {
        if (state[i]) continue;
        if (next[i] == (int32_t)i) ++next[i];
        if (next[i] >= (int32_t)ntr) { state[i] = -1; continue; }
        a1.push_back(&inputProfiles[i]);
        a2.push_back(&inputProfiles[next[i]]);
        who.push_back(i);
      }
      if (who.empty()) break;
      std::vector<int32_t> sc;
      std::vector<std::string> ops;
      if (!align_profiles(dev.ctx, endfree, a1, a2, sc, ops)) return -1;
      for (std::size_t k = 0; k < who.size(); ++k) {
        const uint32_t i = who[k];
        int32_t numAligned = 0;
        for (char op : ops[k]) numAligned += op == 's';
        const double frac = (double)numAligned / (double)(int32_t)inputProfiles[i].cols;
        const double thr = numAligned * c.matchFraction * c.match + numAligned * (1 - c.matchFraction) * c.mismatch;
        if (frac > 0.1 && numAligned > 25 && sc[k] > thr) state[i] = 1;
        else ++next[i];
      }
    }
    std::vector<Profile> seqProfiles;
    std::vector<uint32_t> idxMap;
    std::vector<bool> fwd;
    for (uint32_t i = 0; i < ntr; ++i) {
      if (state[i] != 1) {
        std::cerr << "Warning: " << stem(c.ab[i]) << " is not matching to any of the other traces! Trace file will be excluded!" << std::endl;
        continue;
      }
      seqProfiles.push_back(inputProfiles[i]);
      idxMap.push_back(i);
      fwd.push_back(fwdProfiles[i]);
    }
    if (fwd.size() < 2) {
      std::cerr << "At least 2 traces are required for de novo assembly!" << std::endl;
      return -1;
    }
    std::cout << stamp() << "Assemble traces" << std::endl;
    std::vector<uint32_t> seqidx;
    if (msa(dev.ctx, endfree, seqProfiles, align, seqidx) != TRACYHIP_OK) return gpu_fail("msa"), -1;
    consensus(c.fractionCalled, align, gapped, cs, qstr, false);
    write_denovo_outputs(c, traces, idxMap, fwd, seqidx, align, gapped, cs);
  }
  write_assembly_outputs(c, align, gapped, cs, qstr);
  std::cout << stamp() << "Done." << std::endl;
  return 0;
}
