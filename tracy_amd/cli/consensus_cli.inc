// consensus_cli.inc -- `tracy consensus` (consensus.h:332-598) on the C ABI; included by tracy_amd_cli.cpp.
//
//   tracy_amd_cli consensus [options] trace1.ab1 trace2.ab1
//   tracy_amd_cli consensus [options] --batch manifest.tsv     lines: trace1 <TAB> trace2 <TAB> outprefix
//
// Two traces: strand of the second by gotohScore (AlignConfig<true,true>), profile x profile alignment on the
// device, then the genotype-likelihood consensus on the host.  Files: <prefix>_1st.abif, _2nd.abif, .align.fa,
// .fa, .fq, .txt.
//
// --batch: every pair of the manifest through tracyhip_consensus_traces (consensus.hip) in blocks (run_blocks): host threads read,
// basecall, trim and profile block k + 1 and write the files of block k - 1 while one device call runs block k.  The files of a pair
// are byte for byte those of the two-file command.

struct ConsJob {
  std::string path[2], outprefix;
  bool ok = false;
  Profile p1, f2;  // trimmed profile of trace 1, trimmed forward profile of trace 2
  // results
  bool forward = true, overlap = false;
  int32_t score = 0;
  AlignRows rows;
  std::string cons;
  std::vector<uint32_t> qual;
};

struct ConsBatchOptions {
  ConsensusOptions co;
  uint16_t linelimit, tl1, tr1, tl2, tr2;
  int32_t gapopen, gapext, match, mismatch;
  uint32_t minOverlap;
  float matchFraction, pratio, trimStringency;
  int device;
};

// the host stages of one pair up to its profiles (the two-file command's steps and messages); returns the CLI exit code
int consensus_prepare(ConsBatchOptions const& o, ConsJob& j) {
  Trace tr[2];
  BaseCalls bc[2];
  for (int k = 0; k < 2; ++k) {
    if (!load_trace(j.path[k], tr[k])) return -1;
    if (tr[k].basecallpos.empty()) {
      std::cerr << "Trace file lacks basecalls!" << std::endl;
      return -1;
    }
  }
  for (int k = 0; k < 2; ++k) basecall(tr[k], bc[k], o.pratio);
  uint32_t tl1 = o.tl1, tr1 = o.tr1, tl2 = o.tl2, tr2 = o.tr2;
  if (o.trimStringency >= 1) {
    uint32_t l = 0, r = 0;
    trimTrace(o.trimStringency, bc[0], l, r);
    tl1 = (uint16_t)l; tr1 = (uint16_t)r;
    l = 0; r = 0;
    trimTrace(o.trimStringency, bc[1], l, r);
    tl2 = (uint16_t)l; tr2 = (uint16_t)r;
  }
  if (tl1 + tr1 >= bc[0].bcPos.size()) {
    std::cerr << "The sum of the left and right trim size is larger than the trace: " << j.path[0] << std::endl;
    return -1;
  }
  if (tl2 + tr2 >= bc[1].bcPos.size()) {
    std::cerr << "The sum of the left and right trim size is larger than the trace:" << j.path[1] << std::endl;
    return -1;
  }
  traceTxtOut(j.outprefix + "_1st.abif", bc[0], tr[0], tl1, tr1);
  traceTxtOut(j.outprefix + "_2nd.abif", bc[1], tr[1], tl2, tr2);
  createProfile(tr[0], bc[0], j.p1, tl1, tr1);
  createProfile(tr[1], bc[1], j.f2, tl2, tr2);
  return 0;
}

// one block of pairs through one tracyhip_consensus_traces call
bool consensus_device(tracyhip_ctx* ctx, ConsBatchOptions const& o, std::vector<ConsJob*> const& js) {
  const uint32_t np = (uint32_t)js.size();
  if (np == 0) return true;
  std::vector<uint64_t> o1(np), o2(np), off(np);
  std::vector<uint32_t> l1(np), l2(np);
  uint64_t n1 = 0, n2 = 0, tot = 0;
  for (uint32_t i = 0; i < np; ++i) {
    l1[i] = (uint32_t)js[i]->p1.cols;
    l2[i] = (uint32_t)js[i]->f2.cols;
    o1[i] = n1; n1 += 6ull * l1[i];
    o2[i] = n2; n2 += 6ull * l2[i];
    off[i] = tot; tot += (uint64_t)l1[i] + l2[i];
  }
  std::vector<float> d1(n1), d2(n2);
  for (uint32_t i = 0; i < np; ++i) {
    std::copy(js[i]->p1.v.begin(), js[i]->p1.v.end(), d1.begin() + o1[i]);
    std::copy(js[i]->f2.v.begin(), js[i]->f2.v.end(), d2.begin() + o2[i]);
  }
  tracyhip_consensus_job job{};
  job.npairs = np;
  job.first = tracyhip_seqset{TRACYHIP_SEQ_PROFILE, d1.data(), o1.data(), l1.data(), np};
  job.second = tracyhip_seqset{TRACYHIP_SEQ_PROFILE, d2.data(), o2.data(), l2.data(), np};
  job.compute_union = o.co.computeUnion ? 1 : 0;
  job.iupac = o.co.useIUPAC ? 1 : 0;
  job.min_overlap = o.minOverlap;
  job.match_fraction = o.matchFraction;
  std::vector<int32_t> sf(np), sr(np), sc(np), status(np);
  std::vector<uint8_t> fwd(np), r0(std::max<uint64_t>(tot, 1)), r1(std::max<uint64_t>(tot, 1)), cons(std::max<uint64_t>(tot, 1));
  std::vector<uint32_t> na(np), nm(np), olen(np), clen(np);
  std::vector<uint16_t> qual(std::max<uint64_t>(tot, 1));
  tracyhip_consensus_result res{sf.data(), sr.data(), fwd.data(), sc.data(), na.data(), nm.data(), status.data(), r0.data(), r1.data(),
                                olen.data(), cons.data(), qual.data(), clen.data(), off.data()};
  tracyhip_params endfree{o.match, o.mismatch, o.gapopen, o.gapext, 1, 1};  // AlignConfig<true,true> ("global" in consensus.h:464)
  if (tracyhip_consensus_traces(ctx, &job, &endfree, TRACYHIP_MEM_HOST, &res) != TRACYHIP_OK) {
    gpu_fail("consensus");
    return false;
  }
  for (uint32_t i = 0; i < np; ++i) {
    ConsJob& j = *js[i];
    j.forward = fwd[i] != 0;
    j.score = sc[i];
    j.overlap = status[i] == TRACYHIP_CONS_OK;
    j.rows.row0.assign(reinterpret_cast<const char*>(r0.data() + off[i]), olen[i]);
    j.rows.row1.assign(reinterpret_cast<const char*>(r1.data() + off[i]), olen[i]);
    j.cons.assign(reinterpret_cast<const char*>(cons.data() + off[i]), clen[i]);
    j.qual.assign(qual.begin() + off[i], qual.begin() + off[i] + clen[i]);
    j.p1 = Profile();
    j.f2 = Profile();
  }
  return true;
}

// the files the two-file command writes after the overlap test, composed in memory and written once each
void consensus_write(ConsBatchOptions const& o, ConsJob const& j) {
  auto put = [](std::string const& path, std::ostringstream const& os) {
    TextBuf b(os.str().size() + 16);
    b << os.str();
    b.write(path);
  };
  {
    std::ostringstream v;
    v << ">" << stem(j.path[0]) << std::endl << j.rows.row0 << std::endl;
    v << ">" << stem(j.path[1]) << (j.forward ? " (forward)" : " (reverse)") << std::endl << j.rows.row1 << std::endl;
    put(j.outprefix + ".align.fa", v);
  }
  {
    std::ostringstream f;
    consensusFastaOut(f, o.co, j.cons);
    put(j.outprefix + ".fa", f);
  }
  {
    std::ostringstream f;
    consensusFastqOut(f, o.co, j.cons, j.qual);
    put(j.outprefix + ".fq", f);
  }
  {
    std::ostringstream f;
    plotClustalPairwise(f, j.rows, stem(j.path[0]), stem(j.path[1]), j.forward, j.score, o.linelimit);
    put(j.outprefix + ".txt", f);
  }
}

int consensus_batch(ConsBatchOptions const& o, std::string const& manifest, int argc, char** argv) {
  std::vector<ConsJob> jobs;
  {
    std::ifstream mf(manifest.c_str());
    if (!mf) {
      std::cerr << "Manifest is missing: " << manifest << std::endl;
      return 1;
    }
    std::string line;
    while (std::getline(mf, line)) {
      if (line.empty() || line[0] == '#') continue;
      std::istringstream ss(line);
      ConsJob j;
      if (!std::getline(ss, j.path[0], '\t') || !std::getline(ss, j.path[1], '\t') || !std::getline(ss, j.outprefix, '\t')) {
        std::cerr << "Malformed manifest line: " << line << std::endl;
        return 1;
      }
      jobs.push_back(std::move(j));
    }
  }
  for (ConsJob const& j : jobs)
    for (int k = 0; k < 2; ++k)
      if (!regular_nonempty(j.path[k])) {
        std::cerr << "Input trace file is missing: " << file_name(j.path[k]) << std::endl;
        return 1;
      }
  echo_command(argc, argv);
  std::cout << stamp() << "Load ab1 files" << std::endl;
  const uint32_t nthreads = usable_cores();
  StageTimes times;
  std::atomic<int> failed(0), no_overlap(0);
  auto prep = [&](uint32_t lo, uint32_t hi) {
    Stopwatch sw;
    std::vector<int> rcs(hi - lo, 0);
    for_each_index(hi - lo, nthreads, [&](uint32_t i) { rcs[i] = consensus_prepare(o, jobs[lo + i]); });
    for (uint32_t i = lo; i < hi; ++i) {
      if (rcs[i - lo] != 0) {
        std::cerr << "skipping " << jobs[i].path[0] << " " << jobs[i].path[1] << std::endl;
        ++failed;
      } else {
        jobs[i].ok = true;
      }
    }
    times.add("read_basecall_profile_s", sw.seconds());
  };
  Device dev;
  std::future<int> dev_ready = std::async(std::launch::async, [&]() {
    Stopwatch sw;
    const int rc = tracyhip_create(o.device, &dev.ctx) == TRACYHIP_OK ? 0 : -1;
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
      std::cout << stamp() << "Alignment" << std::endl;
    }
    Stopwatch sw;
    std::vector<ConsJob*> js;
    for (uint32_t i = lo; i < hi; ++i)
      if (jobs[i].ok) js.push_back(&jobs[i]);
    const bool ok = consensus_device(dev.ctx, o, js);
    times.add("device_s", sw.seconds());
    return ok;
  };
  bool said_out = false;
  auto write = [&](uint32_t lo, uint32_t hi) {
    Stopwatch sw;
    if (!said_out) std::cout << stamp() << "Output" << std::endl;
    said_out = true;
    for (uint32_t i = lo; i < hi; ++i)  // (the messages of pairs without overlap in manifest order)
      if (jobs[i].ok && !jobs[i].overlap) {
        std::cerr << "Error: No sufficient trace overlap! (" << jobs[i].outprefix << ")" << std::endl;
        ++no_overlap;
      }
    for_each_index(hi - lo, nthreads, [&](uint32_t i) {
      ConsJob& j = jobs[lo + i];
      if (j.ok && j.overlap) consensus_write(o, j);
      ConsJob done;
      done.ok = j.ok;
      j = std::move(done);  // the block's results are released here
    });
    times.add("writers_s", sw.seconds());
  };
  if (!run_blocks((uint32_t)jobs.size(), block_size(), prep, device, write)) return -1;
  times.report((uint32_t)jobs.size(), nthreads);
  std::cout << stamp() << "Done." << std::endl;
  const int rc = (failed || TextBuf::write_errors()) ? 2 : no_overlap ? 1 : 0;
  end_process(rc);
}

int consensus_main(int argc, char** argv) {
  ConsensusOptions co;
  uint16_t linelimit = 60, tl1 = 50, tr1 = 50, tl2 = 50, tr2 = 50;
  int32_t gapopen = -10, gapext = -4, match = 3, mismatch = -5;
  uint32_t minOverlap = 25;
  float matchFraction = 0.5f, pratio = 0.33f, trimStringency = 0;
  std::string outprefix = "out", batch;
  std::vector<std::string> files;
  int device = 0;
  static const std::map<std::string, char> longs = {{"help", '?'}, {"label", 'b'}, {"pratio", 'p'}, {"fracmatch", 'f'}, {"minoverlap", 'c'},
                                                    {"gapopen", 'g'}, {"gapext", 'e'}, {"match", 'm'}, {"mismatch", 'n'}, {"trim", 't'},
                                                    {"trimLeft1", 'q'}, {"trimRight1", 'u'}, {"trimLeft2", 'r'}, {"trimRight2", 's'},
                                                    {"linelimit", 'l'}, {"outprefix", 'o'}, {"intersect", 'i'}, {"iupac", 'a'}, {"device", 'D'},
                                                    {"batch", 'B'}};
  bool bad = false;
  for (int i = 1; i < argc && !bad; ++i) {
    std::string a = argv[i], val;
    char opt = 0;
    bool has_val = false;
    if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
      std::string name = a.substr(2);
      const std::size_t eq = name.find('=');
      if (eq != std::string::npos) { val = name.substr(eq + 1); name = name.substr(0, eq); has_val = true; }
      auto it = longs.find(name);
      if (it == longs.end()) { std::cerr << "unrecognised option '" << a << "'" << std::endl; bad = true; break; }
      opt = it->second;
    } else if (a.size() >= 2 && a[0] == '-' && !(a[1] >= '0' && a[1] <= '9')) {
      opt = a[1];
      if (a.size() > 2) { val = a.substr(2); has_val = true; }
    } else {
      files.push_back(a);
      continue;
    }
    if (opt == '?') { bad = true; break; }
    if (opt == 'i') { co.computeUnion = false; continue; }
    if (opt == 'a') { co.useIUPAC = true; continue; }
    if (!has_val) {
      if (i + 1 >= argc) { std::cerr << "the required argument for option '" << a << "' is missing" << std::endl; bad = true; break; }
      val = argv[++i];
    }
    switch (opt) {
      case 'b': co.label = val; break;
      case 'p': pratio = std::strtof(val.c_str(), nullptr); break;
      case 'f': matchFraction = std::strtof(val.c_str(), nullptr); break;
      case 'c': minOverlap = (uint32_t)std::strtoul(val.c_str(), nullptr, 10); break;
      case 'g': gapopen = std::atoi(val.c_str()); break;
      case 'e': gapext = std::atoi(val.c_str()); break;
      case 'm': match = std::atoi(val.c_str()); break;
      case 'n': mismatch = std::atoi(val.c_str()); break;
      case 't': trimStringency = std::strtof(val.c_str(), nullptr); break;
      case 'q': tl1 = (uint16_t)std::atoi(val.c_str()); break;
      case 'u': tr1 = (uint16_t)std::atoi(val.c_str()); break;
      case 'r': tl2 = (uint16_t)std::atoi(val.c_str()); break;
      case 's': tr2 = (uint16_t)std::atoi(val.c_str()); break;
      case 'l': linelimit = (uint16_t)std::atoi(val.c_str()); break;
      case 'o': outprefix = val; break;
      case 'D': device = std::atoi(val.c_str()); break;
      case 'B': batch = val; break;
      default: std::cerr << "unrecognised option '" << a << "'" << std::endl; bad = true; break;
    }
  }
  if (bad || (files.empty() == batch.empty())) {
    std::cout << "Usage: tracy " << argv[0] << " [OPTIONS] trace1.ab1 trace2.ab1" << std::endl;
    std::cout << "       tracy " << argv[0] << " [OPTIONS] --batch manifest.tsv" << std::endl;
    std::cout << "Generic options:\n"
                 "  -? [ --help ]                    show help message\n"
                 "  -b [ --label ] arg (=Consensus)  sample label\n"
                 "  -p [ --pratio ] arg (=0.33)      peak ratio to call base\n"
                 "  -f [ --fracmatch ] arg (=0.5)    min. fraction of matches [0:1]\n"
                 "  -c [ --minoverlap ] arg (=25)    min. overlap length\n"
                 "\nAlignment options:\n"
                 "  -g [ --gapopen ] arg (=-10)      gap open\n"
                 "  -e [ --gapext ] arg (=-4)        gap extension\n"
                 "  -m [ --match ] arg (=3)          match\n"
                 "  -n [ --mismatch ] arg (=-5)      mismatch\n"
                 "\nTrimming options:\n"
                 "  -t [ --trim ] arg (=0)           trimming stringency [1:9], 0: use trimLeft and trimRight\n"
                 "  -q [ --trimLeft1 ] arg (=50)     trim size left (1st trace)\n"
                 "  -u [ --trimRight1 ] arg (=50)    trim size right (1st trace)\n"
                 "  -r [ --trimLeft2 ] arg (=50)     trim size left (2nd trace)\n"
                 "  -s [ --trimRight2 ] arg (=50)    trim size right (2nd trace)\n"
                 "\nOutput options:\n"
                 "  -l [ --linelimit ] arg (=60)     alignment line length\n"
                 "  -o [ --outprefix ] arg (=out)    output prefix\n"
                 "  -i [ --intersect ]               use only trace intersection for consensus\n"
                 "  -a [ --iupac ]                   use IUPAC nucleotide code in consensus (max. 2 nucleotides)\n"
                 "  --batch arg                      manifest: trace1<TAB>trace2<TAB>outprefix per line (all pairs on the GPU\n"
                 "                                   in blocks; the options above apply to every pair)\n\n";
    return -1;
  }
  if (!batch.empty()) {
    ConsBatchOptions o{co, linelimit, tl1, tr1, tl2, tr2, gapopen, gapext, match, mismatch, minOverlap, matchFraction, pratio, trimStringency, device};
    return consensus_batch(o, batch, argc, argv);
  }
  if (files.size() != 2) {
    std::cerr << "Exactly 2 input trace files are required!" << std::endl;
    return 1;
  }
  for (auto const& f : files)
    if (!regular_nonempty(f)) {
      std::cerr << "Input trace file is missing: " << file_name(f) << std::endl;
      return 1;
    }
  echo_command(argc, argv);
  Trace tr[2];
  BaseCalls bc[2];
  for (int k = 0; k < 2; ++k) {
    std::cout << stamp() << "Load " << files[k] << " file" << std::endl;
    if (!load_trace(files[k], tr[k])) return -1;
    if (tr[k].basecallpos.empty()) {
      std::cerr << "Trace file lacks basecalls!" << std::endl;
      return -1;
    }
  }
  for (int k = 0; k < 2; ++k) basecall(tr[k], bc[k], pratio);
  if (trimStringency >= 1) {
    uint32_t l = 0, r = 0;
    trimTrace(trimStringency, bc[0], l, r);
    tl1 = (uint16_t)l; tr1 = (uint16_t)r;
    l = 0; r = 0;
    trimTrace(trimStringency, bc[1], l, r);
    tl2 = (uint16_t)l; tr2 = (uint16_t)r;
  }
  if ((uint32_t)tl1 + tr1 >= bc[0].bcPos.size()) {
    std::cerr << "The sum of the left and right trim size is larger than the trace: " << files[0] << std::endl;
    return -1;
  }
  if ((uint32_t)tl2 + tr2 >= bc[1].bcPos.size()) {
    std::cerr << "The sum of the left and right trim size is larger than the trace:" << files[1] << std::endl;
    return -1;
  }
  traceTxtOut(outprefix + "_1st.abif", bc[0], tr[0], tl1, tr1);
  traceTxtOut(outprefix + "_2nd.abif", bc[1], tr[1], tl2, tr2);
  Profile trimmed1, fwd2, rev2;
  createProfile(tr[0], bc[0], trimmed1, tl1, tr1);
  createProfile(tr[1], bc[1], fwd2, tl2, tr2);
  reverseComplementProfile(fwd2, rev2);

  Device dev;
  if (tracyhip_create(device, &dev.ctx) != TRACYHIP_OK) {
    gpu_fail("no usable GPU");
    return -1;
  }
  tracyhip_params endfree{match, mismatch, gapopen, gapext, 1, 1};  // AlignConfig<true,true> ("global" in consensus.h:464)
  std::vector<int32_t> gs;
  {
    std::vector<Profile> a1(1, trimmed1), a2;
    a2.push_back(fwd2);
    a2.push_back(rev2);
    if (scorePairs(dev.ctx, endfree, a1, a2, std::vector<uint32_t>{0, 0}, std::vector<uint32_t>{0, 1}, gs) != TRACYHIP_OK)
      return gpu_fail("orientation scores"), -1;
  }
  const bool forward = gs[0] > gs[1];
  Profile const& trimmed2 = forward ? fwd2 : rev2;
  std::cout << stamp() << "Alignment" << std::endl;
  std::vector<int32_t> sc;
  std::vector<std::string> ops;
  {
    std::vector<Profile const*> a1(1, &trimmed1), a2(1, &trimmed2);
    if (!align_profiles(dev.ctx, endfree, a1, a2, sc, ops)) return -1;
  }
  AlignRows fali;
  fali.row0 = profile_row(trimmed1, ops[0], true);
  fali.row1 = profile_row(trimmed2, ops[0], false);
  uint32_t numAligned = 0, numMatch = 0;
  for (std::size_t j = 0; j < fali.cols(); ++j)
    if (fali.row0[j] != '-' && fali.row1[j] != '-') {
      ++numAligned;
      if (fali.row0[j] == fali.row1[j]) ++numMatch;
    }
  const double matchFrac = numAligned ? (double)numMatch / (double)numAligned : 0.0;
  if (numAligned < minOverlap || matchFrac < matchFraction) {
    std::cerr << "Error: No sufficient trace overlap!" << std::endl;
    return 1;
  }
  std::cout << stamp() << "Output" << std::endl;
  {
    std::ofstream v((outprefix + ".align.fa").c_str());
    v << ">" << stem(files[0]) << std::endl << fali.row0 << std::endl;
    v << ">" << stem(files[1]) << (forward ? " (forward)" : " (reverse)") << std::endl << fali.row1 << std::endl;
  }
  std::string cons;
  std::vector<uint32_t> qual;
  pairwiseConsensus(co, fali, trimmed1, trimmed2, cons, qual);
  {
    std::ofstream f((outprefix + ".fa").c_str());
    consensusFastaOut(f, co, cons);
  }
  {
    std::ofstream f((outprefix + ".fq").c_str());
    consensusFastqOut(f, co, cons, qual);
  }
  {
    std::ofstream f((outprefix + ".txt").c_str());
    plotClustalPairwise(f, fali, stem(files[0]), stem(files[1]), forward, sc[0], linelimit);
  }
  std::cout << stamp() << "Done." << std::endl;
  return 0;
}
