"""Device k-mer seeding (DeviceGenome, tracyhip_seed_traces) against host seeding (Genome.seed, tracyhost_seed_batch): every field of
every trace, window bytes included, over the shapes getReferenceSlice (fmindex.h:236-326) distinguishes -- both strands, substitutions,
N runs, lower-case FASTA, several contigs (one shorter than a window, one named twice), windows clipped at both ends of a contig,
repeats that only the second pass anchors, vote ties, palindromic k-mers, unanchorable traces, traces without windows, traces the
device defers to the host -- and seeding followed by extension with the windows kept on the device."""
import gzip

import numpy as np
import pytest

import sage_oracle as so

pytestmark = pytest.mark.gpu

FIELDS = ("status", "forward", "kmersupport", "pos", "contig", "slice_len")


def rand_dna(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n).tolist())


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from tracy_amd import hostlib
    rng = np.random.default_rng(123)
    rep = rand_dna(rng, 400)
    dup = rand_dna(rng, 300)
    c1 = rand_dna(rng, 30000)
    c1 = c1[:5000] + rep + c1[5000:12000] + "N" * 300 + c1[12000:20000] + rep + c1[20000:]   # a repeat + an N run
    c2 = rand_dna(rng, 9000)
    c2 = c2[:3000] + rep + c2[3000:6000] + dup + dup + c2[6000:7000] + "RYKM" + c2[7000:]      # tandem duplicate, IUPAC letters
    c3 = rand_dna(rng, 2500)                                                                    # shorter than a window
    c4 = rand_dna(rng, 5000)                                                                    # a second contig named chrA
    low = c2[:100].lower() + c2[100:]                                                           # lower case is upper-cased
    contigs = [("chrA", c1), ("chrB description", low), ("chrC", c3), ("chrA", c4), ("chrD", "ACGTACG")]
    d = tmp_path_factory.mktemp("seed_device")
    path = str(d / "toy.fa.gz")
    with gzip.open(path, "wt") as f:
        for name, body in contigs:
            f.write(">%s\n" % name)
            for i in range(0, len(body), 60):
                f.write(body[i:i + 60] + "\n")
    g = hostlib.Genome(path, 15, 4)
    ipath = str(d / "toy.tidx")
    g.save(ipath)
    gi = hostlib.Genome(ipath, 15, 4)
    seqs = [c1, c2, c3, c4]
    yield {"fasta": g, "tidx": gi}, seqs, rep, dup
    gi.close()
    g.close()


def mutate(rng, r, sub=0.01, nfrac=0.0):
    r = list(r)
    for k in range(len(r)):
        u = rng.random()
        if u < sub:
            r[k] = "ACGT"[int(rng.integers(0, 4))]
        elif u < sub + nfrac:
            r[k] = "N"
    return "".join(r)


def toy_reads(rng, seqs, rep, dup):
    reads = []
    for i in range(160):
        ci = int(rng.integers(0, len(seqs)))
        seq = seqs[ci].upper()
        L = min(int(rng.integers(150, 1200)), len(seq) - 1)
        start = int(rng.choice([0, len(seq) - L, rng.integers(0, len(seq) - L + 1)]))   # contig starts and ends
        r = mutate(rng, seq[start:start + L], 0.01, 0.01 if i % 3 == 0 else 0.0)
        if i % 7 == 0:
            r = rand_dna(rng, 40) + r                                                       # hangs over the contig's start
        if i % 2:
            r = so._revcomp_str(r)
        reads.append(r)
    reads.append(rep[20:380])                                                               # repeat: anchored by the second pass only
    reads.append(so._revcomp_str(rep[:390]))
    reads.append(dup[100:] + dup[:200])                                                     # across the tandem duplicate
    reads.append(dup[20:280])                                                               # inside it: two equally supported offsets
    reads.append(so._revcomp_str(dup[50:] + dup[:150]))
    reads.append("N" * 60 + seqs[1][6800:7600].upper() + "N" * 30)                         # N runs in the trace
    reads += [rand_dna(rng, 700) for _ in range(6)]                                         # unanchorable
    reads.append(rand_dna(rng, 80))                                                         # no window at trims 50 + 50
    reads.append(seqs[0][100:180])
    reads.append(seqs[0][2000:2600] + "R" + seqs[0][2601:3000])                             # IUPAC letter: deferred
    reads.append(seqs[0][4000:4500].lower())                                                # lower case: deferred
    reads.append(seqs[0][:20])                                                              # shorter than a trim: deferred
    return reads


def assert_same(got, want, n, where):
    for k in ("status", "slice_len"):
        assert np.array_equal(np.asarray(got[k][:n]), np.asarray(want[k][:n])), (where, k)
    ok = np.nonzero(np.asarray(want["status"][:n]) == 1)[0]
    for k in FIELDS:
        assert np.array_equal(np.asarray(got[k])[ok], np.asarray(want[k])[ok]), (where, k)
    if "slices" in want:
        for i in range(n):
            assert got["slices"][i] == want["slices"][i], (where, i)


@pytest.mark.parametrize("which", ["fasta", "tidx"])
@pytest.mark.parametrize("trims,support,maxindel", [((50, 50), 3, 1000), ((20, 30), 3, 500), ((14, 14), 2, 300), ((10, 5), 3, 200)])
def test_device_seed_equals_host(ctx, toy, which, trims, support, maxindel):
    gs, seqs, rep, dup = toy
    g = gs[which]
    dg = g.to_device(ctx)
    try:
        reads = [r.encode() for r in toy_reads(np.random.default_rng(5), seqs, rep, dup)]
        want = g.seed(reads, trims[0], trims[1], support, maxindel, 4)
        got = dg.seed(reads, trims[0], trims[1], support, maxindel, 4)
        assert_same(got, want, len(reads), (which, trims))
        st = np.asarray(want["status"])
        assert st.sum() > 100 and (st == 0).sum() >= 2
        if trims == (10, 5):
            assert got["n_deferred"] == len(reads)  # trims shorter than k - 1: the host's two scans
        else:
            assert got["n_deferred"] >= 2, got["n_deferred"]
        # the duplicate name reports the first contig; reverse windows are reverse-complemented
        assert set(np.asarray(got["contig"])[st == 1]) <= {0, 1, 2}
        assert (np.asarray(got["forward"])[st == 1] == 0).sum() > 20
    finally:
        dg.close()


def test_pass_one_and_ties(ctx, toy):
    """the repeat is anchored by the second pass (all hits below 1000 occurrences) at the smallest of its equally supported offsets"""
    gs, seqs, rep, dup = toy
    g = gs["fasta"]
    dg = g.to_device(ctx)
    reads = [rep[20:380].encode(), dup[20:280].encode(), so._revcomp_str(dup[30:290]).encode()]
    want = g.seed(reads, 20, 20, 3, 300, 2)
    got = dg.seed(reads, 20, 20, 3, 300, 2)
    assert_same(got, want, 3, "repeat/tie")
    assert got["n_deferred"] == 0 and list(got["status"]) == [1, 1, 1]
    dg.close()


def test_palindromes_even_k(ctx, tmp_path):
    from tracy_amd import hostlib
    rng = np.random.default_rng(12)
    body = rand_dna(rng, 20000)
    for at in range(500, 19000, 900):
        h = rand_dna(rng, 6)
        body = body[:at] + h + so._revcomp_str(h) + body[at + 12:]
    path = str(tmp_path / "pal.fa")
    with open(path, "w") as f:
        f.write(">chrP\n" + body + "\n")
    g = hostlib.Genome(path, 12, 2)
    dg = g.to_device(ctx)
    reads = []
    for i in range(60):
        st = int(rng.integers(0, len(body) - 400))
        r = mutate(rng, body[st:st + int(rng.integers(120, 380))])
        reads.append((so._revcomp_str(r) if i % 2 else r).encode())
    reads.append(("ACGTACGTACGT" * 10).encode())
    for trims in ((20, 20), (11, 30)):
        want = g.seed(reads, trims[0], trims[1], 3, 300, 2)
        got = dg.seed(reads, trims[0], trims[1], 3, 300, 2)
        assert_same(got, want, len(reads), trims)
        assert got["n_deferred"] == 0
    dg.close()
    g.close()


def test_vote_cap_defers_and_results_stay(ctx, toy):
    gs, seqs, rep, dup = toy
    g = gs["fasta"]
    dg = g.to_device(ctx)
    reads = [r.encode() for r in toy_reads(np.random.default_rng(9), seqs, rep, dup)]
    want = g.seed(reads, 50, 50, 3, 1000, 4)
    ctx.set_option("seed_vote_cap", 8)
    try:
        assert ctx.describe()["seed_vote_cap"] == "8"
        got = dg.seed(reads, 50, 50, 3, 1000, 4)
    finally:
        ctx.set_option("seed_vote_cap", 2048)
    assert_same(got, want, len(reads), "cap 8")
    assert got["n_deferred"] > 100
    dg.close()


def test_long_trace_is_deferred(ctx, toy):
    gs, seqs, rep, dup = toy
    g = gs["fasta"]
    dg = g.to_device(ctx)
    rng = np.random.default_rng(3)
    reads = [(rand_dna(rng, 65530 - 3000) + seqs[0][1000:4000].upper()).encode(), seqs[0][1000:2000].upper().encode()]
    want = g.seed(reads, 50, 50, 3, 1000, 2)
    got = dg.seed(reads, 50, 50, 3, 1000, 2)
    assert_same(got, want, 2, "long")
    assert got["n_deferred"] == 1 and list(want["status"]) == [1, 1]
    dg.close()


def test_device_memory_windows(ctx, toy):
    """mem = device: the windows in a torch tensor on the GPU, the same bytes as the host's"""
    import torch
    from tracy_amd import capi, hostlib
    gs, seqs, rep, dup = toy
    g = gs["tidx"]
    dg = g.to_device(ctx)
    reads = [r.encode() for r in toy_reads(np.random.default_rng(11), seqs, rep, dup)]
    packed = hostlib.Genome.pack_consensus(reads)
    want = g.seed_packed(packed, 50, 50, 3, 1000, 4)
    got = dg.seed_packed(packed, 50, 50, 3, 1000, 4, mem=capi.MEM_DEVICE)
    assert isinstance(got["slices_2d"], torch.Tensor) and got["slices_2d"].is_cuda
    assert got["n_deferred"] >= 2
    n = len(reads)
    for k in FIELDS:
        ok = want["status"][:n] == 1
        assert np.array_equal(got[k][:n][ok], want[k][:n][ok]), k
    assert np.array_equal(got["status"][:n], want["status"][:n])
    dev = got["slices_2d"].cpu().numpy()
    for i in range(n):
        L = int(want["slice_len"][i])
        assert dev[i, :L].tobytes() == want["slices_2d"][i, :L].tobytes(), i
    dg.close()


def c3_batch(nt, genome_mb, seed=22):
    """configs[3]-shaped: random genome, 1 kb traces, every other one from the reverse strand, 1 % substitutions"""
    rng = np.random.default_rng(seed)
    n = int(genome_mb * 1e6)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = rng.integers(0, 4, size=n, dtype=np.uint8)
    starts = rng.integers(0, n - 1000 - 50, size=nt)
    c = codes[starts[:, None] + np.arange(1000)[None, :]]
    odd = (np.arange(nt) % 2).astype(bool)
    c[odd] = (3 - c[odd])[:, ::-1]
    flip = rng.random(c.shape) < 0.01
    c = np.where(flip, (c + 1) % 4, c).astype(np.uint8)
    return lut[codes].tobytes(), c, [lut[r].tobytes() for r in c]


@pytest.fixture(scope="module")
def c3(tmp_path_factory):
    from tracy_amd import hostlib
    text, codes, reads = c3_batch(20000, 3.0)
    path = str(tmp_path_factory.mktemp("c3") / "c3.fa")
    with open(path, "wb") as f:
        f.write(b">chrSyn\n" + text + b"\n")
    g = hostlib.Genome(path, 15, 8)
    yield g, codes, reads
    g.close()


def test_configs3_batch_all_identical(ctx, c3):
    from tracy_amd import hostlib
    g, codes, reads = c3
    dg = g.to_device(ctx)
    packed = hostlib.Genome.pack_consensus(reads)
    want = g.seed_packed(packed, 50, 50, 3, 1000, 8)
    got = dg.seed_packed(packed, 50, 50, 3, 1000, 8)
    assert got["n_deferred"] == 0
    assert (want["status"] == 1).all()
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), k
    for i in range(len(reads)):
        L = int(want["slice_len"][i])
        assert got["slices_2d"][i, :L].tobytes() == want["slices_2d"][i, :L].tobytes(), i
    dg.close()


def test_seed_then_extend_on_device(ctx, c3):
    """tracyhip_align_traces with `oriented`, fed the windows device seeding left on the device (MEM_DEVICE), gives what the same
    call gives on host-seeded windows"""
    import ctypes as C
    import torch
    from tracy_amd import capi, hostlib
    g, codes, reads = c3
    nt = 300
    dg = g.to_device(ctx)
    packed = hostlib.Genome.pack_consensus(reads[:nt])
    hs = g.seed_packed(packed, 50, 50, 3, 1000, 8)
    ds = dg.seed_packed(packed, 50, 50, 3, 1000, 8, mem=capi.MEM_DEVICE)
    ok = np.nonzero(hs["status"][:nt] == 1)[0]
    assert len(ok) == nt and ds["n_deferred"] == 0
    prof = np.full((nt, 6, 1000), 0.0, np.float32)
    prof[:, :4, :] = 0.02
    for code in range(4):
        prof[:, code, :][codes[:nt] == code] = 0.94
    score = (3, -5, -10, -4)
    want = ctx.align_traces([prof[i] for i in ok], [hs["slices_2d"][i, :hs["slice_len"][i]].tobytes() for i in ok], score, 50, 50,
                            oriented=hs["forward"][ok])
    cap = ds["slices_2d"].shape[1]
    pp = capi.PackedSeqs([prof[i] for i in ok], capi.SEQ_PROFILE)
    pw = capi.PackedSeqs([], capi.SEQ_CHAR)
    pw.count = len(ok)
    pw.offset = ok.astype(np.uint64) * np.uint64(cap)
    pw.length = np.ascontiguousarray(ds["slice_len"][ok], dtype=np.uint32)
    p = capi.PreparedAlign(pp, pw, score, 50, 50, oriented=np.ascontiguousarray(ds["forward"][ok]))
    dprof = torch.from_numpy(pp.data).cuda()
    p.job.profiles = pp.seqset(dprof.data_ptr())
    p.job.refs = pw.seqset(ds["slices_2d"].data_ptr())
    dres = {k: torch.zeros(v.shape, dtype=torch.int32 if str(v.dtype) == "uint32" else getattr(torch, str(v.dtype)), device="cuda")
            for k, v in p.res.items()}
    for k, v in dres.items():
        setattr(p.out, k, v.data_ptr())
    torch.cuda.synchronize()
    capi._check(capi.lib().tracyhip_align_traces(ctx._h, C.byref(p.job), C.byref(p.prm), capi.MEM_DEVICE, C.byref(p.out)))
    torch.cuda.synchronize()
    for k, v in dres.items():
        p.res[k] = v.cpu().numpy().view(p.res[k].dtype)
    got = p.results()
    for k in ("score_fwd", "score_rev", "forward", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final"):
        assert np.array_equal(got[k], want[k]), k
    assert got["btr"] == want["btr"]
    dg.close()
