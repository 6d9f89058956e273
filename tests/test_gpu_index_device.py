"""The genome index built on the device (tracyhip_genome_build, Genome.from_fasta_on_device) against the host's in-memory build
(GenomeIndex::build): directory and table word for word over k = 1 .. 32, explicit bucket_bits, N runs, lower case, IUPAC letters, contigs
without a window, duplicate names, palindromes, a poly-A run and a tandem repeat that fill single buckets, a few Mb of random sequence;
seeding on the device-built index; `tracy_amd_cli index -d`; and a device genome without a host table."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import sage_oracle as so

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tracy_amd", "bin", "tracy_amd_cli")
FIELDS = ("status", "forward", "kmersupport", "pos", "contig", "slice_len")


def rand_dna(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n).tolist())


def write_fasta(path, contigs):
    with gzip.open(path, "wt") as f:
        for name, body in contigs:
            f.write(">%s\n" % name)
            for i in range(0, len(body), 60):
                f.write(body[i:i + 60] + "\n")
    return path


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """the FASTA files of the cases, written once"""
    d = tmp_path_factory.mktemp("index_device")
    rng = np.random.default_rng(123)
    # the seed tests' toy genome: a repeat, an N run, a tandem duplicate, IUPAC letters, lower case, a contig shorter than k, a name twice
    rep, dup = rand_dna(rng, 400), rand_dna(rng, 300)
    c1 = rand_dna(rng, 30000)
    c1 = c1[:5000] + rep + c1[5000:12000] + "N" * 300 + c1[12000:20000] + rep + c1[20000:]
    c2 = rand_dna(rng, 9000)
    c2 = c2[:3000] + rep + c2[3000:6000] + dup + dup + c2[6000:7000] + "RYKM" + c2[7000:]
    c3, c4 = rand_dna(rng, 2500), rand_dna(rng, 5000)
    toy = [("chrA", c1), ("chrB description", c2[:100].lower() + c2[100:]), ("chrC", c3), ("chrA", c4), ("chrD", "ACGTACG")]
    # contigs without a valid window: all N, shorter than k, every run of ACGT shorter than k; palindromes (x + revcomp(x)) for even k
    pal = "".join(p + so._revcomp_str(p) for p in (rand_dna(rng, int(rng.integers(1, 17))) for _ in range(2000)))
    empty = [("allN", "N" * 5000), ("short", "ACGTAC"), ("broken", "ACGTNACGTRACGTN" * 200), ("pal", pal),
             ("acgt", "ACGT" * 3000), ("tail", rand_dna(rng, 4000))]
    # repeats that put most of the table into a few buckets: 200 kb of poly-A, a 37-mer repeated 6000 times, a dinucleotide repeat
    unit = rand_dna(rng, 37)
    r1 = rand_dna(rng, 150000)
    repeats = [("r1", r1[:50000] + "A" * 200000 + r1[50000:100000] + unit * 6000 + r1[100000:] + "AC" * 20000), ("r2", "T" * 30000)]
    big = [("chr%d" % i, rand_dna(rng, n)) for i, n in enumerate((2000000, 1500000, 500000))]
    return dict(toy=write_fasta(str(d / "toy.fa.gz"), toy), empty=write_fasta(str(d / "empty.fa.gz"), empty),
                repeats=write_fasta(str(d / "repeats.fa.gz"), repeats), big=write_fasta(str(d / "big.fa.gz"), big),
                dir=d, toy_contigs=[c1, c2, c3, c4], rep=rep, dup=dup)


def host_view(path, k, nthreads):
    """the host build and its view (the view's arrays live as long as the Genome)"""
    from tracy_amd import hostlib
    g = hostlib.Genome(path, k, nthreads)
    return g, g.view()


def device_view(path, ctx, k, bits=None):
    from tracy_amd import hostlib
    g, dg = hostlib.Genome.from_fasta_on_device(path, ctx, kmer=k, bucket_bits=bits)
    v = g.view()
    dg.close()
    return g, v


def assert_same_index(got, want, where):
    for key in ("k", "bucket_bits", "ntab", "text_len", "ncontigs"):
        assert got[key] == want[key], (where, key, got[key], want[key])
    for key in ("dir", "tab", "text", "starts", "lengths"):
        assert np.array_equal(got[key], want[key]), (where, key)


def reference_index(text, k, bits):
    """an independent oracle of GenomeIndex::build's order, in numpy: (dir, tab)"""
    t = np.frombuffer(text, dtype=np.uint8)
    lut = np.full(256, 255, np.uint8)
    lut[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    c = lut[t]
    nwin = len(t) - k + 1
    bad = np.concatenate([[0], np.cumsum(c == 255)])
    ok = (bad[k:k + nwin] - bad[:nwin]) == 0
    p = np.nonzero(ok)[0]
    code = np.zeros(len(p), np.uint64)
    rc = np.zeros(len(p), np.uint64)
    for j in range(k):
        x = c[p + j].astype(np.uint64)
        code = (code << np.uint64(2)) | x
        rc = rc | ((np.uint64(3) - x) << np.uint64(2 * j))
    flip = rc < code
    key = np.where(flip, rc, code)
    pos = p.astype(np.uint64) | (flip.astype(np.uint64) << np.uint64(63))
    slot = key & np.uint64((1 << bits) - 1)
    o = np.lexsort((pos, key, slot))
    tab = np.stack([key[o], pos[o]], axis=1)
    d = np.zeros((1 << bits) + 1, np.uint64)
    np.add.at(d, slot.astype(np.int64) + 1, np.uint64(1))
    return np.cumsum(d).astype(np.uint64), tab


@pytest.mark.parametrize("k", [1, 2, 7, 12, 15, 31, 32])
def test_toy_genome_every_k(ctx, data, k):
    from tracy_amd import hostlib
    h, want = host_view(data["toy"], k, 4)
    g, got = device_view(data["toy"], ctx, k)
    assert_same_index(got, want, ("toy", k))


@pytest.mark.parametrize("k,bits", [(15, 12), (7, 10), (12, 24), (7, 14), (3, 6)])
def test_explicit_bucket_bits_against_the_host(ctx, data, monkeypatch, k, bits):
    from tracy_amd import hostlib
    monkeypatch.setenv("TRACY_AMD_SEED_BUCKET_BITS", str(max(bits, 8)))  # (the host's knob: 8 .. 24)
    h, want = host_view(data["toy"], k, 4)
    assert want["bucket_bits"] == bits
    g, got = device_view(data["toy"], ctx, k, bits)
    assert_same_index(got, want, (k, bits))


@pytest.mark.parametrize("k,bits", [(1, 0), (1, 1), (2, 2), (4, 5), (15, 3)])
def test_bucket_bits_below_the_knobs_range(ctx, data, k, bits):
    g, got = device_view(data["toy"], ctx, k, bits)
    d, tab = reference_index(got["text"].tobytes(), k, bits)
    assert got["bucket_bits"] == bits
    assert np.array_equal(got["dir"], d) and np.array_equal(got["tab"], tab)


@pytest.mark.parametrize("k", [4, 8, 15, 16])
def test_windowless_contigs_and_palindromes(ctx, data, k):
    from tracy_amd import hostlib
    h, want = host_view(data["empty"], k, 4)
    g, got = device_view(data["empty"], ctx, k)
    assert_same_index(got, want, ("empty", k))
    if k % 2 == 0:  # palindromic k-mers are there, and not flipped
        codes, pos = got["tab"][:, 0], got["tab"][:, 1]
        text = got["text"].tobytes()
        plain = (pos & np.uint64((1 << 63) - 1)).astype(np.int64)
        win = [text[q:q + k].decode() for q in plain]
        pal = np.array([w == so._revcomp_str(w) for w in win])
        assert pal.sum() > 100
        assert not np.any((pos >> np.uint64(63))[pal])


def test_a_genome_without_any_window(ctx, data):
    from tracy_amd import hostlib
    path = write_fasta(str(data["dir"] / "nowin.fa.gz"), [("a", "N" * 100), ("b", "ACGTN" * 50)])
    h, want = host_view(path, 15, 2)
    g, got = device_view(path, ctx, 15)
    assert got["ntab"] == 0
    assert_same_index(got, want, "nowin")


@pytest.mark.parametrize("k", [12, 15, 32])
def test_repeats_fill_single_buckets(ctx, data, k):
    from tracy_amd import hostlib
    h, want = host_view(data["repeats"], k, 8)
    assert int(np.diff(want["dir"]).max()) > 200000  # one bucket holds the poly-A / poly-T run
    g, got = device_view(data["repeats"], ctx, k)
    assert_same_index(got, want, ("repeats", k))


@pytest.mark.parametrize("k", [1, 2, 15])
def test_a_few_mb_of_random_sequence(ctx, data, k):
    from tracy_amd import hostlib
    h, want = host_view(data["big"], k, 8)
    g, got = device_view(data["big"], ctx, k)
    assert_same_index(got, want, ("big", k))


def toy_reads(rng, data):
    seqs, rep, dup = data["toy_contigs"], data["rep"], data["dup"]
    reads = []
    for i in range(120):
        seq = seqs[int(rng.integers(0, len(seqs)))].upper()
        L = min(int(rng.integers(150, 1200)), len(seq) - 1)
        start = int(rng.integers(0, len(seq) - L + 1))
        r = list(seq[start:start + L])
        for q in range(len(r)):
            if rng.random() < 0.01:
                r[q] = "ACGT"[int(rng.integers(0, 4))]
        r = "".join(r)
        reads.append(so._revcomp_str(r) if i % 2 else r)
    reads += [rep[20:380], dup[100:] + dup[:200], rand_dna(rng, 700), rand_dna(rng, 80)]
    return reads


def deferred_reads(data):
    s = data["toy_contigs"][0]
    return [s[2000:2600] + "R" + s[2601:3000], s[4000:4500].lower(), s[:20]]  # IUPAC letter, lower case, shorter than a trim


def test_seeding_on_the_device_built_index(ctx, data):
    from tracy_amd import hostlib
    host = hostlib.Genome(data["toy"], 15, 4)
    g, dg = hostlib.Genome.from_fasta_on_device(data["toy"], ctx, kmer=15)
    try:
        reads = [r.encode() for r in toy_reads(np.random.default_rng(5), data) + deferred_reads(data)]
        for trims, support, maxindel in [((50, 50), 3, 1000), ((14, 14), 2, 300)]:
            want = host.seed(reads, trims[0], trims[1], support, maxindel, 4)
            got = dg.seed(reads, trims[0], trims[1], support, maxindel, 4)
            assert got["n_deferred"] >= 3
            n = len(reads)
            for key in ("status", "slice_len"):
                assert np.array_equal(got[key], want[key]), key
            ok = np.nonzero(want["status"] == 1)[0]
            assert len(ok) > 100
            for key in FIELDS:
                assert np.array_equal(np.asarray(got[key])[ok], np.asarray(want[key])[ok]), key
            for i in range(n):
                assert got["slices"][i] == want["slices"][i], i
            # the copied-back table seeds on the host exactly as the host build does
            hg = g.seed(reads, trims[0], trims[1], support, maxindel, 4)
            for key in FIELDS:
                assert np.array_equal(hg[key], want[key]), key
    finally:
        dg.close()


def test_without_copy_back(ctx, data):
    from tracy_amd import hostlib
    host = hostlib.Genome(data["toy"], 15, 4)
    g, dg = hostlib.Genome.from_fasta_on_device(data["toy"], ctx, kmer=15, copy_back=False)
    try:
        assert not g.has_table()
        want = host.view()
        from tracy_amd import capi
        assert capi.genome_ntab(dg._h) == want["ntab"]
        d, t = capi.genome_download(dg._h, want["bucket_bits"])
        assert np.array_equal(d, want["dir"]) and np.array_equal(t, want["tab"])
        reads = [r.encode() for r in toy_reads(np.random.default_rng(9), data)]
        got = dg.seed(reads)
        ref = host.seed(reads)
        assert got["n_deferred"] == 0
        for key in ("status", "slice_len"):
            assert np.array_equal(got[key], ref[key]), key
        assert got["slices"] == ref["slices"]
        with pytest.raises(RuntimeError, match="copy_back"):
            dg.seed(reads + [r.encode() for r in deferred_reads(data)])
    finally:
        dg.close()


@pytest.mark.parametrize("k", [15, 5])
def test_cli_index_on_the_device_writes_the_same_file(data, tmp_path, k):
    a, b = str(tmp_path / "host.tidx"), str(tmp_path / "device.tidx")
    subprocess.run([CLI, "index", "-k", str(k), "-o", a, data["toy"]], check=True, capture_output=True, timeout=300)
    r = subprocess.run([CLI, "index", "-k", str(k), "-d", "0", "-o", b, data["toy"]], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert open(a, "rb").read() == open(b, "rb").read()
