"""Host side of the device-built genome index (tracyhip_genome_build): a FASTA loaded without a table (tracyhost_genome_load), a table
taken over from elsewhere (tracyhost_genome_adopt -> view / save / count as after the in-memory build), the descriptor check of a build
(tracyhip_genome_validate_text, which needs no device) and the one bucket_bits rule host and device builds share
(tracyhost_default_bucket_bits)."""
import ctypes as C
import gzip

import numpy as np
import pytest


def rand_dna(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).tolist()).decode()


def write_fasta(path, contigs):
    with gzip.open(path, "wt") as f:
        for name, body in contigs:
            f.write(">%s\n" % name)
            for i in range(0, len(body), 60):
                f.write(body[i:i + 60] + "\n")


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    rng = np.random.default_rng(321)
    c1 = rand_dna(rng, 20000)
    c1 = c1[:4000] + "N" * 200 + c1[4000:9000] + "A" * 3000 + c1[9000:]
    c2 = rand_dna(rng, 6000).lower()
    contigs = [("chrA", c1), ("chrB text", c2), ("chrC", "ACGTNNACG"), ("chrA", rand_dna(rng, 3000))]
    path = str(tmp_path_factory.mktemp("idx") / "g.fa.gz")
    write_fasta(path, contigs)
    return path


def loaded(path):
    from tracy_amd import hostlib
    fn = hostlib.lib().tracyhost_genome_load
    fn.restype = C.c_void_p
    h = fn(path.encode())
    assert h
    g = hostlib.Genome.__new__(hostlib.Genome)
    g._h, g.kmer = C.c_void_p(h), 15
    return g


def test_load_has_text_but_no_table(fasta):
    from tracy_amd import hostlib
    g = loaded(fasta)
    assert not g.has_table()
    with pytest.raises(IOError):
        g.view()
    v = hostlib.GenomeView()
    assert hostlib.lib().tracyhost_genome_text(g._h, C.byref(v)) == 0
    assert v.ncontigs == 4 and v.ntab == 0 and not v.tab and not v.bkt
    ref = hostlib.Genome(fasta, 15, 2)
    rv = ref.view()
    text = np.ctypeslib.as_array(C.cast(v.text, C.POINTER(C.c_uint8)), shape=(v.text_len,))
    assert np.array_equal(text, rv["text"])
    assert g.contig_names() == ref.contig_names()


def test_load_refuses_an_index_file(fasta, tmp_path):
    from tracy_amd import hostlib
    ref = hostlib.Genome(fasta, 15, 2)
    ipath = str(tmp_path / "g.tidx")
    ref.save(ipath)
    fn = hostlib.lib().tracyhost_genome_load
    fn.restype = C.c_void_p
    assert not fn(ipath.encode())
    assert not fn(str(tmp_path / "missing.fa").encode())


@pytest.mark.parametrize("k", [1, 5, 15, 32])
def test_adopt_of_the_host_table_is_the_host_index(fasta, tmp_path, k):
    from tracy_amd import hostlib
    ref = hostlib.Genome(fasta, k, 2)
    rv = ref.view()
    g = loaded(fasta)
    g.kmer = k
    dirs, tab = rv["dir"].copy(), rv["tab"].copy()
    assert hostlib.lib().tracyhost_genome_adopt(g._h, C.c_uint32(k), C.c_uint32(rv["bucket_bits"]), C.c_void_p(dirs.ctypes.data),
                                                C.c_void_p(tab.ctypes.data), C.c_uint64(len(tab))) == 0
    del dirs, tab  # (adopt copies)
    v = g.view()
    for key in ("k", "bucket_bits", "ntab", "text_len", "ncontigs"):
        assert v[key] == rv[key], key
    for key in ("dir", "tab", "text", "starts", "lengths"):
        assert np.array_equal(v[key], rv[key]), key
    a, b = str(tmp_path / "adopted.tidx"), str(tmp_path / "built.tidx")
    g.save(a)
    ref.save(b)
    assert open(a, "rb").read() == open(b, "rb").read()
    pat = v["text"][100:100 + k].tobytes()
    assert g.count(pat) == ref.count(pat)


def test_adopt_refuses_what_is_not_a_table(fasta):
    from tracy_amd import hostlib
    ref = hostlib.Genome(fasta, 15, 2)
    rv = ref.view()
    g = loaded(fasta)
    adopt = hostlib.lib().tracyhost_genome_adopt
    d, t = rv["dir"].copy(), rv["tab"].copy()
    args = lambda k, bits, n: (g._h, C.c_uint32(k), C.c_uint32(bits), C.c_void_p(d.ctypes.data), C.c_void_p(t.ctypes.data), C.c_uint64(n))
    assert adopt(*args(15, rv["bucket_bits"], len(t) - 1)) != 0     # last directory entry is not ntab
    assert adopt(*args(0, rv["bucket_bits"], len(t))) != 0
    assert adopt(*args(15, 25, len(t))) != 0
    d[5], d[6] = d[6] + 1, d[6]                                      # not monotone
    assert adopt(*args(15, rv["bucket_bits"], len(t))) != 0
    assert not g.has_table()
    gi = hostlib.Genome(fasta, 15, 2)                                # an in-memory build holds its own table: adopt still works
    d = rv["dir"].copy()
    assert adopt(gi._h, C.c_uint32(15), C.c_uint32(rv["bucket_bits"]), C.c_void_p(d.ctypes.data), C.c_void_p(t.ctypes.data), C.c_uint64(len(t))) == 0


def text_desc(fasta, k, bits):
    from tracy_amd import capi, hostlib
    g = loaded(fasta)
    v = hostlib.GenomeView()
    assert hostlib.lib().tracyhost_genome_text(g._h, C.byref(v)) == 0
    starts = np.ctypeslib.as_array(C.cast(v.starts, C.POINTER(C.c_uint64)), shape=(v.ncontigs,)).copy()
    lengths = np.ctypeslib.as_array(C.cast(v.lengths, C.POINTER(C.c_uint32)), shape=(v.ncontigs,)).copy()
    d = capi.GenomeDesc()
    d.k, d.bucket_bits, d.dir, d.tab, d.ntab = k, bits, None, None, 0
    d.text, d.text_len, d.ncontigs = v.text, v.text_len, v.ncontigs
    d.starts, d.lengths = starts.ctypes.data, lengths.ctypes.data
    return g, d, starts, lengths, v


def test_validate_text_accepts_a_loaded_genome(fasta):
    from tracy_amd import capi
    for k, bits in [(1, 0), (1, 2), (7, 14), (12, 24), (15, 24), (15, 8), (32, 24)]:
        g, d, *_ = text_desc(fasta, k, bits)
        capi.genome_validate_text(d)
        cid = np.array([0, 1, 2, 0], dtype=np.uint32)
        d.contig_id = cid.ctypes.data
        capi.genome_validate_text(d)


@pytest.mark.parametrize("corruption", ["k_zero", "k_large", "bits_2k", "bits_24", "contig_outside", "contig_order", "contig_id",
                                        "dir", "tab", "ntab", "no_text", "no_contigs"])
def test_validate_text_rejects(fasta, corruption):
    from tracy_amd import capi
    k, bits = 15, 24
    if corruption == "k_zero":
        k, bits = 0, 0
    elif corruption == "k_large":
        k = 33
    elif corruption == "bits_2k":
        k, bits = 5, 11
    elif corruption == "bits_24":
        k, bits = 15, 25
    g, d, starts, lengths, v = text_desc(fasta, k, bits)
    keep = []
    if corruption == "contig_outside":
        lengths[3] = np.uint32(v.text_len)
    elif corruption == "contig_order":
        starts[1] = starts[0]
    elif corruption == "contig_id":
        cid = np.array([0, 1, 2, 4], dtype=np.uint32)
        keep.append(cid)
        d.contig_id = cid.ctypes.data
    elif corruption in ("dir", "tab"):
        arr = np.zeros(16, dtype=np.uint64)
        keep.append(arr)
        setattr(d, corruption, arr.ctypes.data)
    elif corruption == "ntab":
        d.ntab = 3
    elif corruption == "no_text":
        d.text = None
    elif corruption == "no_contigs":
        d.ncontigs = 0
    with pytest.raises(capi.TracyHipError) as e:
        capi.genome_validate_text(d)
    assert e.value.code == capi.ERR_ARG
    assert "tracyhip_genome_build" in str(e.value)


@pytest.mark.parametrize("knob", [None, "8", "12", "20", "24", "30", "4", "x"])
def test_default_bucket_bits_is_the_builds(fasta, monkeypatch, knob):
    from tracy_amd import hostlib
    if knob is None:
        monkeypatch.delenv("TRACY_AMD_SEED_BUCKET_BITS", raising=False)
    else:
        monkeypatch.setenv("TRACY_AMD_SEED_BUCKET_BITS", knob)
    for k in (1, 3, 5, 7, 12, 15, 32):
        g = hostlib.Genome(fasta, k, 2)
        assert g.view()["bucket_bits"] == hostlib.default_bucket_bits(k), (knob, k)
        g.close()
    if knob is None:
        assert [hostlib.default_bucket_bits(k) for k in (1, 5, 12, 13, 32)] == [2, 10, 24, 24, 24]


@pytest.mark.parametrize("bad", ["x", "-1", "1.5", ""])
def test_cli_index_device_option_is_checked(fasta, tmp_path, bad):
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tracy_amd", "bin", "tracy_amd_cli")
    out = str(tmp_path / "x.tidx")
    r = subprocess.run([cli, "index", "-d", bad, "-o", out, fasta], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--device" in r.stdout
    assert not os.path.exists(out)
