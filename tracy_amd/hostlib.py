"""ctypes binding of the host-side C++ library (libtracy_host.so): basecalling, trace -> profile and the
seeded synthetic workloads.  These stages run on the host in the reference as well (abif.h, profile.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        p = os.path.join(_HERE, "lib", "libtracy_host.so")
        if not os.path.exists(p):
            raise ImportError("tracy_amd: %s is missing -- run `python tracy_amd/build.py`" % p)
        _LIB = C.CDLL(p)
        _LIB.tracyhost_basecall.restype = C.c_size_t
        _LIB.tracyhost_iupac.restype = C.c_char
    return _LIB


def basecall(trace, basecallpos, sigratio=0.33):
    trace = np.ascontiguousarray(trace, dtype=np.int32)
    pos = np.ascontiguousarray(basecallpos, dtype=np.int32)
    n = len(pos)
    pri = C.create_string_buffer(n + 1)
    sec = C.create_string_buffer(n + 1)
    con = C.create_string_buffer(n + 1)
    bc = np.zeros(max(n, 1), dtype=np.int32)
    k = lib().tracyhost_basecall(trace.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(trace.shape[1]),
                                 pos.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(n), C.c_float(sigratio), pri, sec,
                                 con, bc.ctypes.data_as(C.POINTER(C.c_int32)))
    return pri.raw[:k], sec.raw[:k], con.raw[:k], bc[:k].copy()


def create_profile(trace, bcpos, primary, secondary, trimleft=0, trimright=0):
    trace = np.ascontiguousarray(trace, dtype=np.int32)
    bcpos = np.ascontiguousarray(bcpos, dtype=np.int32)
    nbc = len(bcpos)
    out = np.zeros(6 * max(nbc, 1), dtype=np.float32)
    sz = lib().tracyhost_create_profile(trace.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(trace.shape[1]),
                                        bcpos.ctypes.data_as(C.POINTER(C.c_int32)), bytes(primary), bytes(secondary),
                                        C.c_size_t(nbc), int(trimleft), int(trimright),
                                        out.ctypes.data_as(C.POINTER(C.c_float)))
    return out[:6 * sz].reshape(6, sz).copy()


def synth_align(seed0, ntraces, n, mf, nthreads=0):
    """returns refs uint8 [ntraces][n], profiles float32 [ntraces][6][mf], reverse uint8 [ntraces]"""
    refs = np.zeros((ntraces, n), dtype=np.uint8)
    profs = np.zeros((ntraces, 6, mf), dtype=np.float32)
    rev = np.zeros(ntraces, dtype=np.uint8)
    lib().tracyhost_synth_align(C.c_uint64(seed0), C.c_uint32(ntraces), C.c_uint32(n), C.c_uint32(mf),
                                refs.ctypes.data_as(C.POINTER(C.c_uint8)), profs.ctypes.data_as(C.POINTER(C.c_float)),
                                rev.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint32(nthreads))
    return refs, profs, rev


def synth_decompose(seed, n, mf, maxlen=30, kind=0, frac1=0.6):
    """one synthetic heterozygous trace: returns ref (bytes), signal int32 [4][ns], basecallpos int32, indel"""
    ns = 12 * mf + 12
    ref = np.zeros(n, dtype=np.uint8)
    sig = np.zeros((4, ns), dtype=np.int32)
    pos = np.zeros(mf + 64, dtype=np.int32)
    indel = C.c_int32(0)
    lib().tracyhost_synth_decompose.restype = C.c_uint32
    npos = lib().tracyhost_synth_decompose(C.c_uint64(seed), C.c_uint32(n), C.c_uint32(mf), C.c_uint32(maxlen), int(kind),
                                           C.c_double(frac1), ref.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           sig.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(ns),
                                           pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(indel))
    return ref.tobytes(), sig, pos[:npos].copy(), indel.value


def synth_decompose_batch(seed0, nt, n, mf, nthreads=0, mix=0):
    """returns dict(refs [nt][n] u8, signal [nt][4][ns] i32, bcpos [nt][mf] i32, primary/secondary [nt][mf] u8,
    profiles [nt][6][mf] f32).  mix 0: 80 % het indels, 20 % SNVs only, forward strand.  mix 1 (BASELINE configs[2] as
    SURVEY.md 8d words it): 80 % het indel + het SNVs, 10 % homozygous indel only, 10 % no variant; odd traces read the
    reverse strand of their window."""
    ns = 12 * mf + 12
    out = dict(refs=np.zeros((nt, n), np.uint8), signal=np.zeros((nt, 4, ns), np.int32), bcpos=np.zeros((nt, mf), np.int32),
               primary=np.zeros((nt, mf), np.uint8), secondary=np.zeros((nt, mf), np.uint8),
               profiles=np.zeros((nt, 6, mf), np.float32))
    lib().tracyhost_synth_decompose_batch2(C.c_uint64(seed0), C.c_uint32(nt), C.c_uint32(n), C.c_uint32(mf),
                                           out["refs"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                           out["signal"].ctypes.data_as(C.POINTER(C.c_int32)),
                                           out["bcpos"].ctypes.data_as(C.POINTER(C.c_int32)),
                                           out["primary"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                           out["secondary"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                           out["profiles"].ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(nthreads), int(mix))
    return out


def basecall_qual(trace, basecallpos, sigratio=0.33):
    """basecall() including the estimated per-base qualities (abif.h:232-253)"""
    trace = np.ascontiguousarray(trace, dtype=np.int32)
    pos = np.ascontiguousarray(basecallpos, dtype=np.int32)
    n = len(pos)
    pri, sec, con = (C.create_string_buffer(n + 1) for _ in range(3))
    bc = np.zeros(max(n, 1), dtype=np.int32)
    q = np.zeros(max(n, 1), dtype=np.uint8)
    fn = lib().tracyhost_basecall_qual
    fn.restype = C.c_size_t
    k = fn(trace.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(trace.shape[1]), pos.ctypes.data_as(C.POINTER(C.c_int32)),
           C.c_size_t(n), C.c_float(sigratio), pri, sec, con, bc.ctypes.data_as(C.POINTER(C.c_int32)),
           q.ctypes.data_as(C.POINTER(C.c_uint8)))
    return pri.raw[:k], sec.raw[:k], con.raw[:k], bc[:k].copy(), q[:k].copy()


def basecall_batch(signal, basecallpos, sigratio=0.33, stringency=0.0, nthreads=0, want=True):
    """the host chain (basecall + qualities, trimTrace when stringency >= 1, createProfile) of a batch of equally shaped traces on
    `nthreads` threads: signal int32 [nt][4][ns], basecallpos int32 [nt][np].  Returns (seconds the slowest thread spent in the chain,
    dict of results or None when want is False)."""
    signal = np.ascontiguousarray(signal, dtype=np.int32)
    pos = np.ascontiguousarray(basecallpos, dtype=np.int32)
    nt, _, ns = signal.shape
    npos = pos.shape[1]
    res = None
    ptr = [None] * 7
    if want:
        res = dict(primary=np.zeros((nt, npos), np.uint8), secondary=np.zeros((nt, npos), np.uint8), bcpos=np.zeros((nt, npos), np.int32),
                   estqual=np.zeros((nt, npos), np.uint8), profiles=np.zeros((nt, 6 * npos), np.float32), bc_len=np.zeros(nt, np.uint32),
                   trims=np.zeros((nt, 2), np.uint32))
        ptr = [C.c_void_p(res[k].ctypes.data) for k in ("primary", "secondary", "bcpos", "estqual", "profiles", "bc_len", "trims")]
    fn = lib().tracyhost_basecall_batch
    fn.restype = C.c_double
    secs = fn(C.c_void_p(signal.ctypes.data), C.c_uint32(nt), C.c_uint32(ns), C.c_void_p(pos.ctypes.data), C.c_uint32(npos), C.c_float(sigratio),
              C.c_float(stringency), C.c_uint32(nthreads), *ptr)
    return secs, res


def _read_trace_with(l, prefix, path, with_format):
    rd = getattr(l, prefix + "trace_read")
    rd.restype = C.c_void_p
    fmt = C.c_int32(-1)
    h = rd(os.fsencode(path), C.byref(fmt)) if with_format else rd(os.fsencode(path))
    if not h:
        return None
    h = C.c_void_p(h)
    try:
        ns, nc = C.c_uint64(0), C.c_uint64(0)
        getattr(l, prefix + "trace_dims")(h, C.byref(ns), C.byref(nc))
        sig = np.zeros((4, max(ns.value, 1)), dtype=np.int32)
        pos = np.zeros(max(nc.value, 1), dtype=np.int32)
        b1, b2 = C.create_string_buffer(nc.value + 1), C.create_string_buffer(nc.value + 1)
        q = np.zeros(max(nc.value, 1), dtype=np.uint8)
        getattr(l, prefix + "trace_get")(h, sig.ctypes.data_as(C.POINTER(C.c_int32)), pos.ctypes.data_as(C.POINTER(C.c_int32)), b1, b2,
                                         q.ctypes.data_as(C.POINTER(C.c_uint8)))
        return dict(format=fmt.value, signal=sig[:, :ns.value].copy(), basecallpos=pos[:nc.value].copy(), basecalls1=b1.raw[:nc.value],
                    basecalls2=b2.raw[:nc.value], qual=q[:nc.value].copy())
    finally:
        getattr(l, prefix + "trace_free")(h)


def read_trace(path):
    """ABIF (readab, abif.h:286-405) or SCF (readscf, scf.h:38-102) chromatogram -> dict, None when unreadable"""
    return _read_trace_with(lib(), "tracyhost_", path, True)


def write_abif(path, signal, peaks, primary, qual, secondary=b"", order=b"GATC"):
    """the build's own ABIF writer: signal int32 [4][ns] in A,C,G,T order"""
    signal = np.ascontiguousarray(signal, dtype=np.int32)
    peaks = np.ascontiguousarray(peaks, dtype=np.int32)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    rc = lib().tracyhost_writeab(os.fsencode(path), signal.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(signal.shape[1]),
                                 peaks.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(peaks)), bytes(primary),
                                 C.c_size_t(len(primary)), qual.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(len(qual)),
                                 bytes(secondary) if secondary else None, C.c_size_t(len(secondary)), bytes(order))
    if rc != 0:
        raise IOError("tracy_amd: cannot write %s" % path)


def trace_txt(outfile, trace, basecallpos, sigratio=0.33, left_trim=0, right_trim=0):
    """basecall + traceTxtOut (abif.h:513-533)"""
    trace = np.ascontiguousarray(trace, dtype=np.int32)
    pos = np.ascontiguousarray(basecallpos, dtype=np.int32)
    return lib().tracyhost_trace_txt(os.fsencode(outfile), trace.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(trace.shape[1]),
                                     pos.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(pos)), C.c_float(sigratio),
                                     C.c_uint32(left_trim), C.c_uint32(right_trim))


def align_outputs(prefix, trace_stem, trace, basecallpos, sigratio, row0, row1, chrom, refslice, pos, forward, score, linelimit=60):
    """writes <prefix>.align.fa / .txt / .json exactly as `tracy align` does (sage.h:313-345)"""
    trace = np.ascontiguousarray(trace, dtype=np.int32)
    bp = np.ascontiguousarray(basecallpos, dtype=np.int32)
    return lib().tracyhost_align_outputs(os.fsencode(prefix), trace_stem.encode(), trace.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.c_size_t(trace.shape[1]), bp.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(len(bp)),
                                         C.c_float(sigratio), bytes(row0), bytes(row1), C.c_size_t(len(row0)), chrom.encode(),
                                         bytes(refslice), C.c_size_t(len(refslice)), C.c_uint32(pos), int(bool(forward)), int(score),
                                         C.c_uint32(linelimit))


def trim_trace(trace, basecallpos, sigratio, stringency):
    trace = np.ascontiguousarray(trace, dtype=np.int32)
    bp = np.ascontiguousarray(basecallpos, dtype=np.int32)
    l, r = C.c_uint32(0), C.c_uint32(0)
    lib().tracyhost_trim_trace(trace.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(trace.shape[1]), bp.ctypes.data_as(C.POINTER(C.c_int32)),
                               C.c_size_t(len(bp)), C.c_float(sigratio), C.c_float(stringency), C.byref(l), C.byref(r))
    return l.value, r.value


def load_fasta(path):
    """loadSingleFasta (fasta.h:54-95) -> (name, seq) or None"""
    name = C.create_string_buffer(4096)
    cap = os.path.getsize(path) + 16
    seq = C.create_string_buffer(cap)
    fn = lib().tracyhost_load_fasta
    fn.restype = C.c_int64
    n = fn(os.fsencode(path), name, C.c_size_t(4096), seq, C.c_size_t(cap))
    if n < 0:
        return None
    return name.value.decode("latin1"), seq.raw[:n].decode()


class DecomposeReport(C.Structure):
    _fields_ = [("prefix", C.c_char_p), ("genome_name", C.c_char_p), ("input_name", C.c_char_p), ("trace", C.POINTER(C.c_int32)),
                ("nsamples", C.c_uint64), ("basecallpos", C.POINTER(C.c_int32)), ("npos", C.c_uint64), ("pratio", C.c_float),
                ("trim_left", C.c_uint32), ("trim_right", C.c_uint32), ("qual_cut", C.c_uint32), ("linelimit", C.c_uint32),
                ("primary", C.c_char_p), ("secondary", C.c_char_p), ("secdecomp", C.c_char_p), ("ncalls", C.c_uint64),
                ("rows", (C.c_char_p * 2) * 3), ("cols", C.c_uint64 * 3), ("var_rows", (C.c_char_p * 2) * 2), ("var_cols", C.c_uint64 * 2),
                ("call_variants", C.c_int32), ("chr", C.c_char_p), ("forward", C.c_int32), ("pos", C.c_uint32 * 2),
                ("slice_len", C.c_uint64 * 2), ("ref_len", C.c_uint64), ("score", C.c_int32 * 3), ("indelshift", C.c_int32),
                ("breakpoint", C.c_uint32), ("a1", C.c_double), ("a2", C.c_double), ("dcp_indel", C.POINTER(C.c_int32)),
                ("dcp_err", C.POINTER(C.c_int32)), ("dcp_n", C.c_uint64)]


def decompose_outputs(prefix, genome_name, input_name, trace, basecallpos, pratio, trims, qual_cut, linelimit, primary, secondary, secdecomp,
                      rows, var_rows, chrom, forward, pos, slice_len, ref_len, scores, indelshift, breakpoint, a1a2, dcp):
    """writes the files of `tracy decompose` (indigo.h:340-442); rows: 3 x (row0, row1); var_rows: None or 2 x (row0, row1)"""
    trace = np.ascontiguousarray(trace, dtype=np.int32)
    bp = np.ascontiguousarray(basecallpos, dtype=np.int32)
    di = np.array([a for a, _ in dcp], dtype=np.int32)
    de = np.array([b for _, b in dcp], dtype=np.int32)
    r = DecomposeReport()
    r.prefix, r.genome_name, r.input_name, r.chr = os.fsencode(prefix), genome_name.encode(), input_name.encode(), chrom.encode()
    r.trace, r.nsamples = trace.ctypes.data_as(C.POINTER(C.c_int32)), trace.shape[1]
    r.basecallpos, r.npos, r.pratio = bp.ctypes.data_as(C.POINTER(C.c_int32)), len(bp), pratio
    r.trim_left, r.trim_right, r.qual_cut, r.linelimit = trims[0], trims[1], qual_cut, linelimit
    r.primary, r.secondary, r.secdecomp, r.ncalls = bytes(primary), bytes(secondary), bytes(secdecomp), len(primary)
    for k in range(3):
        r.rows[k][0], r.rows[k][1], r.cols[k] = bytes(rows[k][0]), bytes(rows[k][1]), len(rows[k][0])
    r.call_variants = 1 if var_rows else 0
    if var_rows:
        for k in range(2):
            r.var_rows[k][0], r.var_rows[k][1], r.var_cols[k] = bytes(var_rows[k][0]), bytes(var_rows[k][1]), len(var_rows[k][0])
    r.forward, r.ref_len, r.indelshift, r.breakpoint = int(bool(forward)), ref_len, int(bool(indelshift)), breakpoint
    for k in range(2):
        r.pos[k], r.slice_len[k] = pos[k], slice_len[k]
    for k in range(3):
        r.score[k] = scores[k]
    r.a1, r.a2 = a1a2
    r.dcp_indel, r.dcp_err, r.dcp_n = di.ctypes.data_as(C.POINTER(C.c_int32)), de.ctypes.data_as(C.POINTER(C.c_int32)), len(dcp)
    return lib().tracyhost_decompose_outputs(C.byref(r))


class GenomeView(C.Structure):  # tracyhost_genome_view_t (tracy_host_capi.cpp)
    _fields_ = [("k", C.c_uint32), ("bucket_bits", C.c_uint32), ("bkt", C.c_void_p), ("tab", C.c_void_p), ("ntab", C.c_uint64),
                ("text", C.c_void_p), ("text_len", C.c_uint64), ("starts", C.c_void_p), ("lengths", C.c_void_p), ("ncontigs", C.c_uint32)]


def genome_desc(view, contig_id=None):
    """a tracyhip_genome_desc over the arrays of a view dict (Genome.view(), or arrays of one's own: a test may corrupt them)"""
    from . import capi
    d = capi.GenomeDesc()
    d.k, d.bucket_bits, d.ntab, d.text_len, d.ncontigs = view["k"], view["bucket_bits"], view["ntab"], view["text_len"], view["ncontigs"]
    d.dir, d.tab, d.text = view["dir"].ctypes.data, view["tab"].ctypes.data, view["text"].ctypes.data
    d.starts, d.lengths = view["starts"].ctypes.data, view["lengths"].ctypes.data
    d.contig_id = contig_id.ctypes.data if contig_id is not None else None
    return d


def default_bucket_bits(kmer):
    """tracyhost_default_bucket_bits: the directory size an in-memory build picks for k (min(2k, 24) or the TRACY_AMD_SEED_BUCKET_BITS knob)"""
    return int(lib().tracyhost_default_bucket_bits(C.c_uint32(kmer)))


def _contig_ids(names):
    first = {}
    return np.array([first.setdefault(nm, i) for i, nm in enumerate(names)], dtype=np.uint32)  # duplicate names: the first contig


class Genome:
    """indexed genome for k-mer seeding (tracy_amd/host/seed.hpp): plain or gzip-compressed multi-FASTA (table built in memory), or an
    index file written by save() / `tracy_amd_cli index` (mapped read-only; ranks of one node share the page cache's copy)"""

    def __init__(self, path, kmer=15, nthreads=0):
        self._h = None
        fn = lib().tracyhost_genome_open
        fn.restype = C.c_void_p
        h = fn(os.fsencode(path), C.c_uint32(kmer), C.c_uint32(nthreads))
        if not h:
            raise IOError("tracy_amd: cannot read genome %s" % path)
        self._h = C.c_void_p(h)
        self.kmer = kmer

    @classmethod
    def from_fasta_on_device(cls, path, ctx, kmer=15, bucket_bits=None, copy_back=True):
        """the index built on the device of `ctx` (tracyhip_genome_build) from a plain or gzip-compressed multi-FASTA -> (Genome, DeviceGenome).
        The Genome holds the text; with copy_back it also holds the device-built table (tracyhip_genome_download + tracyhost_genome_adopt:
        word for word the table Genome(path, kmer) builds), so save(), view() and host seeding work and DeviceGenome seeds DEFERRED traces
        on the host as usual.  Without copy_back the Genome has no table and DeviceGenome.seed raises on a deferred trace: one with
        letters other than ACGTN, a trim shorter than k - 1, |consensus| + k >= 65536 -- and one whose vote lists exceed the context's
        seed_vote_cap (a read inside a gene family or repeat, a read of more than ~2 100 windows) unless the context runs with
        set_option("seed_spill", 1), which answers those on the device.
        bucket_bits: None = the host build's choice (tracyhost_default_bucket_bits)."""
        from . import capi
        fn = lib().tracyhost_genome_load
        fn.restype = C.c_void_p
        h = fn(os.fsencode(path))
        if not h:
            raise IOError("tracy_amd: cannot read genome %s (a FASTA file, not an index)" % path)
        g = cls.__new__(cls)
        g._h, g.kmer = C.c_void_p(h), kmer
        bits = default_bucket_bits(kmer) if bucket_bits is None else int(bucket_bits)
        v = GenomeView()
        if lib().tracyhost_genome_text(g._h, C.byref(v)) != 0:
            raise IOError("tracy_amd: genome %s has no text" % path)
        d = capi.GenomeDesc()
        d.k, d.bucket_bits, d.dir, d.tab, d.ntab = kmer, bits, None, None, 0
        d.text, d.text_len, d.starts, d.lengths, d.ncontigs = v.text, v.text_len, v.starts, v.lengths, v.ncontigs
        cid = _contig_ids(g.contig_names())
        d.contig_id = cid.ctypes.data
        dh = capi.genome_build(ctx, d)
        try:
            if copy_back:
                dirs, tab = capi.genome_download(dh, bits)
                if lib().tracyhost_genome_adopt(g._h, C.c_uint32(kmer), C.c_uint32(bits), C.c_void_p(dirs.ctypes.data),
                                                C.c_void_p(tab.ctypes.data if tab.size else 0), C.c_uint64(len(tab))) != 0:
                    raise IOError("tracy_amd: the device-built table was refused")
        except Exception:
            capi.genome_free(dh)
            raise
        return g, DeviceGenome.wrap(g, ctx, dh, host_table=copy_back)

    def has_table(self):
        v = GenomeView()
        return lib().tracyhost_genome_view(self._h, C.byref(v)) == 0

    def close(self):
        if self._h:
            lib().tracyhost_genome_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def save(self, path):
        """write the index (text, contigs, sorted k-mer table) to one file that Genome(path) maps read-only: `tracy index`, index.h:79-124"""
        if lib().tracyhost_genome_save(self._h, os.fsencode(path)) != 0:
            raise IOError("tracy_amd: cannot write index %s" % path)

    def count(self, pattern):
        fn = lib().tracyhost_genome_count
        fn.restype = C.c_uint64
        return int(fn(self._h, bytes(pattern), C.c_size_t(len(pattern))))

    @staticmethod
    def pack_consensus(consensus):
        """the batch as a C caller holds it: one byte block, offsets, lengths (seed_packed takes these; packing a list of Python
        strings is interpreter work, not part of the seeding stage)"""
        n = len(consensus)
        lens = np.array([len(c) for c in consensus], dtype=np.uint32)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        if n:
            offs[1:n] = np.cumsum(lens.astype(np.uint64))[:-1]
        return dict(n=n, blob=b"".join(bytes(c) for c in consensus) + b"\0", offs=offs, lens=lens)

    def seed_packed(self, packed, trim_left=50, trim_right=50, min_support=3, maxindel=1000, nthreads=0, out=None):
        """getReferenceSlice for a packed batch (pack_consensus); `out`: the dict a previous call returned, reused as the result
        buffers of this one (same batch shape) -- what a caller that seeds block after block does.  Returns the raw form of seed()."""
        n = packed["n"]
        cap = int(packed["lens"].max() if n else 0) + 2 * maxindel + 2
        if out is None or out["slices_2d"].shape != (max(n, 1), cap):
            out = dict(status=np.zeros(max(n, 1), np.int32), forward=np.zeros(max(n, 1), np.uint8), kmersupport=np.zeros(max(n, 1), np.uint32),
                       pos=np.zeros(max(n, 1), np.uint32), contig=np.zeros(max(n, 1), np.uint32), slice_len=np.zeros(max(n, 1), np.uint32),
                       slices_2d=np.zeros((max(n, 1), cap), dtype=np.uint8))
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        lib().tracyhost_seed_batch(self._h, C.c_uint32(n), packed["blob"], p(packed["offs"], C.c_uint64), p(packed["lens"], C.c_uint32), C.c_uint32(trim_left),
                                   C.c_uint32(trim_right), C.c_uint32(self.kmer), C.c_uint32(min_support), C.c_uint32(maxindel),
                                   C.c_uint32(nthreads), p(out["status"], C.c_int32), p(out["forward"], C.c_uint8),
                                   p(out["kmersupport"], C.c_uint32), p(out["pos"], C.c_uint32), p(out["contig"], C.c_uint32),
                                   out["slices_2d"].ctypes.data_as(C.c_char_p), C.c_uint64(cap), p(out["slice_len"], C.c_uint32))
        return out

    def view(self):
        """the index's arrays (tracyhost_genome_view; valid while this Genome is open) as a dict: k, bucket_bits, ncontigs, ntab,
        text_len and numpy views dir (uint64 [2^bits + 1]), tab (uint64 [ntab][2]: code, pos with bit 63 the strand part), text
        (uint8), starts (uint64), lengths (uint32)"""
        v = GenomeView()
        if lib().tracyhost_genome_view(self._h, C.byref(v)) != 0:
            raise IOError("tracy_amd: the genome has no k-mer table")

        def arr(ptr, ty, n):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ty)), shape=(int(n),)) if n else np.zeros(0, dtype=np.dtype(ty))
        nb = (1 << v.bucket_bits) + 1
        return dict(k=int(v.k), bucket_bits=int(v.bucket_bits), ncontigs=int(v.ncontigs), ntab=int(v.ntab), text_len=int(v.text_len),
                    dir=arr(v.bkt, C.c_uint64, nb), tab=arr(v.tab, C.c_uint64, 2 * v.ntab).reshape(-1, 2),
                    text=arr(v.text, C.c_uint8, v.text_len), starts=arr(v.starts, C.c_uint64, v.ncontigs),
                    lengths=arr(v.lengths, C.c_uint32, v.ncontigs), _raw=v)

    def contig_names(self):
        fn = lib().tracyhost_genome_contig_name
        fn.restype = C.c_char_p
        return [fn(self._h, C.c_uint32(i)).decode() for i in range(lib().tracyhost_genome_contigs(self._h))]

    def to_device(self, ctx):
        """the index copied once to the device of `ctx` (tracyhip_genome_upload) -> DeviceGenome, whose seed() / seed_packed() answer
        like this Genome's"""
        return DeviceGenome(self, ctx)

    def seed(self, consensus, trim_left=50, trim_right=50, min_support=3, maxindel=1000, nthreads=0, raw=False):
        """getReferenceSlice (fmindex.h:236-326) for a list of consensus strings -> dict of arrays + oriented windows
        (`slices`: list of bytes; raw=True: `slices_2d` uint8 [n][cap] + `slice_len` instead, no per-trace copies)"""
        n = len(consensus)
        lens = np.array([len(c) for c in consensus], dtype=np.uint32)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        if n:
            offs[1:n] = np.cumsum(lens.astype(np.uint64))[:-1]
        blob = b"".join(bytes(c) for c in consensus) + b"\0"
        cap = int(lens.max() if n else 0) + 2 * maxindel + 2
        out = dict(status=np.zeros(max(n, 1), np.int32), forward=np.zeros(max(n, 1), np.uint8), kmersupport=np.zeros(max(n, 1), np.uint32),
                   pos=np.zeros(max(n, 1), np.uint32), contig=np.zeros(max(n, 1), np.uint32), slice_len=np.zeros(max(n, 1), np.uint32))
        slices = np.zeros((max(n, 1), cap), dtype=np.uint8)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        lib().tracyhost_seed_batch(self._h, C.c_uint32(n), blob, p(offs, C.c_uint64), p(lens, C.c_uint32), C.c_uint32(trim_left),
                                   C.c_uint32(trim_right), C.c_uint32(self.kmer), C.c_uint32(min_support), C.c_uint32(maxindel),
                                   C.c_uint32(nthreads), p(out["status"], C.c_int32), p(out["forward"], C.c_uint8),
                                   p(out["kmersupport"], C.c_uint32), p(out["pos"], C.c_uint32), p(out["contig"], C.c_uint32),
                                   slices.ctypes.data_as(C.c_char_p), C.c_uint64(cap), p(out["slice_len"], C.c_uint32))
        out = {k: v[:n] for k, v in out.items()}
        if raw:
            out["slices_2d"] = slices
        else:
            out["slices"] = [slices[i, :out["slice_len"][i]].tobytes() for i in range(n)]
        return out


class DeviceGenome:
    """a Genome's index on one device (tracyhip_genome_upload): getReferenceSlice for batches of traces by tracyhip_seed_traces.  seed() /
    seed_packed() return what Genome.seed() / seed_packed() return, plus n_deferred: the traces outside what the device answers
    (TRACYHIP_SEED_DEFERRED: letters other than ACGTN, short trims, long traces, and -- unless the context's option seed_spill is on --
    vote lists over its seed_vote_cap), which are seeded on the host (tracyhost_seed_batch) and merged in; and n_spilled: the traces over
    seed_vote_cap that the spill launch answered on the device (seed_spill on; 0 otherwise)."""

    def __init__(self, genome, ctx):
        from . import capi
        self._h = None
        self.genome, self.ctx, self.kmer = genome, ctx, genome.kmer
        v = genome.view()
        self._h = capi.genome_upload(ctx, genome_desc(v, _contig_ids(genome.contig_names())))
        self.bytes = capi.genome_bytes(self._h)
        self.host_table = True

    @classmethod
    def wrap(cls, genome, ctx, handle, host_table=True):
        """a DeviceGenome over an existing device handle (tracyhip_genome_build / _upload), which it then owns and frees.  host_table: whether
        `genome` holds the same table, for the host seeding of DEFERRED traces (False: seed() raises on a deferred trace)"""
        from . import capi
        self = cls.__new__(cls)
        self._h = handle
        self.genome, self.ctx, self.kmer = genome, ctx, genome.kmer
        self.bytes = capi.genome_bytes(handle)
        self.host_table = bool(host_table)
        return self

    def close(self):
        if self._h:
            from . import capi
            capi.genome_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def seed_packed(self, packed, trim_left=50, trim_right=50, min_support=3, maxindel=1000, nthreads=0, out=None, mem=None):
        """getReferenceSlice for a packed batch (Genome.pack_consensus) on the device.  mem = capi.MEM_HOST (default): slices_2d is a
        numpy array as from Genome.seed_packed; capi.MEM_DEVICE: the consensus goes to the device once per call and slices_2d is a torch
        uint8 tensor on it (the windows stay there, e.g. for align_traces with MEM_DEVICE).  `out`: a previous call's dict, reused."""
        from . import capi
        mem = capi.MEM_HOST if mem is None else mem
        n = packed["n"]
        nn = max(n, 1)
        cap = int(packed["lens"].max() if n else 0) + 2 * maxindel + 2
        if out is None or tuple(out["slices_2d"].shape) != (nn, cap):
            out = dict(status=np.zeros(nn, np.int32), forward=np.zeros(nn, np.uint8), kmersupport=np.zeros(nn, np.uint32),
                       pos=np.zeros(nn, np.uint32), contig=np.zeros(nn, np.uint32), slice_len=np.zeros(nn, np.uint32))
            if mem == capi.MEM_DEVICE:
                import torch
                out["slices_2d"] = torch.zeros((nn, cap), dtype=torch.uint8, device="cuda:%d" % torch.cuda.current_device())
            else:
                out["slices_2d"] = np.zeros((nn, cap), dtype=np.uint8)
        blob = packed["blob"]
        if mem == capi.MEM_DEVICE:
            import torch
            import warnings
            with warnings.catch_warnings():  # (read only: the bytes object is not written through the view)
                warnings.simplefilter("ignore")
                dblob = torch.frombuffer(blob, dtype=torch.uint8).to(out["slices_2d"].device)
            data, slices = dblob.data_ptr(), out["slices_2d"].data_ptr()
            torch.cuda.synchronize()
        else:
            data, slices = C.cast(C.c_char_p(blob), C.c_void_p).value, out["slices_2d"].ctypes.data
        ss = capi.SeqSet()
        ss.kind, ss.data, ss.count = capi.SEQ_CHAR, data, n
        ss.offset = packed["offs"].ctypes.data_as(C.POINTER(C.c_uint64))
        ss.length = packed["lens"].ctypes.data_as(C.POINTER(C.c_uint32))
        prm = capi.SeedParams(0, 0, self.kmer, min_support, maxindel)
        trim_arrays = capi.trims_each(prm, trim_left, trim_right, n)  # ints, or per-trace array-likes (kept alive over the call)
        r = capi.SeedResult()
        for k in ("status", "forward", "kmersupport", "pos", "contig", "slice_len"):
            setattr(r, k, out[k].ctypes.data)
        r.slices, r.slice_cap = slices, cap
        capi.seed_traces(self.ctx, self._h, ss, prm, mem, r)
        dfr = np.nonzero(out["status"][:n] == capi.SEED_DEFERRED)[0]
        out["n_deferred"] = int(len(dfr))
        out["n_spilled"] = int(self.ctx.last_call_stats()["seed_spilled"])
        if len(dfr) and not self.host_table:
            raise RuntimeError("tracy_amd: %d trace(s) deferred to host seeding, but the genome was built on the device without "
                               "copy_back: there is no host table to seed them with" % len(dfr))
        # the host's answer for exactly those traces; with per-trace trims the host, which takes one pair per call, seeds them pair by pair
        pair_of = (lambda i: (int(trim_arrays[0][i]) & 0xFFFF, int(trim_arrays[1][i]) & 0xFFFF)) if trim_arrays else (lambda i: (trim_left, trim_right))
        for (tl, tr) in sorted({pair_of(i) for i in dfr}):
            sel = np.array([i for i in dfr if pair_of(i) == (tl, tr)], dtype=dfr.dtype)
            sub = Genome.pack_consensus([blob[int(packed["offs"][i]):int(packed["offs"][i]) + int(packed["lens"][i])] for i in sel])
            h = self.genome.seed_packed(sub, tl, tr, min_support, maxindel, nthreads)
            hs = h["slices_2d"]
            if hs.shape[1] < cap:
                hs = np.pad(hs, ((0, 0), (0, cap - hs.shape[1])))
            for k in ("status", "slice_len"):
                out[k][sel] = h[k][:len(sel)]
            ok = h["status"][:len(sel)] == 1
            for k in ("forward", "kmersupport", "pos", "contig"):
                out[k][sel[ok]] = h[k][:len(sel)][ok]
            if mem == capi.MEM_DEVICE:
                import torch
                idx = torch.from_numpy(sel.astype(np.int64)).to(out["slices_2d"].device)
                out["slices_2d"][idx] = torch.from_numpy(np.ascontiguousarray(hs[:len(sel), :cap])).to(out["slices_2d"].device)
            else:
                out["slices_2d"][sel] = hs[:len(sel), :cap]
        return out

    def seed(self, consensus, trim_left=50, trim_right=50, min_support=3, maxindel=1000, nthreads=0, raw=False):
        """Genome.seed on the device: the same dict (plus n_deferred and n_spilled)"""
        packed = Genome.pack_consensus(consensus)
        n = packed["n"]
        o = self.seed_packed(packed, trim_left, trim_right, min_support, maxindel, nthreads)
        out = {k: o[k][:n] for k in ("status", "forward", "kmersupport", "pos", "contig", "slice_len")}
        out["n_deferred"], out["n_spilled"] = o["n_deferred"], o["n_spilled"]
        if raw:
            out["slices_2d"] = o["slices_2d"]
        else:
            out["slices"] = [o["slices_2d"][i, :out["slice_len"][i]].tobytes() for i in range(n)]
        return out


# ---- gapped chromatograms on the host (tracyhost_pad_batch): the fallback and the baseline of tracyhip_pad_traces ------------------------
PAD_KINDS = (("signal", None), ("bcpos", np.int32), ("primary", np.uint8), ("secondary", np.uint8), ("consensus", np.uint8), ("estqual", np.uint8))


def pad_alloc(flat, nsamples_out, ncalls_out):
    """result arrays of a padding call sized by the per-trace sizes (samples per channel, calls): dict with the six per-trace arrays, the
    payload arrays and their offsets / capacities"""
    nt = flat["nt"]
    scap = np.ascontiguousarray(nsamples_out, dtype=np.uint32)[:nt].copy() if nt else np.zeros(0, np.uint32)
    ccap = np.ascontiguousarray(ncalls_out, dtype=np.uint32)[:nt].copy() if nt else np.zeros(0, np.uint32)
    o = dict(sample_cap=np.append(scap, np.uint32(0)), call_cap=np.append(ccap, np.uint32(0)))
    o["sample_offset"] = np.zeros(nt + 1, np.uint64)
    o["call_offset"] = np.zeros(nt + 1, np.uint64)
    o["sample_offset"][1:] = np.cumsum(4 * scap.astype(np.uint64))
    o["call_offset"][1:] = np.cumsum(ccap.astype(np.uint64))
    o["signal"] = np.zeros(max(int(o["sample_offset"][nt]), 1), flat["signal"].dtype)
    for k, dt in PAD_KINDS[1:]:
        o[k] = np.zeros(max(int(o["call_offset"][nt]), 1), dt)
    o["status"] = np.zeros(max(nt, 1), np.int32)
    for k in ("nsamples_out", "ncalls_out", "leading_gaps", "trailing_gaps", "step"):
        o[k] = np.zeros(max(nt, 1), np.uint32)
    return o


def pad_batch_raw(flat, out, nthreads=0, sizes_only=False):
    """one tracyhost_pad_batch call over the flattened arrays of a PreparedPad (capi.py) into `out` (pad_alloc)"""
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    pay = (lambda k: None) if sizes_only else (lambda k: p(out[k]))
    rc = lib().tracyhost_pad_batch(C.c_uint32(flat["nt"]), p(flat["signal"]), p(flat["sig_off"]), p(flat["nsamples"]), C.c_uint32(flat["signal"].dtype.itemsize),
                                   p(flat["bcpos"]), p(flat["primary"]), p(flat["secondary"]), p(flat["consensus"]), p(flat["estqual"]),
                                   p(flat["bc_off"]), p(flat["bc_len"]), p(flat["rows"]), p(flat["row_off"]), p(flat["row_len"]),
                                   p(flat.get("trim_l")), p(flat.get("trim_r")), p(flat.get("reverse")), p(out["status"]), p(out["nsamples_out"]),
                                   p(out["ncalls_out"]), p(out["leading_gaps"]), p(out["trailing_gaps"]), p(out["step"]), pay("signal"),
                                   p(out["sample_offset"]), p(out["sample_cap"]), pay("bcpos"), pay("primary"), pay("secondary"), pay("consensus"),
                                   pay("estqual"), p(out["call_offset"]), p(out["call_cap"]), C.c_uint32(nthreads))
    if rc != 0:
        raise ValueError("tracyhost_pad_batch: bad arguments")
    return out


def pad_unpack(out, t):
    """trace t of a finished padding call (pad_alloc layout, host arrays) as the dict the tests compare"""
    st, nso, nco = int(out["status"][t]), int(out["nsamples_out"][t]), int(out["ncalls_out"][t])
    r = dict(status=st, nsamples_out=nso, ncalls_out=nco)
    if st != 0:
        return r
    so, co = int(out["sample_offset"][t]), int(out["call_offset"][t])
    r.update(signal=out["signal"][so:so + 4 * nso].reshape(4, nso), bcPos=out["bcpos"][co:co + nco], primary=out["primary"][co:co + nco].tobytes(),
             secondary=out["secondary"][co:co + nco].tobytes(), consensus=out["consensus"][co:co + nco].tobytes(), estQual=out["estqual"][co:co + nco],
             leadingGaps=int(out["leading_gaps"][t]), trailingGaps=int(out["trailing_gaps"][t]), step=int(out["step"][t]))
    return r


def pad_batch(flat, nthreads=0):
    """trim, reverse and pad a batch on host threads: a sizes-only call, buffers of exactly those sizes, the call; per-trace dicts (status 1:
    the reference's loops cannot run the trace)"""
    sizes = pad_batch_raw(flat, pad_alloc(flat, np.zeros(flat["nt"], np.uint32), np.zeros(flat["nt"], np.uint32)), nthreads, sizes_only=True)
    out = pad_batch_raw(flat, pad_alloc(flat, sizes["nsamples_out"], sizes["ncalls_out"]), nthreads)
    return [pad_unpack(out, t) for t in range(flat["nt"])]


# ---- the per-trace text of the writers on the host (tracyhost_render_batch): the fallback and the baseline of tracyhip_render_traces -----
RENDER_TSV, RENDER_JSON, RENDER_GAPPED = 0, 1, 2


def render_alloc(nt, text_cap, fill=None):
    """result arrays of a printing call with room for text_cap[t] bytes of trace t: status, text_len, text, text_offset, text_cap"""
    cap = np.ascontiguousarray(text_cap, dtype=np.uint64)[:nt].copy() if nt else np.zeros(0, np.uint64)
    o = dict(text_cap=np.append(cap, np.uint64(0)), text_offset=np.zeros(nt + 1, np.uint64))
    o["text_offset"][1:] = np.cumsum(cap)
    o["text"] = np.zeros(max(int(o["text_offset"][nt]), 1), np.uint8) if fill is None else np.full(max(int(o["text_offset"][nt]), 1), fill, np.uint8)
    o["status"] = np.zeros(max(nt, 1), np.int32)
    o["text_len"] = np.zeros(max(nt, 1), np.uint32)
    return o


def render_batch_raw(flat, form, out, nthreads=0, sizes_only=False):
    """one tracyhost_render_batch call over the flattened arrays of a PreparedRender (capi.py) into `out` (render_alloc)"""
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    rc = lib().tracyhost_render_batch(C.c_uint32(flat["nt"]), C.c_uint32(form), p(flat["signal"]), p(flat["sig_off"]), p(flat["nsamples"]),
                                      C.c_uint32(flat["signal"].dtype.itemsize), p(flat["bcpos"]), p(flat["primary"]), p(flat["secondary"]),
                                      p(flat.get("consensus")), p(flat["estqual"]), p(flat["bc_off"]), p(flat["bc_len"]), p(flat.get("trim_l")),
                                      p(flat.get("trim_r")), p(out["status"]), p(out["text_len"]), None if sizes_only else p(out["text"]),
                                      p(out["text_offset"]), p(out["text_cap"]), C.c_uint32(nthreads))
    if rc != 0:
        raise ValueError("tracyhost_render_batch: bad arguments")
    return out


def render_unpack(out, t):
    """trace t of a finished printing call (render_alloc layout, host arrays): dict(status, text_len[, text])"""
    st, n = int(out["status"][t]), int(out["text_len"][t])
    r = dict(status=st, text_len=n)
    if st == 0:
        o = int(out["text_offset"][t])
        r["text"] = out["text"][o:o + n].tobytes()
    return r


def render_batch(flat, form, nthreads=0):
    """print a batch on host threads: a sizes-only call, a buffer of exactly those sizes, the call; per-trace dicts (status 1: the
    reference's loops cannot run the trace, or it is beyond what the device answers)"""
    sizes = render_batch_raw(flat, form, render_alloc(flat["nt"], np.zeros(flat["nt"], np.uint64)), nthreads, sizes_only=True)
    out = render_batch_raw(flat, form, render_alloc(flat["nt"], sizes["text_len"]), nthreads)
    return [render_unpack(out, t) for t in range(flat["nt"])]


# ---- the text printed from alignment rows on the host (tracyhost_alntext_batch): the fallback and the baseline of
# tracyhip_render_alignments ---------------------------------------------------------------------------------------------------------------
ALNTEXT_PLOT, ALNTEXT_FASTA, ALNTEXT_JSON = 0, 1, 2
alntext_alloc = render_alloc  # (the result arrays of a printing call: status, text_len, text, text_offset, text_cap)
alntext_unpack = render_unpack


def alntext_pack(rows0, rows1, name0, name1, ref_pos, ref_len, forward, score=None):
    """per-alignment rows (bytes), names (bytes) and numbers as the flattened arrays of a PreparedAlnText (capi.py): rows back to back,
    the names of an alignment behind each other in one array"""
    nt = len(rows0)
    z = lambda dt: np.zeros(nt + 1, dt)
    f = dict(nt=nt, cols=z(np.uint32), rows_off=z(np.uint64), name0_off=z(np.uint64), name0_len=z(np.uint32), name1_off=z(np.uint64),
             name1_len=z(np.uint32))
    if any(len(a) != len(b) for a, b in zip(rows0, rows1)):
        raise ValueError("the two rows of an alignment have one length")
    f["cols"][:nt] = [len(r) for r in rows0]
    f["rows_off"][1:] = np.cumsum(f["cols"][:nt].astype(np.uint64))
    f["rows0"] = np.frombuffer(b"".join(bytes(r) for r in rows0) + b"\0", np.uint8).copy()
    f["rows1"] = np.frombuffer(b"".join(bytes(r) for r in rows1) + b"\0", np.uint8).copy()
    f["name0_len"][:nt] = [len(x) for x in name0]
    f["name1_len"][:nt] = [len(x) for x in name1]
    both = f["name0_len"][:nt].astype(np.uint64) + f["name1_len"][:nt].astype(np.uint64)
    f["name0_off"][1:] = np.cumsum(both)
    f["name1_off"][:nt] = f["name0_off"][:nt] + f["name0_len"][:nt]
    f["names"] = np.frombuffer(b"".join(bytes(a) + bytes(b) for a, b in zip(name0, name1)) + b"\0", np.uint8).copy()
    f["ref_pos"] = np.append(np.asarray(ref_pos, dtype=np.int64).astype(np.int32)[:nt], np.int32(0))
    f["ref_len"] = np.append(np.asarray(ref_len, dtype=np.uint32)[:nt], np.uint32(0))
    f["forward"] = np.append(np.asarray(forward, dtype=np.uint8)[:nt], np.uint8(0))
    f["score"] = np.append(np.asarray(score if score is not None else np.zeros(nt), dtype=np.int64).astype(np.int32)[:nt], np.int32(0))
    return f


def alntext_batch_raw(flat, form, out, key=0, linelimit=60, nthreads=0, sizes_only=False):
    """one tracyhost_alntext_batch call over the flattened arrays of a PreparedAlnText (capi.py) into `out` (alntext_alloc)"""
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    rc = lib().tracyhost_alntext_batch(C.c_uint32(flat["nt"]), C.c_uint32(form), C.c_uint32(key), C.c_uint32(linelimit), p(flat["rows0"]),
                                       p(flat["rows1"]), p(flat["rows_off"]), p(flat["cols"]), p(flat["names"]), p(flat["name0_off"]),
                                       p(flat["name0_len"]), p(flat["name1_off"]), p(flat["name1_len"]), p(flat["ref_pos"]), p(flat["ref_len"]),
                                       p(flat["forward"]), p(flat["score"]), p(out["status"]), p(out["text_len"]),
                                       None if sizes_only else p(out["text"]), p(out["text_offset"]), p(out["text_cap"]), C.c_uint32(nthreads))
    if rc != 0:
        raise ValueError("tracyhost_alntext_batch: bad arguments")
    return out


def alntext_batch(flat, form, key=0, linelimit=60, nthreads=0):
    """print a batch of alignments on host threads: a sizes-only call, a buffer of exactly those sizes, the call; per-alignment dicts"""
    sizes = alntext_batch_raw(flat, form, alntext_alloc(flat["nt"], np.zeros(flat["nt"], np.uint64)), key, linelimit, nthreads, sizes_only=True)
    out = alntext_batch_raw(flat, form, alntext_alloc(flat["nt"], sizes["text_len"]), key, linelimit, nthreads)
    return [alntext_unpack(out, t) for t in range(flat["nt"])]


# ---- the readers over a batch of file images on the host (tracyhost_read_batch): the fallback and the baseline of tracyhip_read_traces ---
READ_KINDS = (("signal", None), ("basecallpos", np.int32), ("basecalls1", np.uint8), ("basecalls2", np.uint8), ("qual", np.uint8))


def read_pack(files):
    """file images (bytes, or paths that are read here) one after another: dict(nt, bytes, file_off, file_len)"""
    imgs = []
    for f in files:
        if isinstance(f, (bytes, bytearray, memoryview)):
            imgs.append(bytes(f))
        else:
            with open(f, "rb") as fh:
                imgs.append(fh.read())
    nt = len(imgs)
    flen = np.array([len(b) for b in imgs] + [0], dtype=np.uint32)
    off = np.zeros(nt + 1, np.uint64)
    off[1:] = np.cumsum(flen[:nt].astype(np.uint64))
    return dict(nt=nt, bytes=np.frombuffer(b"".join(imgs) + b"\0" * 4, np.uint8).copy(), file_off=off, file_len=flen)


def read_alloc(nt, sample_dtype, nsamples, ncalls, fill=None):
    """result arrays of a reading call with room for nsamples[t] samples per channel and ncalls[t] calls of trace t"""
    scap = np.ascontiguousarray(nsamples, dtype=np.uint32)[:nt].copy() if nt else np.zeros(0, np.uint32)
    ccap = np.ascontiguousarray(ncalls, dtype=np.uint32)[:nt].copy() if nt else np.zeros(0, np.uint32)
    o = dict(sample_cap=np.append(scap, np.uint32(0)), call_cap=np.append(ccap, np.uint32(0)))
    o["sample_offset"] = np.zeros(nt + 1, np.uint64)
    o["call_offset"] = np.zeros(nt + 1, np.uint64)
    o["sample_offset"][1:] = np.cumsum(4 * scap.astype(np.uint64))
    o["call_offset"][1:] = np.cumsum(ccap.astype(np.uint64))
    for k, dt in READ_KINDS:
        size = max(int(o["sample_offset" if k == "signal" else "call_offset"][nt]), 1)
        o[k] = np.zeros(size, dt or sample_dtype) if fill is None else np.full(size, fill, dt or sample_dtype)
    o["status"] = np.zeros(max(nt, 1), np.int32)
    o["format"] = np.zeros(max(nt, 1), np.int32)
    o["nsamples"] = np.zeros(max(nt, 1), np.uint32)
    o["ncalls"] = np.zeros(max(nt, 1), np.uint32)
    return o


def read_batch_raw(flat, out, nthreads=0, sizes_only=False):
    """one tracyhost_read_batch call over packed file images (read_pack) into `out` (read_alloc)"""
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    pay = (lambda k: None) if sizes_only else (lambda k: p(out[k]))
    rc = lib().tracyhost_read_batch(C.c_uint32(flat["nt"]), p(flat["bytes"]), p(flat["file_off"]), p(flat["file_len"]),
                                    C.c_uint32(out["signal"].dtype.itemsize), p(out["status"]), p(out["format"]), p(out["nsamples"]), p(out["ncalls"]),
                                    pay("signal"), p(out["sample_offset"]), p(out["sample_cap"]), pay("basecallpos"), pay("basecalls1"),
                                    pay("basecalls2"), pay("qual"), p(out["call_offset"]), p(out["call_cap"]), C.c_uint32(nthreads))
    if rc != 0:
        raise ValueError("tracyhost_read_batch: bad arguments")
    return out


def read_unpack(out, t):
    """trace t of a finished reading call (read_alloc layout, host arrays) in the fields of read_trace, with its status"""
    st, ns, nc = int(out["status"][t]), int(out["nsamples"][t]), int(out["ncalls"][t])
    r = dict(status=st, format=int(out["format"][t]), nsamples=ns, ncalls=nc)
    if st != 0:
        return r
    so, co = int(out["sample_offset"][t]), int(out["call_offset"][t])
    r.update(signal=out["signal"][so:so + 4 * ns].reshape(4, ns), basecallpos=out["basecallpos"][co:co + nc],
             basecalls1=out["basecalls1"][co:co + nc].tobytes(), basecalls2=out["basecalls2"][co:co + nc].tobytes(), qual=out["qual"][co:co + nc])
    return r


def read_batch(files, sample_dtype=np.int32, nthreads=0):
    """read a batch of file images on host threads: a sizes-only call, buffers of exactly those sizes, the call; per-trace dicts (status 1:
    the reader refuses the image, or a sample does not fit the sample type)"""
    flat = files if isinstance(files, dict) else read_pack(files)
    nt = flat["nt"]
    sizes = read_batch_raw(flat, read_alloc(nt, sample_dtype, np.zeros(nt, np.uint32), np.zeros(nt, np.uint32)), nthreads, sizes_only=True)
    out = read_batch_raw(flat, read_alloc(nt, sample_dtype, sizes["nsamples"], sizes["ncalls"]), nthreads)
    return [read_unpack(out, t) for t in range(nt)]


# ---- the text printed from the decompose results on the host (tracyhost_dcptext_batch): the fallback and the baseline of
# tracyhip_render_decompositions ----------------------------------------------------------------------------------------------------------
DCPTEXT_DECOMP, DCPTEXT_JSON, DCPTEXT_VCF = 0, 1, 2
dcptext_alloc = render_alloc  # (the result arrays of a printing call: status, text_len, text, text_offset, text_cap)
dcptext_unpack = render_unpack
DCPTEXT_PAYLOADS = ("dcp_indel", "dcp_err", "rows0_0", "rows1_0", "rows0_1", "rows1_1", "rows0_2", "rows1_2", "bcpos", "estqual", "var", "var_text",
                    "var_n", "names")


def dcptext_pack(traces, max_variants=16, max_text=256):
    """per-trace dicts as the flattened arrays of a PreparedDcpText (capi.py).  A trace: dcp [(indel, err)], rows 3 x (row0, row1), bcpos,
    estqual, variants [dict(pos, basenum, gt, ref, alt)] (or var_n and records of its own: raw_var_n, raw_records [8 numbers each]),
    ref_pos (2), forward, score (3), breakpoint, indelshift, trim_left, trim_right, chr1, chr2, frac1, frac2 (bytes)"""
    from .capi import VARIANT_DTYPE
    nt = len(traces)
    z = lambda dt, n=nt + 1: np.zeros(n, dt)
    cum = lambda lens: np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)
    f = dict(nt=nt, max_variants=int(max_variants), max_text=int(max_text))
    f["dcp_rows"] = np.array([len(t["dcp"]) for t in traces] + [0], np.uint32)
    f["dcp_off"] = cum(f["dcp_rows"][:nt])
    flat = [p for t in traces for p in t["dcp"]]
    f["dcp_indel"] = np.array([a for a, _ in flat] + [0], np.int32)
    f["dcp_err"] = np.array([b for _, b in flat] + [0], np.int32)
    for k in range(3):
        f["cols_%d" % k] = np.array([len(t["rows"][k][0]) for t in traces] + [0], np.uint32)
        f["rows_off_%d" % k] = cum(f["cols_%d" % k][:nt])
        for r in range(2):
            f["rows%d_%d" % (r, k)] = np.frombuffer(b"".join(bytes(t["rows"][k][r]) for t in traces) + b"\0" * 4, np.uint8).copy()
    f["bc_len"] = np.array([len(t["bcpos"]) for t in traces] + [0], np.uint32)
    f["bc_off"] = cum(f["bc_len"][:nt])
    f["bcpos"] = np.concatenate([np.asarray(t["bcpos"], dtype=np.int32) for t in traces] + [np.zeros(1, np.int32)])
    f["estqual"] = np.concatenate([np.asarray(t["estqual"], dtype=np.uint8) for t in traces] + [np.zeros(1, np.uint8)])
    f["var"] = np.zeros(max(nt, 1) * max_variants, VARIANT_DTYPE)
    f["var_text"] = np.zeros(max(nt, 1) * max_text, np.uint8)
    f["var_n"] = z(np.uint32, max(nt, 1))
    for i, t in enumerate(traces):
        if "raw_records" in t:
            f["var_n"][i] = t["raw_var_n"]
            for j, rec in enumerate(t["raw_records"]):
                f["var"][i * max_variants + j] = tuple(rec)
            text = bytes(t.get("raw_text", b""))
            f["var_text"][i * max_text:i * max_text + len(text)] = np.frombuffer(text, np.uint8)
            continue
        at = 0
        f["var_n"][i] = len(t["variants"])
        for j, v in enumerate(t["variants"]):
            ref, alt = bytes(v["ref"]), bytes(v["alt"])
            f["var"][i * max_variants + j] = (v["pos"], v["basenum"], v["gt"], v.get("call_index", 0), at, len(ref), at + len(ref), len(alt))
            f["var_text"][i * max_text + at:i * max_text + at + len(ref) + len(alt)] = np.frombuffer(ref + alt, np.uint8)
            at += len(ref) + len(alt)
    for k in range(2):
        f["ref_pos_%d" % k] = np.array([t["ref_pos"][k] for t in traces] + [0], np.uint32)
    for k in range(3):
        f["score_%d" % k] = np.array([t["score"][k] for t in traces] + [0], np.int32)
    f["forward"] = np.array([1 if t["forward"] else 0 for t in traces] + [0], np.uint8)
    f["indelshift"] = np.array([1 if t["indelshift"] else 0 for t in traces] + [0], np.uint8)
    for k in ("breakpoint", "trim_left", "trim_right"):
        f[k] = np.array([t[k] for t in traces] + [0], np.uint32)
    parts = ("chr1", "chr2", "frac1", "frac2")
    lens = np.array([[len(t[p]) for p in parts] for t in traces], np.uint64).reshape(nt, 4)
    offs = cum(lens.reshape(-1))
    for j, p in enumerate(parts):
        f[p + "_len"] = np.append(lens[:, j].astype(np.uint32), np.uint32(0))
        f[p + "_off"] = np.append(offs[j:4 * nt:4], np.uint64(0)).astype(np.uint64)
    f["names"] = np.frombuffer(b"".join(bytes(t[p]) for t in traces for p in parts) + b"\0" * 4, np.uint8).copy()
    return f


def dcptext_job(flat, form, qual_cut, ptr):
    """a tracyhip_dcptext_job (capi.DcpTextJob) over the flattened arrays; ptr(key): the address of payload array `key`"""
    from . import capi
    u64, u32 = capi._u64p, capi._u32p
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    job = capi.DcpTextJob()
    job.n, job.form, job.qual_cut = flat["nt"], form, qual_cut
    job.dcp_indel, job.dcp_err = ptr("dcp_indel"), ptr("dcp_err")
    job.dcp_offset, job.dcp_rows = u64(flat["dcp_off"]), u32(flat["dcp_rows"])
    for k in range(3):
        job.rows0[k], job.rows1[k] = ptr("rows0_%d" % k), ptr("rows1_%d" % k)
        job.rows_offset[k], job.cols[k] = u64(flat["rows_off_%d" % k]), u32(flat["cols_%d" % k])
        job.score[k] = i32(flat["score_%d" % k])
    job.bcpos, job.estqual = ptr("bcpos"), ptr("estqual")
    job.bc_offset, job.bc_len = u64(flat["bc_off"]), u32(flat["bc_len"])
    job.var, job.var_text, job.var_n = ptr("var"), ptr("var_text"), ptr("var_n")
    job.max_variants, job.max_text = flat["max_variants"], flat["max_text"]
    if flat.get("var_index") is not None:  # (the place of every trace in the variant arrays; without it trace t lies at t)
        job.var_index = u32(flat["var_index"])
    for k in range(2):
        job.ref_pos[k] = u32(flat["ref_pos_%d" % k])
        job.chr_offset[k], job.chr_len[k] = u64(flat["chr%d_off" % (k + 1)]), u32(flat["chr%d_len" % (k + 1)])
        job.frac_offset[k], job.frac_len[k] = u64(flat["frac%d_off" % (k + 1)]), u32(flat["frac%d_len" % (k + 1)])
    job.forward, job.indelshift = u8(flat["forward"]), u8(flat["indelshift"])
    job.breakpoint, job.trim_left, job.trim_right = u32(flat["breakpoint"]), u32(flat["trim_left"]), u32(flat["trim_right"])
    job.names = ptr("names")
    return job


def dcptext_batch_raw(flat, form, out, qual_cut=45, nthreads=0, sizes_only=False):
    """one tracyhost_dcptext_batch call over the flattened arrays of a PreparedDcpText (capi.py) into `out` (dcptext_alloc)"""
    from . import capi
    job = dcptext_job(flat, form, qual_cut, lambda k: flat[k].ctypes.data)
    res = capi.RenderResult()
    res.status = out["status"].ctypes.data_as(C.POINTER(C.c_int32))
    res.text_len = capi._u32p(out["text_len"])
    res.text = None if sizes_only else out["text"].ctypes.data
    res.text_offset, res.text_cap = capi._u64p(out["text_offset"]), capi._u64p(out["text_cap"])
    if lib().tracyhost_dcptext_batch(C.byref(job), C.byref(res), C.c_uint32(nthreads)) != 0:
        raise ValueError("tracyhost_dcptext_batch: bad arguments")
    return out


def dcptext_batch(flat, form, qual_cut=45, nthreads=0):
    """print a batch of decompose reports on host threads: a sizes-only call, a buffer of exactly those sizes, the call; per-trace dicts
    (status 1: the writers would index outside an array)"""
    sizes = dcptext_batch_raw(flat, form, dcptext_alloc(flat["nt"], np.zeros(flat["nt"], np.uint64)), qual_cut, nthreads, sizes_only=True)
    out = dcptext_batch_raw(flat, form, dcptext_alloc(flat["nt"], sizes["text_len"]), qual_cut, nthreads)
    return [dcptext_unpack(out, t) for t in range(flat["nt"])]
