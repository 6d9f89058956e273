"""ctypes binding of include/tracy_hip.h (plumbing for tests and bench.py; plain pointers and sizes).

Loading fails loudly when the in-tree library is missing: build it with `python tracy_amd/build.py`
(or __graft_entry__.build()).  Nothing here computes on the CPU.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

OK, ERR_ARG, ERR_HIP, ERR_OOM, ERR_RANGE, ERR_NODEVICE = 0, -1, -2, -3, -4, -5
MEM_HOST, MEM_DEVICE = 0, 1
SEQ_CHAR, SEQ_PROFILE = 0, 1


class TracyHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("tracyhip error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("go", C.c_int32), ("ge", C.c_int32),
                ("hfree", C.c_int32), ("vfree", C.c_int32)]


class SeqSet(C.Structure):
    _fields_ = [("kind", C.c_int32), ("data", C.c_void_p), ("offset", C.POINTER(C.c_uint64)),
                ("length", C.POINTER(C.c_uint32)), ("count", C.c_uint32)]


class Pairs(C.Structure):
    _fields_ = [("npairs", C.c_uint32), ("a1", SeqSet), ("a2", SeqSet), ("a1_index", C.POINTER(C.c_uint32)),
                ("a2_index", C.POINTER(C.c_uint32))]


class AlignJob(C.Structure):
    _fields_ = [("ntraces", C.c_uint32), ("profiles", SeqSet), ("refs", SeqSet), ("ref_index", C.POINTER(C.c_uint32)),
                ("trim_left", C.c_uint32), ("trim_right", C.c_uint32), ("oriented", C.POINTER(C.c_uint8)),
                ("strand_by_certificate", C.c_uint32), ("trim_left_each", C.POINTER(C.c_uint32)),
                ("trim_right_each", C.POINTER(C.c_uint32))]


def trims_each(job, trim_left, trim_right, nt):
    """Fill a job's trims (AlignJob, DecomposeJob.dprm's scalars, SeedParams) from ints -- the scalar pair, as ever -- or from per-trace
    array-likes of length nt (trim_left_each / trim_right_each; an int beside an array is repeated).  Returns what must stay alive."""
    scalars = job.dprm if hasattr(job, "dprm") else job
    if np.ndim(trim_left) == 0 and np.ndim(trim_right) == 0:
        scalars.trim_left, scalars.trim_right = int(trim_left), int(trim_right)
        return ()
    arrs = []
    for v in (trim_left, trim_right):
        a = np.full(nt, v, dtype=np.uint32) if np.ndim(v) == 0 else np.ascontiguousarray(v, dtype=np.uint32)
        if a.shape != (nt,):
            raise ValueError("per-trace trims: expected %d values, got shape %s" % (nt, a.shape))
        arrs.append(a)
    scalars.trim_left, scalars.trim_right = 0, 0
    job.trim_left_each = arrs[0].ctypes.data_as(C.POINTER(C.c_uint32))
    job.trim_right_each = arrs[1].ctypes.data_as(C.POINTER(C.c_uint32))
    return tuple(arrs)


class AlignResult(C.Structure):
    _fields_ = [("score_fwd", C.c_void_p), ("score_rev", C.c_void_p), ("forward", C.c_void_p),
                ("score_prelim", C.c_void_p), ("slice_begin", C.c_void_p), ("slice_len", C.c_void_p),
                ("ref_pos", C.c_void_p), ("score_final", C.c_void_p), ("ops", C.c_void_p),
                ("ops_offset", C.POINTER(C.c_uint64)), ("ops_len", C.c_void_p), ("rows0", C.c_void_p), ("rows1", C.c_void_p)]


class CallStats(C.Structure):
    _fields_ = [("traces", C.c_uint32), ("stream_ordered", C.c_uint32), ("host_syncs", C.c_uint32), ("fallback_traces", C.c_uint32),
                ("pruned", C.c_uint32), ("pruned_uncertified", C.c_uint32), ("prelim_banded", C.c_uint32), ("prelim_repeated", C.c_uint32),
                ("final_banded", C.c_uint32), ("final_repeated", C.c_uint32), ("allele_pruned", C.c_uint32 * 2),
                ("allele_uncertified", C.c_uint32 * 2), ("allele_banded", C.c_uint32 * 3), ("allele_repeated", C.c_uint32 * 3),
                ("allele_shared_prefix", C.c_uint32), ("cons_fixup_columns", C.c_uint32), ("cons_chunks", C.c_uint32),
                ("asm_chunks", C.c_uint32), ("asm_steps", C.c_uint32),
                ("denovo_chunks", C.c_uint32), ("denovo_rounds", C.c_uint32), ("denovo_steps", C.c_uint32)]


class CallStatsVariants(CallStats):
    """CallStats (the counters through denovo_steps, kept as it was: tests pin its tail) with the four counters of
    tracyhip_decompose_variants appended -- ctypes lays a subclass's fields out behind its base's, as the C struct grew.  The struct
    has grown since: CallStatsWildtype below is THE mirror of tracyhip_call_stats, and the only one to hand to
    tracyhip_last_call_stats -- anything shorter is an out-of-bounds write.  Context.last_call_stats uses it."""
    _fields_ = [("var_traces", C.c_uint32), ("var_realigned", C.c_uint32), ("var_truncated", C.c_uint32), ("var_chunks", C.c_uint32)]


class CallStatsSweeps(CallStatsVariants):
    """CallStatsVariants with the two counters of the offset-form sweeps behind it, as the C struct grew."""
    _fields_ = [("sweep_diag_launches", C.c_uint32), ("prefix_diag_launches", C.c_uint32)]


class CallStatsBands(CallStatsSweeps):
    """CallStatsSweeps with the band stages' list sizes ([kind][strip height 12 / 8 / 4 / quad form]) and the count of stages that took
    the large-batch form behind it, as the C struct grew."""
    _fields_ = [("band_list_pairs", (C.c_uint32 * 4) * 2), ("band_large_launches", C.c_uint32)]


class CallStatsSeed(CallStatsBands):
    """CallStatsBands with the three counters of tracyhip_seed_traces under the option seed_spill behind it, as the C struct grew."""
    _fields_ = [("seed_spilled", C.c_uint32), ("seed_spill_launches", C.c_uint32), ("seed_spill_deferred", C.c_uint32)]


class CallStatsWildtype(CallStatsSeed):
    """CallStatsSeed with the chunk counter of the wildtype jobs of tracyhip_align_traces behind it, as the C struct grew: THE mirror of
    tracyhip_call_stats now, and what Context.last_call_stats hands to the library."""
    _fields_ = [("wt_chunks", C.c_uint32)]


class PadStats(C.Structure):
    """tracyhip_pad_stats: the counters of tracyhip_pad_traces.  Not a further CallStats subclass: tracyhip_call_stats keeps its layout,
    which tests pin against the header; Context.last_call_stats reports both under one dict."""
    _fields_ = [("pad_chunks", C.c_uint32), ("pad_deferred", C.c_uint32), ("pad_too_small", C.c_uint32)]


class RenderStats(C.Structure):
    """tracyhip_render_stats: the counters of tracyhip_render_traces, in a struct of their own as PadStats"""
    _fields_ = [("render_chunks", C.c_uint32), ("render_deferred", C.c_uint32), ("render_too_small", C.c_uint32)]


class AlnTextStats(C.Structure):
    """tracyhip_alntext_stats: the counters of tracyhip_render_alignments, in a struct of their own as RenderStats"""
    _fields_ = [("alntext_chunks", C.c_uint32), ("alntext_deferred", C.c_uint32), ("alntext_too_small", C.c_uint32)]


class ReadStats(C.Structure):
    """tracyhip_read_stats: the counters of tracyhip_read_traces, in a struct of their own as PadStats"""
    _fields_ = [("read_chunks", C.c_uint32), ("read_deferred", C.c_uint32), ("read_too_small", C.c_uint32)]


def library_path():
    return os.path.join(_HERE, "lib", "libtracy_hip.so")


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        p = library_path()
        if not os.path.exists(p):
            raise ImportError("tracy_amd: %s is missing -- run `python tracy_amd/build.py` (hipcc, gfx950). "
                              "There is no CPU fallback." % p)
        _LIB = C.CDLL(p)
        _LIB.tracyhip_last_error.restype = C.c_char_p
        _LIB.tracyhip_version.restype = C.c_char_p
        _LIB.tracyhip_group_context.restype = C.c_void_p
        _LIB.tracyhip_render_bound.restype = C.c_uint64
        _LIB.tracyhip_render_alignments_bound.restype = C.c_uint64
    return _LIB


def _check(rc):
    if rc != OK:
        raise TracyHipError(rc, lib().tracyhip_last_error().decode())


def device_count():
    n = C.c_int(0)
    rc = lib().tracyhip_device_count(C.byref(n))
    return n.value if rc == OK else 0


class PackedSeqs:
    """Host-side packing of a list of sequences (bytes) or profiles (float32 [6][len])."""

    def __init__(self, seqs, kind=None):
        if kind is None:
            kind = SEQ_CHAR if (len(seqs) == 0 or isinstance(seqs[0], (bytes, bytearray))) else SEQ_PROFILE
        self.kind = kind
        self.count = len(seqs)
        self.length = np.zeros(max(self.count, 1), dtype=np.uint32)
        self.offset = np.zeros(max(self.count, 1), dtype=np.uint64)
        pos = 0
        parts = []
        for i, s in enumerate(seqs):
            if kind == SEQ_CHAR:
                a = np.frombuffer(bytes(s), dtype=np.uint8)
                ln = a.size
            else:
                a = np.ascontiguousarray(s, dtype=np.float32)
                assert a.ndim == 2 and a.shape[0] == 6
                ln = a.shape[1]
                a = a.reshape(-1)
            self.length[i] = ln
            self.offset[i] = pos
            pos += a.size
            parts.append(a)
        dt = np.uint8 if kind == SEQ_CHAR else np.float32
        self.data = np.concatenate(parts) if parts and pos else np.zeros(1, dtype=dt)
        self.nelem = pos

    def seqset(self, data_ptr=None):
        s = SeqSet()
        s.kind = self.kind
        s.data = data_ptr if data_ptr is not None else self.data.ctypes.data
        s.offset = self.offset.ctypes.data_as(C.POINTER(C.c_uint64))
        s.length = self.length.ctypes.data_as(C.POINTER(C.c_uint32))
        s.count = self.count
        return s


def describe_options(name=None, value=None):
    """tracyhip_describe_options: the options a context created now would start with (defaults + TRACYHIP_* environment), with
    name = value set on top; needs no device.  Raises where tracyhip_set_option would refuse."""
    nm = None if name is None else str(name).encode()
    val = None if value is None else str(int(value) if isinstance(value, bool) else value).encode()
    n = lib().tracyhip_describe_options(nm, val, None, C.c_size_t(0))
    if n < 0:
        _check(n)
    buf = C.create_string_buffer(n)
    lib().tracyhip_describe_options(nm, val, buf, C.c_size_t(n))
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


class Context:
    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(lib().tracyhip_create(int(device), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().tracyhip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(lib().tracyhip_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_workspace_limit(self, nbytes):
        _check(lib().tracyhip_set_workspace_limit(self._h, C.c_uint64(nbytes)))

    def set_lanes(self, n):
        """batch pipelines split a call into n chunks in flight (own stream + host thread each); 1 = off"""
        _check(lib().tracyhip_set_lanes(self._h, C.c_uint32(n)))

    def synchronize(self):
        _check(lib().tracyhip_synchronize(self._h))

    def set_option(self, name, value):
        """tracyhip_set_option: name without the TRACYHIP_ prefix (the environment is read once, at creation)"""
        _check(lib().tracyhip_set_option(self._h, str(name).encode(), str(int(value) if isinstance(value, bool) else value).encode()))

    def describe(self):
        n = lib().tracyhip_describe(self._h, None, C.c_size_t(0))
        buf = C.create_string_buffer(n)
        lib().tracyhip_describe(self._h, buf, C.c_size_t(n))
        return dict(line.split("=", 1) for line in buf.value.decode().splitlines())

    def last_call_stats(self):
        """tiers the traces of the last align_traces / decompose_traces call took (tracyhip_last_call_stats)"""
        st = CallStatsWildtype()
        _check(lib().tracyhip_last_call_stats(self._h, C.byref(st)))
        out = {}
        for name, ty in (CallStats._fields_ + CallStatsVariants._fields_ + CallStatsSweeps._fields_ + CallStatsBands._fields_
                         + CallStatsSeed._fields_ + CallStatsWildtype._fields_):
            v = getattr(st, name)
            if name == "band_list_pairs":
                out[name] = [list(row) for row in v]
                continue
            out[name] = list(v) if hasattr(v, "__len__") else int(v)
        ps = PadStats()  # (tracyhip_pad_traces counts in a struct of its own: tracyhip_last_pad_stats)
        _check(lib().tracyhip_last_pad_stats(self._h, C.byref(ps)))
        out.update({name: int(getattr(ps, name)) for name, _ in PadStats._fields_})
        rs = RenderStats()  # (and so does tracyhip_render_traces: tracyhip_last_render_stats)
        _check(lib().tracyhip_last_render_stats(self._h, C.byref(rs)))
        out.update({name: int(getattr(rs, name)) for name, _ in RenderStats._fields_})
        ds = ReadStats()  # (and tracyhip_read_traces: tracyhip_last_read_stats)
        _check(lib().tracyhip_last_read_stats(self._h, C.byref(ds)))
        out.update({name: int(getattr(ds, name)) for name, _ in ReadStats._fields_})
        ts = AlnTextStats()  # (and tracyhip_render_alignments: tracyhip_last_alntext_stats)
        _check(lib().tracyhip_last_alntext_stats(self._h, C.byref(ts)))
        out.update({name: int(getattr(ts, name)) for name, _ in AlnTextStats._fields_})
        return out

    # ---- host-buffer convenience wrappers (lists in, numpy out) -----------------------------------
    @staticmethod
    def _pairs(a1, a2, idx1=None, idx2=None):
        p1 = a1 if isinstance(a1, PackedSeqs) else PackedSeqs(a1)
        p2 = a2 if isinstance(a2, PackedSeqs) else PackedSeqs(a2)
        pr = Pairs()
        keep = [p1, p2]
        if idx1 is not None:
            idx1 = np.ascontiguousarray(idx1, dtype=np.uint32)
            idx2 = np.ascontiguousarray(idx2, dtype=np.uint32)
            pr.npairs = len(idx1)
            pr.a1_index = idx1.ctypes.data_as(C.POINTER(C.c_uint32))
            pr.a2_index = idx2.ctypes.data_as(C.POINTER(C.c_uint32))
            keep += [idx1, idx2]
        else:
            assert p1.count == p2.count
            pr.npairs = p1.count
        pr.a1 = p1.seqset()
        pr.a2 = p2.seqset()
        return pr, keep, p1, p2

    def _pair_lengths(self, pr, p1, p2, idx1, idx2):
        if idx1 is None:
            return p1.length[:pr.npairs].astype(np.uint64), p2.length[:pr.npairs].astype(np.uint64)
        return p1.length[np.asarray(idx1)].astype(np.uint64), p2.length[np.asarray(idx2)].astype(np.uint64)

    def score(self, a1, a2, params, needle=False, idx1=None, idx2=None):
        pr, keep, p1, p2 = self._pairs(a1, a2, idx1, idx2)
        prm = Params(*params)
        out = np.zeros(max(pr.npairs, 1), dtype=np.int32)
        fn = lib().tracyhip_needle_score if needle else lib().tracyhip_gotoh_score
        _check(fn(self._h, C.byref(pr), C.byref(prm), MEM_HOST, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out[:pr.npairs]

    def align(self, a1, a2, params, needle=False, idx1=None, idx2=None, rows=False):
        """returns (scores, [btr bytes per pair, push order]) and optionally the alignment rows"""
        pr, keep, p1, p2 = self._pairs(a1, a2, idx1, idx2)
        prm = Params(*params)
        n = pr.npairs
        l1, l2 = self._pair_lengths(pr, p1, p2, idx1, idx2)
        cap = (l1 + l2).astype(np.uint64)
        off = np.zeros(max(n, 1), dtype=np.uint64)
        if n:
            off[1:n] = np.cumsum(cap)[:-1]
        total = int(cap.sum()) if n else 0
        ops = np.zeros(max(total, 1), dtype=np.uint8)
        olen = np.zeros(max(n, 1), dtype=np.uint32)
        scores = np.zeros(max(n, 1), dtype=np.int32)
        fn = lib().tracyhip_needle_align if needle else lib().tracyhip_gotoh_align
        _check(fn(self._h, C.byref(pr), C.byref(prm), MEM_HOST, scores.ctypes.data_as(C.POINTER(C.c_int32)),
                  ops.ctypes.data_as(C.POINTER(C.c_uint8)), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                  olen.ctypes.data_as(C.POINTER(C.c_uint32))))
        btr = [ops[int(off[i]):int(off[i]) + int(olen[i])].tobytes() for i in range(n)]
        if not rows:
            return scores[:n], btr
        r0 = np.zeros(max(total, 1), dtype=np.uint8)
        r1 = np.zeros(max(total, 1), dtype=np.uint8)
        _check(lib().tracyhip_alignment_rows(self._h, C.byref(pr), MEM_HOST, ops.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             olen.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             r0.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             r1.ctypes.data_as(C.POINTER(C.c_uint8))))
        rws = [(r0[int(off[i]):int(off[i]) + int(olen[i])].tobytes(), r1[int(off[i]):int(off[i]) + int(olen[i])].tobytes())
               for i in range(n)]
        return scores[:n], btr, rws


def _align_banded(self, a1, a2, params, band_lo, band_hi, origin=False):
    """tracyhip_gotoh_banded with host buffers: (scores, btr list) or, origin=True, (scores, [(lead, c_e)])"""
    pr, keep, p1, p2 = self._pairs(a1, a2, None, None)
    prm = Params(*params)
    n = pr.npairs
    l1, l2 = self._pair_lengths(pr, p1, p2, None, None)
    cap = (l1 + l2).astype(np.uint64)
    off = np.zeros(max(n, 1), dtype=np.uint64)
    if n:
        off[1:n] = np.cumsum(cap)[:-1]
    ops = np.zeros(max(int(cap.sum()) if n else 0, 1), dtype=np.uint8)
    olen = np.zeros(max(n, 1), dtype=np.uint32)
    scores = np.zeros(max(n, 1), dtype=np.int32)
    ends = np.zeros(2 * max(n, 1), dtype=np.uint32)
    lo = np.ascontiguousarray(band_lo, dtype=np.int32)
    hi = np.ascontiguousarray(band_hi, dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    _check(lib().tracyhip_gotoh_banded(self._h, C.byref(pr), C.byref(prm), lo.ctypes.data_as(i32p), hi.ctypes.data_as(i32p), MEM_HOST,
                                       scores.ctypes.data_as(i32p), ops.ctypes.data_as(C.POINTER(C.c_uint8)), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       olen.ctypes.data_as(C.POINTER(C.c_uint32)), ends.ctypes.data_as(C.POINTER(C.c_uint32)) if origin else None))
    if origin:
        return scores[:n], [(int(ends[2 * i]), int(ends[2 * i + 1])) for i in range(n)]
    return scores[:n], [ops[int(off[i]):int(off[i]) + int(olen[i])].tobytes() for i in range(n)]


class PreparedAlign:
    """host-buffer job / result structs of tracyhip_align_traces (everything they point to is kept alive by this object)"""

    def __init__(self, profiles, refs, params, trim_left=50, trim_right=50, ref_index=None, oriented=None, exact_scores=True,
                 ref_profiles=None, rows=False):
        """ref_profiles (a list of float32 [6][n] or a PackedSeqs): a wildtype job -- the FORWARD profile of every wildtype, indexed by
        ref_index; refs is then not read (pass None).  rows: rows0 / rows1 of the final alignment as well (wildtype jobs only)."""
        pp = profiles if isinstance(profiles, PackedSeqs) else PackedSeqs(profiles, SEQ_PROFILE)
        self.wildtype = ref_profiles is not None
        if self.wildtype:
            pr = ref_profiles if isinstance(ref_profiles, PackedSeqs) else PackedSeqs(ref_profiles, SEQ_PROFILE)
        else:
            pr = refs if isinstance(refs, PackedSeqs) else PackedSeqs(refs, SEQ_CHAR)
        nt = self.nt = pp.count
        job = self.job = AlignJob()
        job.ntraces = nt
        job.profiles = pp.seqset()
        job.refs = pr.seqset()  # (kind PROFILE makes it a wildtype job)
        self.keep = [pp, pr]
        if ref_index is not None:
            ref_index = np.ascontiguousarray(ref_index, dtype=np.uint32)
            job.ref_index = ref_index.ctypes.data_as(C.POINTER(C.c_uint32))
            rlen = pr.length[ref_index]
            self.keep.append(ref_index)
        else:
            rlen = pr.length[:nt]
        self.keep.extend(trims_each(job, trim_left, trim_right, nt))  # ints, or per-trace array-likes
        job.strand_by_certificate = 0 if exact_scores else 1  # opt-in: the losing strand may carry a certified upper bound
        if oriented is not None:
            oriented = np.ascontiguousarray(oriented, dtype=np.uint8)
            job.oriented = oriented.ctypes.data_as(C.POINTER(C.c_uint8))
            self.keep.append(oriented)
        cap = pp.length[:nt].astype(np.uint64) + rlen.astype(np.uint64)
        off = self.off = np.zeros(max(nt, 1), dtype=np.uint64)
        if nt:
            off[1:nt] = np.cumsum(cap)[:-1]
        res = self.res = {
            "score_fwd": np.zeros(max(nt, 1), np.int32), "score_rev": np.zeros(max(nt, 1), np.int32),
            "forward": np.zeros(max(nt, 1), np.uint8), "score_prelim": np.zeros(max(nt, 1), np.int32),
            "slice_begin": np.zeros(max(nt, 1), np.uint32), "slice_len": np.zeros(max(nt, 1), np.uint32),
            "ref_pos": np.zeros(max(nt, 1), np.uint32), "score_final": np.zeros(max(nt, 1), np.int32),
            "ops": np.zeros(max(int(cap.sum()) if nt else 0, 1), np.uint8), "ops_len": np.zeros(max(nt, 1), np.uint32),
        }
        if rows:
            res["rows0"], res["rows1"] = np.zeros_like(res["ops"]), np.zeros_like(res["ops"])
        out = self.out = AlignResult()
        for k in res:
            setattr(out, k, res[k].ctypes.data)
        out.ops_offset = off.ctypes.data_as(C.POINTER(C.c_uint64))
        self.prm = Params(params[0], params[1], params[2], params[3], 1, 0)

    def results(self):
        res, off, nt = dict(self.res), self.off, self.nt
        cut = lambda a: [a[int(off[i]):int(off[i]) + int(res["ops_len"][i])].tobytes() for i in range(nt)]
        btr = cut(res["ops"])
        if "rows0" in res:
            res["rows0"], res["rows1"] = cut(res["rows0"]), cut(res["rows1"])
        for k in list(res):
            if k not in ("ops", "rows0", "rows1"):
                res[k] = res[k][:nt]
        res["btr"] = btr
        return res


def _align_traces(self, profiles, refs, params, trim_left=50, trim_right=50, ref_index=None, oriented=None, exact_scores=True, device=False,
                  ref_profiles=None, rows=False):
    """tracyhip_align_traces with host buffers.  profiles: list of float32 [6][mf]; refs: list of bytes.
    ref_profiles: a wildtype job (refs None) -- the forward profile of every wildtype, a list of float32 [6][n] or a PackedSeqs, joined
    through ref_index; the strand is chosen on the device.  rows=True adds "rows0" / "rows1" (bytes per trace) to the result.
    oriented: None, or rs.forward per trace when the references are already oriented (indexed-genome path).
    trim_left / trim_right: ints, or per-trace array-likes (e.g. PreparedBasecall.trims() of a run with a trim stringency).
    device=True: payloads and result arrays in device memory (torch tensors, TRACYHIP_MEM_DEVICE), copied back afterwards.
    Returns a dict of numpy arrays + the list of final traceback strings (push order)."""
    p = PreparedAlign(profiles, refs, params, trim_left, trim_right, ref_index, oriented, exact_scores, ref_profiles, rows)
    if device:
        import torch
        pp, pr = p.keep[0], p.keep[1]
        dp, dr = torch.from_numpy(pp.data).cuda(), torch.from_numpy(pr.data).cuda()
        p.job.profiles = pp.seqset(dp.data_ptr())
        p.job.refs = pr.seqset(dr.data_ptr())
        dres = {k: torch.zeros(v.shape, dtype=getattr(torch, str(v.dtype)) if str(v.dtype) != "uint32" else torch.int32, device="cuda") for k, v in p.res.items()}
        for k, v in dres.items():
            setattr(p.out, k, v.data_ptr())
        torch.cuda.synchronize()
        _check(lib().tracyhip_align_traces(self._h, C.byref(p.job), C.byref(p.prm), MEM_DEVICE, C.byref(p.out)))
        torch.cuda.synchronize()
        for k, v in dres.items():
            p.res[k] = v.cpu().numpy().view(p.res[k].dtype)
        return p.results()
    if isinstance(self, Group):
        _check(lib().tracyhip_group_align_traces(self._g, C.byref(p.job), C.byref(p.prm), C.byref(p.out)))
    else:
        _check(lib().tracyhip_align_traces(self._h, C.byref(p.job), C.byref(p.prm), MEM_HOST, C.byref(p.out)))
    return p.results()


Context.align_traces = _align_traces


def _align_traces_async(self, job, prm, out, mem=MEM_DEVICE):
    """tracyhip_align_traces_async on prepared structs (they, and everything they point to, must outlive synchronize())"""
    _check(lib().tracyhip_align_traces_async(self._h, C.byref(job), C.byref(prm), mem, C.byref(out)))


Context.align_traces_async = _align_traces_async


CONS_OK, CONS_NO_OVERLAP = 0, 1


class ConsensusJob(C.Structure):
    _fields_ = [("npairs", C.c_uint32), ("first", SeqSet), ("second", SeqSet), ("compute_union", C.c_uint32), ("iupac", C.c_uint32),
                ("min_overlap", C.c_uint32), ("match_fraction", C.c_float)]


class ConsensusResult(C.Structure):
    _fields_ = [("score_fwd", C.c_void_p), ("score_rev", C.c_void_p), ("forward", C.c_void_p), ("score", C.c_void_p),
                ("num_aligned", C.c_void_p), ("num_match", C.c_void_p), ("status", C.c_void_p), ("rows0", C.c_void_p),
                ("rows1", C.c_void_p), ("ops_len", C.c_void_p), ("cons", C.c_void_p), ("qual", C.c_void_p), ("cons_len", C.c_void_p),
                ("offset", C.POINTER(C.c_uint64))]


class _Prepared:
    """what the prepared batch objects share: `job` / `prm` / `out` structs over host arrays -- `keep`, the payload PackedSeqs, one per
    job field of _PAYLOADS; `res`, the result arrays by the field of `out` that points to them -- and their device form"""

    _PAYLOADS = ()

    def _bind_results(self, out, res):
        self.out, self.res = out, res
        for k, v in res.items():
            setattr(out, k, v.ctypes.data)

    def to_device(self):
        """payloads and result arrays as torch tensors on the current device (kept alive by this object)"""
        import torch
        self.dkeep = [torch.from_numpy(p.data).cuda() for p in self.keep]
        for name, p, d in zip(self._PAYLOADS, self.keep, self.dkeep):
            setattr(self.job, name, p.seqset(d.data_ptr()))
        self.dres = {k: torch.zeros(v.nbytes, dtype=torch.uint8, device="cuda") for k, v in self.res.items()}
        for k, v in self.dres.items():
            setattr(self.out, k, v.data_ptr())
        torch.cuda.synchronize()

    def from_device(self):
        for k, v in self.dres.items():
            self.res[k] = v.cpu().numpy().view(self.res[k].dtype)


def _run_prepared(ctx, symbol, p, device):
    """one call of the library on a prepared batch, over host arrays or (device=True) over device memory copied back afterwards"""
    fn = getattr(lib(), symbol)
    if device:
        import torch
        p.to_device()
        _check(fn(ctx._h, C.byref(p.job), C.byref(p.prm), MEM_DEVICE, C.byref(p.out)))
        torch.cuda.synchronize()
        p.from_device()
    else:
        _check(fn(ctx._h, C.byref(p.job), C.byref(p.prm), MEM_HOST, C.byref(p.out)))
    return p.results()


class PreparedConsensus(_Prepared):
    """host-buffer job / result structs of tracyhip_consensus_traces (everything they point to is kept alive by this object).
    first / second: lists of float32 [6][len] (the trimmed profile of trace 1, the trimmed FORWARD profile of trace 2)."""

    _PAYLOADS = ("first", "second")
    _PAIR = (("score_fwd", np.int32), ("score_rev", np.int32), ("forward", np.uint8), ("score", np.int32), ("num_aligned", np.uint32),
             ("num_match", np.uint32), ("status", np.int32), ("ops_len", np.uint32), ("cons_len", np.uint32))

    def __init__(self, first, second, params, union=True, iupac=False, min_overlap=25, match_fraction=0.5):
        p1 = first if isinstance(first, PackedSeqs) else PackedSeqs(first, SEQ_PROFILE)
        p2 = second if isinstance(second, PackedSeqs) else PackedSeqs(second, SEQ_PROFILE)
        if p1.count != p2.count:
            raise ValueError("first and second need one profile per pair")
        n = self.n = p1.count
        self.keep = [p1, p2]
        job = self.job = ConsensusJob()
        job.npairs = n
        job.first = p1.seqset()
        job.second = p2.seqset()
        job.compute_union = 1 if union else 0
        job.iupac = 1 if iupac else 0
        job.min_overlap = int(min_overlap)
        job.match_fraction = float(match_fraction)
        cap = p1.length[:n].astype(np.uint64) + p2.length[:n].astype(np.uint64)
        off = self.off = np.zeros(max(n, 1), dtype=np.uint64)
        if n:
            off[1:n] = np.cumsum(cap)[:-1]
        total = max(int(cap.sum()) if n else 0, 1)
        res = {k: np.zeros(max(n, 1), dt) for k, dt in self._PAIR}
        res.update(rows0=np.zeros(total, np.uint8), rows1=np.zeros(total, np.uint8), cons=np.zeros(total, np.uint8),
                   qual=np.zeros(total, np.uint16))
        self._bind_results(ConsensusResult(), res)
        self.out.offset = off.ctypes.data_as(C.POINTER(C.c_uint64))
        self.prm = Params(*params) if len(params) == 6 else Params(params[0], params[1], params[2], params[3], 1, 1)

    def results(self):
        """per-pair arrays, and lists rows (row0, row1 bytes), cons (bytes), qual (uint16 arrays)"""
        res, off, n = self.res, self.off, self.n
        out = {k: res[k][:n].copy() for k, _ in self._PAIR}
        out["rows"] = [(res["rows0"][int(off[i]):int(off[i]) + int(res["ops_len"][i])].tobytes(),
                        res["rows1"][int(off[i]):int(off[i]) + int(res["ops_len"][i])].tobytes()) for i in range(n)]
        out["cons"] = [res["cons"][int(off[i]):int(off[i]) + int(res["cons_len"][i])].tobytes() for i in range(n)]
        out["qual"] = [res["qual"][int(off[i]):int(off[i]) + int(res["cons_len"][i])].copy() for i in range(n)]
        return out


def _consensus_traces(self, first, second, params, union=True, iupac=False, min_overlap=25, match_fraction=0.5, device=False):
    """tracyhip_consensus_traces: `tracy consensus` for a batch of trace pairs.  params: (match, mismatch, go, ge) with free end gaps
    on both axes (the command's AlignConfig<true,true>), or all six tracyhip_params fields.  device=True: payloads and results in
    device memory (TRACYHIP_MEM_DEVICE), copied back afterwards."""
    p = PreparedConsensus(first, second, params, union, iupac, min_overlap, match_fraction)
    return _run_prepared(self, "tracyhip_consensus_traces", p, device)


Context.consensus_traces = _consensus_traces


def _consensus_traces_async(self, job, prm, out, mem=MEM_HOST):
    """tracyhip_consensus_traces_async on prepared structs (PreparedConsensus: they, and everything they point to, must outlive
    synchronize())"""
    _check(lib().tracyhip_consensus_traces_async(self._h, C.byref(job), C.byref(prm), mem, C.byref(out)))


Context.consensus_traces_async = _consensus_traces_async


class AssembleJob(C.Structure):
    _fields_ = [("ngroups", C.c_uint32), ("traces", SeqSet), ("group_first", C.POINTER(C.c_uint32)), ("references", SeqSet),
                ("ref_index", C.POINTER(C.c_uint32)), ("match_fraction", C.c_float), ("fraction_called", C.c_float),
                ("include_reference", C.c_uint32)]


class AssembleResult(C.Structure):
    _fields_ = [("score_fwd", C.c_void_p), ("score_rev", C.c_void_p), ("forward", C.c_void_p), ("rank", C.c_void_p), ("nrows", C.c_void_p),
                ("ncol", C.c_void_p), ("rows", C.c_void_p), ("gapped", C.c_void_p), ("cons", C.c_void_p), ("qual", C.c_void_p),
                ("cons_len", C.c_void_p), ("rows_offset", C.POINTER(C.c_uint64)), ("col_offset", C.POINTER(C.c_uint64))]


class _PreparedGroups(_Prepared):
    """the two calls over groups of traces: group_first, the per-group capacities and offsets of tracy_hip.h, the per-group results"""

    _GROUP = (("nrows", np.uint32), ("ncol", np.uint32), ("cons_len", np.uint32))

    def _pack_groups(self, groups):
        """the traces of every group in one PackedSeqs, and the summed trace length of every group; sets ng, nt, first"""
        ng = self.ng = len(groups)
        pt = PackedSeqs([p for g in groups for p in g], SEQ_PROFILE)
        self.nt = pt.count
        first = self.first = np.zeros(ng + 1, np.uint32)
        first[1:] = np.cumsum([len(g) for g in groups], dtype=np.int64) if ng else 0
        return pt, [int(pt.length[int(first[g]):int(first[g + 1])].sum()) for g in range(ng)]

    def _bind_groups(self, out, bounds):
        """the result arrays of `out`; bounds: per group the (rows, columns) its alignment can reach at most"""
        ng, nt = self.ng, self.nt
        rowcap = np.array([r * c for r, c in bounds], np.uint64)
        colcap = np.array([c for _, c in bounds], np.uint64)
        self.roff = np.zeros(max(ng, 1), np.uint64)
        self.coff = np.zeros(max(ng, 1), np.uint64)
        if ng:
            self.roff[1:] = np.cumsum(rowcap)[:-1]
            self.coff[1:] = np.cumsum(colcap)[:-1]
        res = {k: np.zeros(max(nt, 1), dt) for k, dt in self._TRACE}
        res.update({k: np.zeros(max(ng, 1), dt) for k, dt in self._GROUP})
        ctot = max(int(colcap.sum()), 1)
        res.update(rows=np.zeros(max(int(rowcap.sum()), 1), np.uint8), gapped=np.zeros(ctot, np.uint8),
                   cons=np.zeros(ctot, np.uint8), qual=np.zeros(ctot, np.uint8))
        self._bind_results(out, res)
        out.rows_offset = self.roff.ctypes.data_as(C.POINTER(C.c_uint64))
        out.col_offset = self.coff.ctypes.data_as(C.POINTER(C.c_uint64))

    def results(self):
        """per-trace and per-group arrays, and per group: rows (list of bytes, [] when nrows is 0), gapped, cons, qual (bytes)"""
        res, ng, nt = self.res, self.ng, self.nt
        out = {k: res[k][:nt].copy() for k, _ in self._TRACE}
        out.update({k: res[k][:ng].copy() for k, _ in self._GROUP})
        rows, gapped, cons, qual = [], [], [], []
        for g in range(ng):
            nr, nc, cl = int(res["nrows"][g]), int(res["ncol"][g]), int(res["cons_len"][g])
            ro, co = int(self.roff[g]), int(self.coff[g])
            rows.append([res["rows"][ro + i * nc:ro + (i + 1) * nc].tobytes() for i in range(nr)])
            gapped.append(res["gapped"][co:co + (nc if nr else 0)].tobytes())
            cons.append(res["cons"][co:co + (cl if nr else 0)].tobytes())
            qual.append(res["qual"][co:co + (cl if nr else 0)].tobytes())
        out.update(rows=rows, gapped=gapped, cons=cons, qual=qual)
        return out


class PreparedAssemble(_PreparedGroups):
    """host-buffer job / result structs of tracyhip_assemble_traces (everything they point to is kept alive by this object).
    groups: one list of float32 [6][len] trace profiles (trimmed, forward) per group; references: one float32 [6][len] profile per
    group, or fewer with ref_index."""

    _PAYLOADS = ("traces", "references")
    _TRACE = (("score_fwd", np.int32), ("score_rev", np.int32), ("forward", np.uint8), ("rank", np.uint32))

    def __init__(self, groups, references, params, match_fraction=0.5, fraction_called=0.1, include_reference=False, ref_index=None):
        pt, sums = self._pack_groups(groups)
        pr = references if isinstance(references, PackedSeqs) else PackedSeqs(references, SEQ_PROFILE)
        ridx = self.ridx = None if ref_index is None else np.ascontiguousarray(ref_index, dtype=np.uint32)
        self.keep = [pt, pr]
        job = self.job = AssembleJob()
        job.ngroups = self.ng
        job.traces = pt.seqset()
        job.group_first = self.first.ctypes.data_as(C.POINTER(C.c_uint32))
        job.references = pr.seqset()
        if ridx is not None:
            job.ref_index = ridx.ctypes.data_as(C.POINTER(C.c_uint32))
        job.match_fraction = float(match_fraction)
        job.fraction_called = float(fraction_called)
        job.include_reference = 1 if include_reference else 0
        # capacities (tracy_hip.h): (K + 1) * (n_ref + sum len) row bytes, n_ref + sum len columns
        bounds = []
        for g, s in enumerate(sums):
            r = g if ridx is None else int(ridx[g])
            n_ref = int(pr.length[r]) if r < pr.count else 0
            bounds.append((len(groups[g]) + 1, n_ref + s))
        self._bind_groups(AssembleResult(), bounds)
        self.prm = Params(*params) if len(params) == 6 else Params(params[0], params[1], params[2], params[3], 1, 0)


def _assemble_traces(self, groups, references, params, match_fraction=0.5, fraction_called=0.1, include_reference=False, ref_index=None,
                     device=False):
    """tracyhip_assemble_traces: the reference-guided chain of `tracy assemble -r` for a batch of trace groups.  params: (match,
    mismatch, go, ge) with the command's AlignConfig<true,false>, or all six tracyhip_params fields.  device=True: payloads and
    results in device memory (TRACYHIP_MEM_DEVICE), copied back afterwards."""
    p = PreparedAssemble(groups, references, params, match_fraction, fraction_called, include_reference, ref_index)
    return _run_prepared(self, "tracyhip_assemble_traces", p, device)


Context.assemble_traces = _assemble_traces


def _assemble_traces_async(self, job, prm, out, mem=MEM_HOST):
    """tracyhip_assemble_traces_async on prepared structs (PreparedAssemble: they, and everything they point to, must outlive
    synchronize())"""
    _check(lib().tracyhip_assemble_traces_async(self._h, C.byref(job), C.byref(prm), mem, C.byref(out)))


Context.assemble_traces_async = _assemble_traces_async


class DenovoJob(C.Structure):
    _fields_ = [("ngroups", C.c_uint32), ("traces", SeqSet), ("group_first", C.POINTER(C.c_uint32)), ("match_fraction", C.c_float),
                ("fraction_called", C.c_float)]


class DenovoResult(C.Structure):
    _fields_ = [("forward", C.c_void_p), ("partner", C.c_void_p), ("row", C.c_void_p), ("nrows", C.c_void_p), ("ncol", C.c_void_p),
                ("rows", C.c_void_p), ("gapped", C.c_void_p), ("cons", C.c_void_p), ("qual", C.c_void_p), ("cons_len", C.c_void_p),
                ("rows_offset", C.POINTER(C.c_uint64)), ("col_offset", C.POINTER(C.c_uint64))]


class PreparedDenovo(_PreparedGroups):
    """host-buffer job / result structs of tracyhip_denovo_traces (everything they point to is kept alive by this object).
    groups: one list of float32 [6][len] trace profiles (trimmed, forward) per group."""

    _PAYLOADS = ("traces",)
    _TRACE = (("forward", np.uint8), ("partner", np.uint32), ("row", np.uint32))

    def __init__(self, groups, params, match_fraction=0.5, fraction_called=0.1):
        pt, sums = self._pack_groups(groups)
        self.keep = [pt]
        job = self.job = DenovoJob()
        job.ngroups = self.ng
        job.traces = pt.seqset()
        job.group_first = self.first.ctypes.data_as(C.POINTER(C.c_uint32))
        job.match_fraction = float(match_fraction)
        job.fraction_called = float(fraction_called)
        # capacities (tracy_hip.h): K * sum len row bytes, sum len columns
        self._bind_groups(DenovoResult(), [(len(g), s) for g, s in zip(groups, sums)])
        self.prm = Params(*params) if len(params) == 6 else Params(params[0], params[1], params[2], params[3], 1, 1)


def _denovo_traces(self, groups, params, match_fraction=0.5, fraction_called=0.1, device=False):
    """tracyhip_denovo_traces: de novo `tracy assemble` (strands, overlap filter, UPGMA tree, consensus) for a batch of trace groups.
    params: (match, mismatch, go, ge) with the command's AlignConfig<true,true>, or all six tracyhip_params fields.  device=True:
    payloads and results in device memory (TRACYHIP_MEM_DEVICE), copied back afterwards."""
    p = PreparedDenovo(groups, params, match_fraction, fraction_called)
    return _run_prepared(self, "tracyhip_denovo_traces", p, device)


Context.denovo_traces = _denovo_traces


def _denovo_traces_async(self, job, prm, out, mem=MEM_HOST):
    """tracyhip_denovo_traces_async on prepared structs (PreparedDenovo: they, and everything they point to, must outlive
    synchronize())"""
    _check(lib().tracyhip_denovo_traces_async(self._h, C.byref(job), C.byref(prm), mem, C.byref(out)))


Context.denovo_traces_async = _denovo_traces_async


class RaggedSrc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("stride_bytes", C.c_uint64), ("elem_bytes", C.c_uint32), ("lens", C.c_void_p), ("lens_stride", C.c_uint32)]


def _pack_ragged_multi(self, kinds, n, out=None):
    """tracyhip_pack_ragged_multi on torch CUDA tensors.  kinds: [(src, stride in ELEMENTS, lens tensor (uint32 / int32), lens_stride)]:
    region i of a kind = `stride` elements of src from i * stride, of which the first lens[i * lens_stride] are used.  Returns (packed uint8
    tensor -- kind-major --, [bytes per kind]); `out`: a uint8 tensor of at least sum(n * stride * itemsize) bytes to pack into (kept by a
    caller that packs every step)."""
    import torch
    arr = (RaggedSrc * len(kinds))()
    cap = 0
    for k, (src, stride, lens, lens_stride) in enumerate(kinds):
        elem = src.element_size()
        arr[k] = RaggedSrc(src.data_ptr(), int(stride) * elem, elem, lens.data_ptr(), int(lens_stride))
        cap += int(n) * int(stride) * elem
    if out is None or out.numel() < cap:
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=kinds[0][0].device)
    kb = (C.c_uint64 * len(kinds))()
    _check(lib().tracyhip_pack_ragged_multi(self._h, arr, C.c_uint32(len(kinds)), C.c_uint32(int(n)), C.c_void_p(out.data_ptr()), C.c_uint64(out.numel()), kb))
    sizes = [int(x) for x in kb]
    return out[:sum(sizes)], sizes


def _pack_ragged(self, src, stride, lens, n=None, lens_stride=1, out=None):
    """one payload kind (tracyhip_pack_ragged): returns (packed uint8 tensor, bytes)"""
    if n is None:
        n = int(lens.numel()) // lens_stride
    packed, sizes = _pack_ragged_multi(self, [(src, stride, lens, lens_stride)], n, out)
    return packed, sizes[0]


Context.pack_ragged = _pack_ragged
Context.pack_ragged_multi = _pack_ragged_multi


def pair_bounds(len1, len2, idx1, idx2, parts):
    """tracyhip_pair_bounds: boundaries of `parts` contiguous slices of a pair list with (nearly) equal DP cell count.
    Pure host arithmetic inside the library (works without a GPU) -- the one rule used by device groups and by rank sharding."""
    len1 = np.ascontiguousarray(len1, dtype=np.uint32)
    len2 = np.ascontiguousarray(len2, dtype=np.uint32)
    idx1 = np.ascontiguousarray(idx1, dtype=np.uint32)
    idx2 = np.ascontiguousarray(idx2, dtype=np.uint32)
    pr = Pairs()
    pr.npairs = len(idx1)
    pr.a1 = SeqSet(SEQ_CHAR, None, None, len1.ctypes.data_as(C.POINTER(C.c_uint32)), len(len1))
    pr.a2 = SeqSet(SEQ_CHAR, None, None, len2.ctypes.data_as(C.POINTER(C.c_uint32)), len(len2))
    pr.a1_index = idx1.ctypes.data_as(C.POINTER(C.c_uint32))
    pr.a2_index = idx2.ctypes.data_as(C.POINTER(C.c_uint32))
    b = np.zeros(parts + 1, dtype=np.uint64)
    _check(lib().tracyhip_pair_bounds(C.byref(pr), C.c_uint32(parts), b.ctypes.data_as(C.POINTER(C.c_uint64))))
    return b.astype(np.int64)


class Group:
    """tracyhip_group: one context per listed device (a device may repeat), host buffers, one host thread per member"""

    def __init__(self, devices=None, ndevices=0):
        self._g = C.c_void_p()
        if devices is None:
            _check(lib().tracyhip_group_create(None, int(ndevices), C.byref(self._g)))
        else:
            arr = (C.c_int * len(devices))(*devices)
            _check(lib().tracyhip_group_create(arr, len(devices), C.byref(self._g)))

    def close(self):
        if self._g:
            lib().tracyhip_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return lib().tracyhip_group_size(self._g)

    def set_lanes(self, n):
        _check(lib().tracyhip_group_set_lanes(self._g, C.c_uint32(n)))

    def score(self, a1, a2, params, idx1=None, idx2=None):
        pr, keep, p1, p2 = Context._pairs(a1, a2, idx1, idx2)
        prm = Params(*params)
        out = np.zeros(max(pr.npairs, 1), dtype=np.int32)
        _check(lib().tracyhip_group_gotoh_score(self._g, C.byref(pr), C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out[:pr.npairs]


class KernelTiming(C.Structure):
    _fields_ = [("ms", C.c_double), ("launches", C.c_uint64), ("cells", C.c_uint64), ("bytes", C.c_uint64)]


# ---- allele deconvolution --------------------------------------------------------------------------
class Breakpoint(C.Structure):
    _fields_ = [("indelshift", C.c_int32), ("traceleft", C.c_int32), ("breakpoint", C.c_uint32), ("best_diff", C.c_float)]


class BaseCallsBatch(C.Structure):
    _fields_ = [("ntraces", C.c_uint32), ("signal", C.c_void_p), ("signal_offset", C.POINTER(C.c_uint64)),
                ("nsamples", C.POINTER(C.c_uint32)), ("bcpos", C.c_void_p), ("primary", C.c_void_p),
                ("secondary", C.c_void_p), ("bc_offset", C.POINTER(C.c_uint64)), ("bc_len", C.POINTER(C.c_uint32)),
                ("peaks", C.c_void_p)]  # (optional: the four channels at every basecall's peak position; None = built on the device)


class DecompParams(C.Structure):
    _fields_ = [("trim_left", C.c_int32), ("trim_right", C.c_int32), ("maxindel", C.c_int32), ("madc", C.c_int32)]


class DecompStatus(C.Structure):
    _fields_ = [("kind", C.c_int32), ("best_ins", C.c_int32), ("best_del", C.c_int32), ("best_fr", C.c_int32),
                ("dcp_n", C.c_uint32), ("pad", C.c_uint32)]


def _u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class HostBaseCalls:
    """pack lists of (signal [4][ns] int32, bcpos, primary, secondary) for the host-buffer entry points"""

    def __init__(self, signals, bcpos, primary, secondary):
        n = len(signals)
        self.n = n
        self.nsamples = np.array([s.shape[1] for s in signals], dtype=np.uint32)
        self.sig_off = np.zeros(max(n, 1), dtype=np.uint64)
        self.bc_len = np.array([len(p) for p in primary], dtype=np.uint32)
        self.bc_off = np.zeros(max(n, 1), dtype=np.uint64)
        so, bo = 0, 0
        for i in range(n):
            self.sig_off[i] = so
            so += 4 * int(self.nsamples[i])
            self.bc_off[i] = bo
            bo += int(self.bc_len[i])
        self.signal = np.concatenate([np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in signals]) if n else np.zeros(1, np.int32)
        self.bcpos = np.concatenate([np.ascontiguousarray(b, dtype=np.int32) for b in bcpos]) if n else np.zeros(1, np.int32)
        self.primary = np.frombuffer(b"".join(bytes(p) for p in primary), dtype=np.uint8).copy() if n else np.zeros(1, np.uint8)
        self.secondary = np.frombuffer(b"".join(bytes(p) for p in secondary), dtype=np.uint8).copy() if n else np.zeros(1, np.uint8)

    def peak_table(self):
        """tracyhip_basecalls::peaks of the batch: int32 [sum of bc_len][4] = the four channels at every basecall's peak position"""
        out = np.zeros((max(int(self.bc_len.sum()), 1), 4), dtype=np.int32)
        for i in range(self.n):
            so, ns, bo, bl = int(self.sig_off[i]), int(self.nsamples[i]), int(self.bc_off[i]), int(self.bc_len[i])
            sig = self.signal[so:so + 4 * ns].reshape(4, ns)
            out[bo:bo + bl] = sig[:, self.bcpos[bo:bo + bl]].T
        return out

    def struct(self, peaks_only=False):
        """peaks_only: the peak table instead of the chromatograms (signal / bcpos NULL)"""
        b = BaseCallsBatch()
        b.ntraces = self.n
        if peaks_only:
            self._peaks = self.peak_table()
            b.peaks = self._peaks.ctypes.data
            b.primary = self.primary.ctypes.data
            b.secondary = self.secondary.ctypes.data
            b.bc_offset = _u64p(self.bc_off)
            b.bc_len = _u32p(self.bc_len)
            return b
        b.signal = self.signal.ctypes.data
        b.signal_offset = _u64p(self.sig_off)
        b.nsamples = _u32p(self.nsamples)
        b.bcpos = self.bcpos.ctypes.data
        b.primary = self.primary.ctypes.data
        b.secondary = self.secondary.ctypes.data
        b.bc_offset = _u64p(self.bc_off)
        b.bc_len = _u32p(self.bc_len)
        return b

    def split(self, arr):
        return [arr[int(self.bc_off[i]):int(self.bc_off[i]) + int(self.bc_len[i])].tobytes() for i in range(self.n)]


def _find_breakpoint(self, profiles):
    pp = profiles if isinstance(profiles, PackedSeqs) else PackedSeqs(profiles, SEQ_PROFILE)
    out = (Breakpoint * max(pp.count, 1))()
    ss = pp.seqset()
    _check(lib().tracyhip_find_breakpoint(self._h, C.byref(ss), MEM_HOST, out))
    return [out[i] for i in range(pp.count)]


def _pack_rows(rows):
    n = len(rows)
    lens = np.array([len(r[0]) for r in rows], dtype=np.uint32)
    off = np.zeros(max(n, 1), dtype=np.uint64)
    if n:
        off[1:n] = np.cumsum(lens.astype(np.uint64))[:-1]
    r0 = np.frombuffer(b"".join(r[0] for r in rows) + b"\0", dtype=np.uint8).copy()
    r1 = np.frombuffer(b"".join(r[1] for r in rows) + b"\0", dtype=np.uint8).copy()
    return r0, r1, off, lens


def _find_homozygous_breakpoint(self, rows, bps):
    n = len(rows)
    r0, r1, off, lens = _pack_rows(rows)
    arr = (Breakpoint * max(n, 1))(*bps)
    status = np.zeros(max(n, 1), dtype=np.int32)
    _check(lib().tracyhip_find_homozygous_breakpoint(self._h, n, r0.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                     r1.ctypes.data_as(C.POINTER(C.c_uint8)), _u64p(off), _u32p(lens), MEM_HOST,
                                                     arr, status.ctypes.data_as(C.POINTER(C.c_int32))))
    return [arr[i] for i in range(n)], status[:n]


def _decompose_alleles(self, hbc, rows, bps, refslice_len, trim_left=50, trim_right=50, maxindel=1000, madc=5):
    n = hbc.n
    r0, r1, off, lens = _pack_rows(rows)
    arr = (Breakpoint * max(n, 1))(*bps)
    rl = np.ascontiguousarray(refslice_len, dtype=np.uint32)
    cap = 2 * maxindel + 2
    doff = (np.arange(max(n, 1), dtype=np.uint64) * np.uint64(cap))
    di = np.zeros(max(n, 1) * cap, dtype=np.int32)
    de = np.zeros(max(n, 1) * cap, dtype=np.int32)
    st = (DecompStatus * max(n, 1))()
    prm = DecompParams(trim_left, trim_right, maxindel, madc)
    b = hbc.struct()
    _check(lib().tracyhip_decompose_alleles(self._h, C.byref(b), r0.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            r1.ctypes.data_as(C.POINTER(C.c_uint8)), _u64p(off), _u32p(lens), arr, _u32p(rl),
                                            C.byref(prm), MEM_HOST, di.ctypes.data_as(C.POINTER(C.c_int32)),
                                            de.ctypes.data_as(C.POINTER(C.c_int32)), _u64p(doff), st))
    dcp = [[(int(di[i * cap + k]), int(de[i * cap + k])) for k in range(st[i].dcp_n)] for i in range(n)]
    status = [(st[i].kind, st[i].best_ins, st[i].best_del, st[i].best_fr) for i in range(n)]
    return hbc.split(hbc.primary), hbc.split(hbc.secondary), dcp, status


def _secondary_decomposed(self, hbc, peaks_only=False):
    out = np.zeros(max(len(hbc.primary), 1), dtype=np.uint8)
    b = hbc.struct(peaks_only)
    _check(lib().tracyhip_secondary_decomposed(self._h, C.byref(b), MEM_HOST, out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def _allelic_fraction(self, hbc, secdecomp, trim_left=50, trim_right=50, peaks_only=False):
    fr = np.zeros(2 * max(hbc.n, 1), dtype=np.float64)
    b = hbc.struct(peaks_only)
    sd = np.ascontiguousarray(secdecomp, dtype=np.uint8)
    _check(lib().tracyhip_allelic_fraction(self._h, C.byref(b), sd.ctypes.data_as(C.POINTER(C.c_uint8)), trim_left, trim_right,
                                           MEM_HOST, fr.ctypes.data_as(C.POINTER(C.c_double))))
    return fr[:2 * hbc.n].reshape(-1, 2)


Context.find_breakpoint = _find_breakpoint
Context.find_homozygous_breakpoint = _find_homozygous_breakpoint
Context.decompose_alleles = _decompose_alleles
Context.secondary_decomposed = _secondary_decomposed
Context.allelic_fraction = _allelic_fraction


class DecomposeJob(C.Structure):
    _fields_ = [("ntraces", C.c_uint32), ("profiles", SeqSet), ("bc", BaseCallsBatch), ("refs", SeqSet),
                ("ref_index", C.POINTER(C.c_uint32)), ("dprm", DecompParams), ("oriented", C.POINTER(C.c_uint8)), ("ref_profiles", SeqSet),
                ("strand_by_certificate", C.c_uint32), ("trim_left_each", C.POINTER(C.c_uint32)),
                ("trim_right_each", C.POINTER(C.c_uint32))]


class DecomposeResult(C.Structure):
    _fields_ = [("bp", C.c_void_p), ("status", C.c_void_p), ("score_fwd", C.c_void_p), ("score_rev", C.c_void_p),
                ("forward", C.c_void_p), ("score_trim", C.c_void_p), ("dcp_indel", C.c_void_p), ("dcp_err", C.c_void_p),
                ("dcp_offset", C.POINTER(C.c_uint64)), ("dstatus", C.c_void_p), ("secdecomp", C.c_void_p),
                ("fractions", C.c_void_p), ("slice_begin", C.c_void_p * 2), ("slice_len", C.c_void_p * 2),
                ("ref_pos", C.c_void_p * 2), ("score", C.c_void_p * 3), ("ops", C.c_void_p * 3),
                ("ops_offset", C.POINTER(C.c_uint64) * 3), ("ops_len", C.c_void_p * 3)]


class DecomposeOutcome(dict):
    """what Context.decompose_traces returns: the result arrays by name; `call` keeps the job / result structs of the call alive for
    Context.decompose_variants"""
    call = None

    def device_tensor(self, key):
        """result array `key` as a call with device_bc left it on the device: the uint8 tensor the host copy was read from (None for a
        call with host buffers).  Context.render_decompositions takes the decomposition tables from here."""
        host = self.call["keep"][10][key]
        addr = C.addressof(host) if isinstance(host, C.Array) else host.ctypes.data
        return next((t for t, a, _ in self.call["keep"][8] if a == addr), None)


def _decompose_traces(self, profiles, hbc, refs, params, trim_left=50, trim_right=50, maxindel=1000, madc=5, oriented=None,
                      ref_profiles=None, exact_scores=True, peaks_only=False, device_bc=None, ref_index=None):
    """tracyhip_decompose_traces with host buffers; hbc: HostBaseCalls (primary/secondary rewritten in place);
    oriented: None, or rs.forward per trace when the references are already oriented (indexed-genome path).
    trim_left / trim_right: ints, or per-trace array-likes (Context.decompose_variants reads them from the job this call keeps).
    ref_profiles: wildtype-trace references, parallel to refs (the wildtypes' primary calls); without `oriented` the call chooses the strand.
    ref_index: reference (and wildtype profile) of every trace, for shared references; None = identity.
    device_bc: a PreparedBasecall(device=True) that has run -- profiles, basecalls and peak table are taken from its device tensors as they
    stand (profiles and hbc may be None), references and results live on the device too (TRACYHIP_MEM_DEVICE) and are copied back."""
    dev = device_bc is not None
    mirrors = []
    pp = prp = d_refs = None
    if dev:
        import torch

    def put(holder, key, buf):  # a result array: the host buffer, or with device_bc its mirror on the device
        addr = C.addressof(buf) if isinstance(buf, C.Array) else buf.ctypes.data
        if dev:
            nbytes = C.sizeof(buf) if isinstance(buf, C.Array) else buf.nbytes
            t = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
            mirrors.append((t, addr, nbytes))
            addr = t.data_ptr()
        if isinstance(key, int):
            holder[key] = addr
        else:
            setattr(holder, key, addr)

    pr = refs if isinstance(refs, PackedSeqs) else PackedSeqs(refs, SEQ_CHAR)
    job = DecomposeJob()
    if dev:
        nt = device_bc.nt
        job.profiles = device_bc.profiles_seqset()
        job.bc = device_bc.basecalls_struct(peaks_only=True)
        d_refs = torch.from_numpy(pr.data).cuda()
        job.refs = pr.seqset(d_refs.data_ptr())
        mf = device_bc.meta["bc_len"][:nt].astype(np.uint64)
        nbases = device_bc.total
    else:
        pp = profiles if isinstance(profiles, PackedSeqs) else PackedSeqs(profiles, SEQ_PROFILE)
        nt = pp.count
        job.profiles = pp.seqset()
        job.bc = hbc.struct(peaks_only)  # (peaks_only: the peak table instead of the chromatograms, tracyhip_basecalls::peaks)
        job.refs = pr.seqset()
        mf = pp.length[:nt].astype(np.uint64)
        nbases = len(hbc.primary)
    job.ntraces = nt
    job.dprm = DecompParams(0, 0, maxindel, madc)
    trim_arrays = trims_each(job, trim_left, trim_right, nt)
    job.strand_by_certificate = 0 if exact_scores else 1  # opt-in: the losing strand may carry a certified upper bound
    if oriented is not None:
        oriented = np.ascontiguousarray(oriented, dtype=np.uint8)
        job.oriented = oriented.ctypes.data_as(C.POINTER(C.c_uint8))
    if ref_profiles is not None:
        # wildtype-trace reference: profiles parallel to refs (= the wildtypes' primary calls).  With `oriented` both are already oriented;
        # without, both are the FORWARD wildtype and the call chooses the strand (score_fwd / score_rev / forward are filled)
        prp = ref_profiles if isinstance(ref_profiles, PackedSeqs) else PackedSeqs(ref_profiles, SEQ_PROFILE)
        if dev:
            d_refprof = torch.from_numpy(prp.data).cuda()
            d_refs = (d_refs, d_refprof)  # (kept alive by the returned call)
            job.ref_profiles = prp.seqset(d_refprof.data_ptr())
        else:
            job.ref_profiles = prp.seqset()
    cap = 2 * maxindel + 2
    doff = np.arange(max(nt, 1), dtype=np.uint64) * np.uint64(cap)
    if ref_index is not None:
        ref_index = np.ascontiguousarray(ref_index, dtype=np.uint32)
        job.ref_index = ref_index.ctypes.data_as(C.POINTER(C.c_uint32))
        rn = pr.length[ref_index].astype(np.uint64)
    else:
        rn = pr.length[:nt].astype(np.uint64)
    res = {
        "bp": (Breakpoint * max(nt, 1))(), "status": np.zeros(max(nt, 1), np.int32),
        "score_fwd": np.zeros(max(nt, 1), np.int32), "score_rev": np.zeros(max(nt, 1), np.int32),
        "forward": np.zeros(max(nt, 1), np.uint8), "score_trim": np.zeros(max(nt, 1), np.int32),
        "dcp_indel": np.zeros(max(nt, 1) * cap, np.int32), "dcp_err": np.zeros(max(nt, 1) * cap, np.int32),
        "dstatus": (DecompStatus * max(nt, 1))(), "secdecomp": np.zeros(max(nbases, 1), np.uint8),
        "fractions": np.zeros(2 * max(nt, 1), np.float64),
    }
    out = DecomposeResult()
    for k in ("bp", "dstatus", "status", "score_fwd", "score_rev", "forward", "score_trim", "dcp_indel", "dcp_err", "secdecomp", "fractions"):
        put(out, k, res[k])
    out.dcp_offset = _u64p(doff)
    keep = []
    for k in range(3):
        caps = (mf + (rn if k < 2 else mf)).astype(np.uint64)
        off = np.zeros(max(nt, 1), dtype=np.uint64)
        if nt:
            off[1:nt] = np.cumsum(caps)[:-1]
        ops = np.zeros(max(int(caps.sum()), 1), np.uint8)
        olen = np.zeros(max(nt, 1), np.uint32)
        sc = np.zeros(max(nt, 1), np.int32)
        put(out.score, k, sc)
        put(out.ops, k, ops)
        out.ops_offset[k] = _u64p(off)
        put(out.ops_len, k, olen)
        res["score%d" % k] = sc
        keep.append((off, ops, olen))
        if k < 2:
            for nm in ("slice_begin", "slice_len", "ref_pos"):
                a = np.zeros(max(nt, 1), np.uint32)
                put(getattr(out, nm), k, a)
                res["%s%d" % (nm, k)] = a
    prm = Params(params[0], params[1], params[2], params[3], 1, 0)
    if dev:
        torch.cuda.synchronize()
        _check(lib().tracyhip_decompose_traces(self._h, C.byref(job), C.byref(prm), MEM_DEVICE, C.byref(out)))
        torch.cuda.synchronize()
        for t, addr, nbytes in mirrors:
            h = t.cpu().numpy()  # (held while its bytes are copied)
            C.memmove(addr, h.ctypes.data, nbytes)
    elif isinstance(self, Group):
        _check(lib().tracyhip_group_decompose_traces(self._g, C.byref(job), C.byref(prm), C.byref(out)))
    else:
        _check(lib().tracyhip_decompose_traces(self._h, C.byref(job), C.byref(prm), MEM_HOST, C.byref(out)))
    for k in range(3):
        off, ops, olen = keep[k]
        res["btr%d" % k] = [ops[int(off[i]):int(off[i]) + int(olen[i])].tobytes() for i in range(nt)]
    res["dcp"] = [[(int(res["dcp_indel"][i * cap + j]), int(res["dcp_err"][i * cap + j])) for j in range(res["dstatus"][i].dcp_n)]
                  for i in range(nt)]
    res = DecomposeOutcome(res)
    # what Context.decompose_variants needs of this call: the structs and everything they point to
    res.call = dict(job=job, out=out, prm=prm, mem=MEM_DEVICE if dev else MEM_HOST, nt=nt,
                    keep=(pr, pp, prp, d_refs, hbc, doff, keep, oriented, mirrors, device_bc, dict(res), trim_arrays, ref_index))
    if dev:  # the decomposed basecalls as the call left them in the device tensors
        rows = device_bc.results(fill_deferred=False)
        res["primary"] = [r["primary"] for r in rows]
        res["secondary"] = [r["secondary"] for r in rows]
        res["secdecomp_list"] = [res["secdecomp"][int(device_bc.pos_off[i]):int(device_bc.pos_off[i]) + rows[i]["bc_len"]].tobytes() for i in range(nt)]
        return res
    res["primary"] = hbc.split(hbc.primary)
    res["secondary"] = hbc.split(hbc.secondary)
    res["secdecomp_list"] = hbc.split(res["secdecomp"])
    return res


Context.decompose_traces = _decompose_traces
Context.align_banded = _align_banded


# ---- variant calling of `tracy decompose -v` (tracyhip_call_variants / tracyhip_decompose_variants) ------------------------------
class Variant(C.Structure):
    _fields_ = [("pos", C.c_int32), ("basenum", C.c_int32), ("gt", C.c_int32), ("call_index", C.c_uint32), ("ref_off", C.c_uint32),
                ("ref_len", C.c_uint32), ("alt_off", C.c_uint32), ("alt_len", C.c_uint32)]


VARIANT_DTYPE = np.dtype([(n, "<i4" if t is C.c_int32 else "<u4") for n, t in Variant._fields_])


class VariantsResult(C.Structure):
    _fields_ = [("var", C.c_void_p), ("text", C.c_void_p), ("var_n", C.c_void_p), ("var_flags", C.c_void_p),
                ("max_variants", C.c_uint32), ("max_text", C.c_uint32)]


class VariantBuffers:
    """the four result arrays of the two variant calls for nt traces, on the host or (device=True) in torch tensors, filled with `fill` so
    that what a call leaves alone can be told; lists() decodes them"""

    def __init__(self, nt, max_variants, max_text, device=False, fill=0):
        self.nt, self.max_variants, self.max_text, self.device = nt, max_variants, max_text, device
        shapes = (("var", max(nt, 1) * max_variants * VARIANT_DTYPE.itemsize), ("text", max(nt, 1) * max_text), ("var_n", max(nt, 1) * 4),
                  ("var_flags", max(nt, 1) * 4))
        if device:
            import torch
            self.t = {k: torch.full((n,), fill, dtype=torch.uint8, device="cuda") for k, n in shapes}
            torch.cuda.synchronize()
            ptr = {k: v.data_ptr() for k, v in self.t.items()}
        else:
            self.h = {k: np.full(n, fill, np.uint8) for k, n in shapes}
            ptr = {k: v.ctypes.data for k, v in self.h.items()}
        self.struct = VariantsResult(ptr["var"], ptr["text"], ptr["var_n"], ptr["var_flags"], max_variants, max_text)

    def arrays(self):
        """(records [nt][max_variants], text [nt][max_text], var_n, var_flags) as numpy arrays on the host"""
        if self.device:
            import torch
            torch.cuda.synchronize()
            self.h = {k: v.cpu().numpy() for k, v in self.t.items()}
        n = max(self.nt, 1)
        return (self.h["var"].view(VARIANT_DTYPE).reshape(n, self.max_variants), self.h["text"].reshape(n, self.max_text),
                self.h["var_n"].view(np.uint32), self.h["var_flags"].view(np.uint32))

    def lists(self):
        """per trace the list of dict(pos, basenum, gt, ref, alt, call_index), and the flags"""
        rec, text, n, flags = self.arrays()
        out = []
        for t in range(self.nt):
            out.append([dict(pos=int(r["pos"]), basenum=int(r["basenum"]), gt=int(r["gt"]),
                             ref=text[t, int(r["ref_off"]):int(r["ref_off"]) + int(r["ref_len"])].tobytes(),
                             alt=text[t, int(r["alt_off"]):int(r["alt_off"]) + int(r["alt_len"])].tobytes(), call_index=int(r["call_index"]))
                        for r in rec[t, :int(n[t])]])
        return out, flags[:self.nt].copy()


def _call_variants(self, rows, pos, forward, bc_len, trim_left=50, trim_right=50, max_variants=256, max_text=4096, device=False, buffers=None):
    """tracyhip_call_variants: rows = (row0, row1) of 2 * ntraces alignments (2t, 2t + 1: the alleles of trace t), pos = rs.pos of each,
    forward / bc_len per trace.  Returns (per trace the list of dict(pos, basenum, gt, ref, alt, call_index), flags); device=True: rows
    and results live in device memory (TRACYHIP_MEM_DEVICE)."""
    nt = len(forward)
    assert len(rows) == 2 * nt and len(pos) == 2 * nt and len(bc_len) == nt
    r0, r1, off, lens = _pack_rows(rows)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    fwd = np.ascontiguousarray(forward, dtype=np.uint8)
    bl = np.ascontiguousarray(bc_len, dtype=np.uint32)
    b = buffers if buffers is not None else VariantBuffers(nt, max_variants, max_text, device)
    p0, p1 = r0.ctypes.data, r1.ctypes.data
    if device:
        import torch
        d0, d1 = torch.from_numpy(r0).cuda(), torch.from_numpy(r1).cuda()
        torch.cuda.synchronize()
        p0, p1 = d0.data_ptr(), d1.data_ptr()
    s = b.struct
    _check(lib().tracyhip_call_variants(self._h, C.c_uint32(nt), C.c_void_p(p0), C.c_void_p(p1), _u64p(off), _u32p(lens),
                                        pos.ctypes.data_as(C.POINTER(C.c_int32)), fwd.ctypes.data_as(C.POINTER(C.c_uint8)), _u32p(bl),
                                        C.c_uint32(trim_left), C.c_uint32(trim_right), C.c_uint32(s.max_variants), C.c_uint32(s.max_text),
                                        MEM_DEVICE if device else MEM_HOST, C.c_void_p(s.var), C.c_void_p(s.text), C.c_void_p(s.var_n),
                                        C.c_void_p(s.var_flags)))
    return b.lists()


def _decompose_variants(self, outcome, slice_pos=None, max_variants=256, max_text=4096, buffers=None):
    """tracyhip_decompose_variants on what Context.decompose_traces returned (host buffers, or device payloads when that call ran with
    device_bc): per trace the list of dict(pos, basenum, gt, ref, alt, call_index), and the flags (bit 0: truncated).  slice_pos: rs.pos of
    every trace's reference window (None: zeros, a single FASTA)."""
    c = outcome.call
    nt = c["nt"]
    sp = np.zeros(max(nt, 1), np.uint32) if slice_pos is None else np.ascontiguousarray(slice_pos, dtype=np.uint32)
    b = buffers if buffers is not None else VariantBuffers(nt, max_variants, max_text, c["mem"] == MEM_DEVICE)
    _check(lib().tracyhip_decompose_variants(self._h, C.byref(c["job"]), C.byref(c["out"]), _u32p(sp), C.byref(c["prm"]), c["mem"],
                                             C.byref(b.struct)))
    return b.lists()


def _decompose_variants_async(self, job, res, slice_pos, prm, out, mem=MEM_HOST):
    """tracyhip_decompose_variants_async on prepared structs (they, and everything they point to, must outlive Context.synchronize();
    slice_pos is copied by the call)"""
    _check(lib().tracyhip_decompose_variants_async(self._h, C.byref(job), C.byref(res), _u32p(slice_pos), C.byref(prm), mem, C.byref(out)))


def decompose_variants_validate(job, res, slice_pos, prm, out, mem=MEM_HOST):
    """tracyhip_decompose_variants_validate: the argument checks of the call (no device needed); raises TracyHipError"""
    _check(lib().tracyhip_decompose_variants_validate(C.byref(job) if job is not None else None, C.byref(res) if res is not None else None,
                                                      _u32p(slice_pos) if slice_pos is not None else None,
                                                      C.byref(prm) if prm is not None else None, mem, C.byref(out) if out is not None else None))


Context.call_variants = _call_variants
Context.decompose_variants = _decompose_variants
Context.decompose_variants_async = _decompose_variants_async
Group.align_traces = _align_traces
Group.decompose_traces = _decompose_traces


# ---- k-mer seeding in an indexed genome on the device (tracyhip_genome_upload / tracyhip_seed_traces) ----------------------------
SEED_UNANCHORED, SEED_ANCHORED, SEED_DEFERRED = 0, 1, 2


class GenomeDesc(C.Structure):
    _fields_ = [("k", C.c_uint32), ("bucket_bits", C.c_uint32), ("dir", C.c_void_p), ("tab", C.c_void_p), ("ntab", C.c_uint64),
                ("text", C.c_void_p), ("text_len", C.c_uint64), ("starts", C.c_void_p), ("lengths", C.c_void_p), ("ncontigs", C.c_uint32),
                ("contig_id", C.c_void_p)]


class SeedParams(C.Structure):
    _fields_ = [("trim_left", C.c_uint32), ("trim_right", C.c_uint32), ("kmer", C.c_uint32), ("min_support", C.c_uint32),
                ("maxindel", C.c_uint32), ("trim_left_each", C.POINTER(C.c_uint32)), ("trim_right_each", C.POINTER(C.c_uint32))]


class SeedResult(C.Structure):
    _fields_ = [("status", C.c_void_p), ("forward", C.c_void_p), ("kmersupport", C.c_void_p), ("pos", C.c_void_p), ("contig", C.c_void_p),
                ("slice_len", C.c_void_p), ("slices", C.c_void_p), ("slice_cap", C.c_uint64)]


def genome_validate(desc):
    """tracyhip_genome_validate: host-side check of an index descriptor (no device needed); raises TracyHipError"""
    _check(lib().tracyhip_genome_validate(C.byref(desc)))


def genome_upload(ctx, desc):
    """tracyhip_genome_upload -> handle (c_void_p); the descriptor's arrays are copied once"""
    h = C.c_void_p()
    _check(lib().tracyhip_genome_upload(ctx._h, C.byref(desc), C.byref(h)))
    return h


def genome_free(h):
    if h:
        lib().tracyhip_genome_free(h)


def genome_bytes(h):
    fn = lib().tracyhip_genome_bytes
    fn.restype = C.c_uint64
    return int(fn(h))


def seed_traces(ctx, genome_h, seqset, params, mem, result):
    """tracyhip_seed_traces on prepared structs"""
    _check(lib().tracyhip_seed_traces(ctx._h, genome_h, C.byref(seqset), C.byref(params), int(mem), C.byref(result)))


def genome_validate_text(desc):
    """tracyhip_genome_validate_text: host-side check of a descriptor a table is to be built from (no device needed); raises TracyHipError"""
    _check(lib().tracyhip_genome_validate_text(C.byref(desc)))


def genome_build(ctx, desc):
    """tracyhip_genome_build -> handle (c_void_p): the text and contigs copied once, dir and tab built on the device"""
    h = C.c_void_p()
    _check(lib().tracyhip_genome_build(ctx._h, C.byref(desc), C.byref(h)))
    return h


def genome_ntab(h):
    n = C.c_uint64()
    _check(lib().tracyhip_genome_ntab(h, C.byref(n)))
    return int(n.value)


def genome_download(h, bucket_bits):
    """tracyhip_genome_download -> (dir uint64 [2^bits + 1], tab uint64 [ntab][2]) as numpy arrays"""
    d = np.empty((1 << bucket_bits) + 1, dtype=np.uint64)
    t = np.empty((genome_ntab(h), 2), dtype=np.uint64)
    _check(lib().tracyhip_genome_download(h, C.c_void_p(d.ctypes.data), C.c_void_p(t.ctypes.data if t.size else 0)))
    return d, t


# ---- basecalling of raw chromatograms on the device (tracyhip_basecall_traces) -------------------------------------------------------
BASECALL_OK, BASECALL_DEFERRED = 0, 1


class BasecallJob(C.Structure):
    _fields_ = [("ntraces", C.c_uint32), ("signal", C.c_void_p), ("signal_offset", C.POINTER(C.c_uint64)), ("nsamples", C.POINTER(C.c_uint32)),
                ("sample_bytes", C.c_uint32), ("basecallpos", C.c_void_p), ("pos_offset", C.POINTER(C.c_uint64)), ("npos", C.POINTER(C.c_uint32)),
                ("sigratio", C.c_float), ("trim_stringency", C.c_float)]


class BasecallResult(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("bc_len", C.POINTER(C.c_uint32)), ("trim_left", C.POINTER(C.c_uint32)),
                ("trim_right", C.POINTER(C.c_uint32)), ("best_section", C.POINTER(C.c_uint32)), ("primary", C.c_void_p), ("secondary", C.c_void_p),
                ("consensus", C.c_void_p), ("bcpos", C.c_void_p), ("estqual", C.c_void_p), ("peaks", C.c_void_p), ("profiles", C.c_void_p)]


_BC_PAYLOADS = (("primary", np.uint8, 1), ("secondary", np.uint8, 1), ("consensus", np.uint8, 1), ("bcpos", np.int32, 1), ("estqual", np.uint8, 1),
                ("peaks", np.int32, 4), ("profiles", np.float32, 6))


class PreparedBasecall:
    """job / result structs of tracyhip_basecall_traces over packed signals (int32 or int16 [4][ns] per trace) and call positions; with
    device=True the payloads are torch tensors on the GPU and stay there: profiles_seqset() / basecalls_struct() hand them to the align,
    consensus and decompose jobs without a host copy.  Everything the structs point to is kept alive by this object."""

    def __init__(self, signals, positions, sigratio=0.33, trim_stringency=0, device=False, sample_dtype=None):
        if isinstance(signals, PreparedRead):
            self._from_read(signals, sigratio, trim_stringency)
            return
        nt = self.nt = len(signals)
        if sample_dtype is None:
            sample_dtype = np.int16 if nt and all(np.asarray(s).dtype == np.int16 for s in signals) else np.int32
        self.sample_dtype = np.dtype(sample_dtype)
        self.device = device
        self.nsamples = np.array([np.asarray(s).shape[1] for s in signals] + [0], dtype=np.uint32)[:max(nt, 1)]
        self.npos = np.array([len(p) for p in positions] + [0], dtype=np.uint32)[:max(nt, 1)]
        self.sig_off = np.zeros(max(nt, 1), np.uint64)
        self.pos_off = np.zeros(max(nt, 1), np.uint64)
        if nt:
            self.sig_off[1:nt] = np.cumsum(4 * self.nsamples[:nt].astype(np.uint64))[:-1]
            self.pos_off[1:nt] = np.cumsum(self.npos[:nt].astype(np.uint64))[:-1]
        self.signal = (np.concatenate([np.ascontiguousarray(s, dtype=self.sample_dtype).reshape(-1) for s in signals])
                       if nt else np.zeros(1, self.sample_dtype))
        self.positions = np.concatenate([np.ascontiguousarray(p, dtype=np.int32) for p in positions] + [np.zeros(1, np.int32)])
        total = self.total = int(self.npos[:nt].sum()) if nt else 0
        self.meta = {k: np.zeros(max(nt, 1), np.int32 if k == "status" else np.uint32)
                     for k in ("status", "bc_len", "trim_left", "trim_right", "best_section")}
        job = self.job = BasecallJob()
        job.ntraces = nt
        job.signal_offset, job.nsamples = _u64p(self.sig_off), _u32p(self.nsamples)
        job.pos_offset, job.npos = _u64p(self.pos_off), _u32p(self.npos)
        job.sample_bytes = self.sample_dtype.itemsize
        job.sigratio = sigratio
        job.trim_stringency = trim_stringency
        out = self.out = BasecallResult()
        out.status = self.meta["status"].ctypes.data_as(C.POINTER(C.c_int32))
        for k in ("bc_len", "trim_left", "trim_right", "best_section"):
            setattr(out, k, _u32p(self.meta[k]))
        if device:
            import torch
            self.d_signal = torch.from_numpy(self.signal).cuda()
            self.d_positions = torch.from_numpy(self.positions).cuda()
            self.payload = {k: torch.zeros(max(total, 1) * w, dtype=getattr(torch, np.dtype(dt).name), device="cuda") for k, dt, w in _BC_PAYLOADS}
            job.signal, job.basecallpos = self.d_signal.data_ptr(), self.d_positions.data_ptr()
            for k, _, _ in _BC_PAYLOADS:
                setattr(out, k, self.payload[k].data_ptr())
            torch.cuda.synchronize()
        else:
            self.payload = {k: np.zeros(max(total, 1) * w, dt) for k, dt, w in _BC_PAYLOADS}
            job.signal, job.basecallpos = self.signal.ctypes.data, self.positions.ctypes.data
            for k, _, _ in _BC_PAYLOADS:
                setattr(out, k, self.payload[k].ctypes.data)
        self.mem = MEM_DEVICE if device else MEM_HOST

    def _from_read(self, rd, sigratio, trim_stringency):
        """over the results of a PreparedRead(device=True) that has run with payload results: its chromatograms and positions are the job's
        signal and basecallpos as they stand (signal_offset = sample_offset, pos_offset = call_offset, npos = ncalls); no payload is
        copied.  A trace the reader deferred has no samples and no positions here: the call defers it too."""
        import torch
        if not rd.device or rd.o is None:
            raise ValueError("basecall_traces: a PreparedRead(device=True) with payload results")
        nt = self.nt = rd.nt
        self.read = rd
        self.device = True
        self.sample_dtype = rd.sample_dtype
        self.nsamples, self.npos = rd.meta["nsamples"], rd.meta["ncalls"]
        self.sig_off, self.pos_off = rd.o["sample_offset"], rd.o["call_offset"]
        self.d_signal, self.d_positions = rd.o["signal"], rd.o["basecallpos"]
        self.signal = self.positions = None  # (on the device only: results() fetches them when a deferred trace needs the host chain)
        total = self.total = int(rd.o["call_offset"][nt])
        self.meta = {k: np.zeros(max(nt, 1), np.int32 if k == "status" else np.uint32)
                     for k in ("status", "bc_len", "trim_left", "trim_right", "best_section")}
        job = self.job = BasecallJob()
        job.ntraces = nt
        job.signal_offset, job.nsamples = _u64p(self.sig_off), _u32p(self.nsamples)
        job.pos_offset, job.npos = _u64p(self.pos_off), _u32p(self.npos)
        job.sample_bytes = self.sample_dtype.itemsize
        job.sigratio = sigratio
        job.trim_stringency = trim_stringency
        out = self.out = BasecallResult()
        out.status = self.meta["status"].ctypes.data_as(C.POINTER(C.c_int32))
        for k in ("bc_len", "trim_left", "trim_right", "best_section"):
            setattr(out, k, _u32p(self.meta[k]))
        self.payload = {k: torch.zeros(max(total, 1) * w, dtype=getattr(torch, np.dtype(dt).name), device="cuda") for k, dt, w in _BC_PAYLOADS}
        job.signal, job.basecallpos = self.d_signal.data_ptr(), self.d_positions.data_ptr()
        for k, _, _ in _BC_PAYLOADS:
            setattr(out, k, self.payload[k].data_ptr())
        torch.cuda.synchronize()
        self.mem = MEM_DEVICE

    def run(self, ctx, asynchronous=False):
        fn = lib().tracyhip_basecall_traces_async if asynchronous else lib().tracyhip_basecall_traces
        _check(fn(ctx._h, C.byref(self.job), self.mem, C.byref(self.out)))
        return self

    def profiles_seqset(self):
        """the `profiles` set of AlignJob / ConsensusJob / DecomposeJob: trace t = bc_len[t] columns at 6 * pos_offset[t]"""
        self._prof_off = (6 * self.pos_off).astype(np.uint64)
        s = SeqSet()
        s.kind = SEQ_PROFILE
        s.data = self.payload["profiles"].data_ptr() if self.device else self.payload["profiles"].ctypes.data
        s.offset, s.length, s.count = _u64p(self._prof_off), _u32p(self.meta["bc_len"]), self.nt
        return s

    def trims(self):
        """(trim_left, trim_right) of a finished run as the per-trace arrays Context.align_traces, PreparedAlign and
        Context.decompose_traces take for their trims: the chain signals -> basecalls -> alignments with a trim stringency set"""
        return self.meta["trim_left"][:self.nt].copy(), self.meta["trim_right"][:self.nt].copy()

    def basecalls_struct(self, peaks_only=True):
        """tracyhip_basecalls of the batch (bcpos / primary / secondary / the peak table as the call left them)"""
        ptr = (lambda a: a.data_ptr()) if self.device else (lambda a: a.ctypes.data)
        b = BaseCallsBatch()
        b.ntraces = self.nt
        if not peaks_only:
            b.signal = ptr(self.d_signal if self.device else self.signal)
            if self.sample_dtype != np.int32:
                raise ValueError("tracyhip_basecalls::signal holds int32 samples: pass peaks_only=True")
            b.signal_offset, b.nsamples = _u64p(self.sig_off), _u32p(self.nsamples)
            b.bcpos = ptr(self.payload["bcpos"])
        b.primary, b.secondary, b.peaks = ptr(self.payload["primary"]), ptr(self.payload["secondary"]), ptr(self.payload["peaks"])
        b.bc_offset, b.bc_len = _u64p(self.pos_off), _u32p(self.meta["bc_len"])
        return b

    def results(self, fill_deferred=True):
        """per trace: dict of numpy views (device payloads are copied back); deferred traces are filled in from the host chain, except those
        with a position outside their chromatogram (`unreadable`: status stays DEFERRED, bc_len 0)"""
        from . import hostlib
        pay = {k: (v.cpu().numpy() if self.device else v) for k, v in self.payload.items()}
        if self.signal is None and fill_deferred and (self.meta["status"][:self.nt] == BASECALL_DEFERRED).any():
            self.signal, self.positions = self.d_signal.cpu().numpy(), self.d_positions.cpu().numpy()
        out = []
        for t in range(self.nt):
            o, n = int(self.pos_off[t]), int(self.meta["bc_len"][t])
            r = dict(status=int(self.meta["status"][t]), bc_len=n, trim_left=int(self.meta["trim_left"][t]),
                     trim_right=int(self.meta["trim_right"][t]), best_section=int(self.meta["best_section"][t]))
            if r["status"] == BASECALL_DEFERRED and fill_deferred:
                ns = int(self.nsamples[t])
                sig = self.signal[int(self.sig_off[t]):int(self.sig_off[t]) + 4 * ns].reshape(4, ns).astype(np.int32)
                pos = self.positions[o:o + int(self.npos[t])]
                if len(pos) and (int(pos.min()) < 0 or int(pos.max()) >= ns):  # the reference indexes the chromatogram unchecked: nobody can call these
                    r.update(unreadable=True, primary=b"", secondary=b"", consensus=b"", bcpos=pos[:0], estqual=np.zeros(0, np.uint8),
                             peaks=np.zeros((0, 4), np.int32), profile=np.zeros((6, 0), np.float32))
                    out.append(r)
                    continue
                pri, sec, con, bcpos, q = hostlib.basecall_qual(sig, pos, self.job.sigratio)
                s = float(self.job.trim_stringency)
                tl, tr = hostlib.trim_trace(sig, pos, self.job.sigratio, min(max(s, 1.0), 9.0)) if s else (0, 0)
                r.update(bc_len=len(pri), trim_left=tl & 0xFFFF, trim_right=tr & 0xFFFF, best_section=None, primary=pri, secondary=sec, consensus=con,
                         bcpos=bcpos, estqual=q, peaks=np.ascontiguousarray(sig[:, bcpos].T) if len(pri) else np.zeros((0, 4), np.int32),
                         profile=hostlib.create_profile(sig, bcpos, pri, sec) if len(pri) else np.zeros((6, 0), np.float32))
            else:
                r.update(primary=pay["primary"][o:o + n].tobytes(), secondary=pay["secondary"][o:o + n].tobytes(),
                         consensus=pay["consensus"][o:o + n].tobytes(), bcpos=pay["bcpos"][o:o + n], estqual=pay["estqual"][o:o + n],
                         peaks=pay["peaks"][4 * o:4 * (o + n)].reshape(n, 4), profile=pay["profiles"][6 * o:6 * (o + n)].reshape(6, n))
            out.append(r)
        return out


def _basecall_traces(self, signals, positions=None, sigratio=0.33, trim_stringency=0, device=False):
    """tracyhip_basecall_traces.  signals may be the PreparedRead that Context.read_traces(device=True) returned: its chromatograms and
    positions are taken where they lie on the GPU (positions is then ignored, device implied).  signals: int32 or int16 [4][ns] per trace (all int16: uploaded as int16); positions: Trace::basecallpos per
    trace.  device=False: host buffers, returns the per-trace results (PreparedBasecall.results).  device=True: returns the PreparedBasecall
    holding torch tensors on the GPU; .profiles_seqset() / .basecalls_struct() feed the align / consensus / decompose jobs, .results()
    copies back."""
    p = PreparedBasecall(signals, positions, sigratio, trim_stringency, device).run(self)
    return p if p.device else p.results()


Context.basecall_traces = _basecall_traces


# ---- the frame of the prepared two-pass calls (read, pad, render, render_alignments, render_decompositions) -----------------------------
class _TwoPassCall:
    """What PreparedRead, PreparedPad, PreparedRender, PreparedAlnText and PreparedDcpText share: a job struct built by the subclass, and a
    result struct that starts as the sizes-only form (per-item arrays alone) and takes payload arrays with with_capacity().  A subclass sets
      _stem      tracyhip_<stem> and tracyhip_<stem>_async are the calls
      _result    the result struct; the element types of its arrays are read from its fields
      _meta      its per-item arrays, which this object owns (self.meta)
      _sizes     those of them that sizes() returns: one array, or a tuple of several
      _caps      its offset / capacity arrays and _pay its payload arrays, both from the dict `o` of the hostlib <_host>_alloc layout
      _host      hostlib.<_host>_unpack reads one item of host_arrays()
      DEFERRED   the status of an item left to the host
      _flat_dev  the arrays of `flat` (the inputs in the layout of the hostlib batch) that may lie on the device alone, in self.d
      _gather    the per-item arrays of `flat` that a sub-batch of deferred items takes rows of (a missing one is an error), and
      _gather_opt  those a job may do without (trims, strands): gathered where `flat` holds them
    and _batch(sub): the hostlib batch over such a sub-batch."""
    _meta = _sizes = _caps = _pay = _flat_dev = _gather = _gather_opt = ()

    def _bind(self, o):
        """the result struct over the arrays of `o` (None: the sizes-only form)"""
        types = dict(self._result._fields_)
        self.meta = {k: np.zeros(max(self.nt, 1), np.dtype(types[k]._type_)) for k in self._meta}
        out = self.out = self._result()
        for k in self._meta:
            setattr(out, k, self.meta[k].ctypes.data_as(types[k]))
        self.o = o
        if o is None:
            return
        for k in self._caps:
            setattr(out, k, o[k].ctypes.data_as(types[k]))
        for k in self._pay:
            setattr(out, k, o[k].data_ptr() if self.device else o[k].ctypes.data)

    def _take(self, o):
        """binds freshly allocated host arrays `o`, their payloads uploaded first with device=True"""
        if self.device:
            import torch
            for k in self._pay:
                o[k] = torch.from_numpy(o[k]).cuda()
            torch.cuda.synchronize()
        self._bind(o)
        return self

    def sizes(self, ctx):
        """the sizes-only call: the sizes per item, 0 for deferred items"""
        self._bind(None)
        self.run(ctx)
        s = tuple(self.meta[k][:self.nt].copy() for k in self._sizes)
        return s if len(s) > 1 else s[0]

    def run(self, ctx, asynchronous=False):
        fn = getattr(lib(), "tracyhip_" + self._stem + ("_async" if asynchronous else ""))
        _check(fn(ctx._h, C.byref(self.job), self.mem, C.byref(self.out)))
        return self

    def host_arrays(self):
        """the result arrays on the host in the layout of the hostlib alloc (device payloads are copied back)"""
        o = dict(self.o)
        if self.device:
            for k in self._pay:
                o[k] = o[k].cpu().numpy()
        o.update(self.meta)
        return o

    def host_flat(self):
        """the inputs on the host in the layout of the hostlib batch"""
        f = dict(self.flat)
        for k in self._flat_dev:
            if k not in f:
                f[k] = self.d[k].cpu().numpy()
        return f

    def results(self, fill_deferred=True):
        """per item the dict of hostlib's unpack; deferred items are filled in by the host (_host_batch, _filled)"""
        from . import hostlib
        o = self.host_arrays()
        unpack = getattr(hostlib, self._host + "_unpack")
        res = [unpack(o, t) for t in range(self.nt)]
        sel = np.array([t for t in range(self.nt) if res[t]["status"] == self.DEFERRED], dtype=np.int64)
        if fill_deferred and len(sel):
            for t, r in zip(sel, self._host_batch(sel)):
                res[t] = self._filled(res[t], r)
        return res

    def _host_batch(self, sel):
        """the host's answers for the items `sel`: a sub-batch over the same payload arrays"""
        f = self.host_flat()
        sub = dict(f, nt=len(sel))
        for k in self._gather + tuple(k for k in self._gather_opt if k in f):
            sub[k] = np.append(f[k][sel], f[k].dtype.type(0))
        return self._batch(sub)

    def _filled(self, mine, r):
        """the result of a deferred item given the host's answer r: the answer, or `unreadable` with the status left DEFERRED"""
        return r if r["status"] == 0 else dict(mine, unreadable=True)


class _TextCall(_TwoPassCall):
    """the three calls that print: one text buffer, RenderResult, the layout of hostlib.render_alloc"""
    _meta = ("status", "text_len")
    _sizes = ("text_len",)
    _caps = ("text_offset", "text_cap")
    _pay = ("text",)

    def with_capacity(self, text_cap, fill=None, offsets=None):
        """a text buffer with room for text_cap[t] bytes of item t (fill: a byte the buffer starts with, for tests that check what a
        call leaves untouched; offsets: text_offset of every item and the buffer's size behind them, instead of back to back)"""
        from . import hostlib
        o = hostlib.render_alloc(self.nt, text_cap, fill)
        if offsets is not None:
            o["text_offset"] = np.ascontiguousarray(offsets, dtype=np.uint64)
            o["text"] = np.full(max(int(o["text_offset"][self.nt]), 1), 0 if fill is None else fill, np.uint8)
        return self._take(o)


# ---- chromatogram files read on the device (tracyhip_read_traces) ---------------------------------------------------------------------
READ_OK, READ_DEFERRED, READ_TOO_SMALL = 0, 1, 2


class ReadJob(C.Structure):
    _fields_ = [("ntraces", C.c_uint32), ("bytes", C.c_void_p), ("file_offset", C.POINTER(C.c_uint64)), ("file_len", C.POINTER(C.c_uint32)),
                ("sample_bytes", C.c_uint32)]


class ReadResult(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("format", C.POINTER(C.c_int32)), ("nsamples", C.POINTER(C.c_uint32)),
                ("ncalls", C.POINTER(C.c_uint32)), ("signal", C.c_void_p), ("sample_offset", C.POINTER(C.c_uint64)),
                ("sample_cap", C.POINTER(C.c_uint32)), ("basecallpos", C.c_void_p), ("basecalls1", C.c_void_p), ("basecalls2", C.c_void_p),
                ("qual", C.c_void_p), ("call_offset", C.POINTER(C.c_uint64)), ("call_cap", C.POINTER(C.c_uint32))]


_READ_PAY = ("signal", "basecallpos", "basecalls1", "basecalls2", "qual")


def read_bound(file_len):
    """tracyhip_read_bound: (nsamples_max, ncalls_max) that any answered file of this length fits; needs no device"""
    ns, nc = C.c_uint32(0), C.c_uint32(0)
    _check(lib().tracyhip_read_bound(C.c_uint32(file_len), C.byref(ns), C.byref(nc)))
    return ns.value, nc.value


class PreparedRead(_TwoPassCall):
    """job / result structs of tracyhip_read_traces.  files: per trace a path (read here, once) or the file image as bytes.  With
    device=True the images and the payload results are torch tensors on the GPU and stay there: Context.basecall_traces takes this object
    as it stands.  Everything the structs point to is kept alive by this object.

    The result side starts as the sizes-only form; with_capacity() allocates the payload results, bounds() gives capacities that need no
    sizes-only call.  sizes(): (nsamples, ncalls).  results(): per trace dict(status, format, nsamples, ncalls, signal [4][ns],
    basecallpos, basecalls1, basecalls2, qual); deferred traces are read by the host readers, except those they refuse too
    (`unreadable`: status stays DEFERRED)."""
    _stem, _result, _host, DEFERRED = "read_traces", ReadResult, "read", READ_DEFERRED
    _meta = ("status", "format", "nsamples", "ncalls")
    _sizes = ("nsamples", "ncalls")
    _caps = ("sample_offset", "sample_cap", "call_offset", "call_cap")
    _pay = _READ_PAY

    def __init__(self, files, sample_dtype=np.int16, device=False):
        from . import hostlib
        self.device = bool(device)
        self.sample_dtype = np.dtype(sample_dtype)
        f = self.flat = files if isinstance(files, dict) else hostlib.read_pack(files)
        nt = self.nt = f["nt"]
        job = self.job = ReadJob()
        job.ntraces = nt
        job.file_offset, job.file_len = _u64p(f["file_off"]), _u32p(f["file_len"])
        job.sample_bytes = self.sample_dtype.itemsize
        if self.device:
            import torch
            self.d_bytes = torch.from_numpy(f["bytes"]).cuda()
            torch.cuda.synchronize()
            job.bytes = self.d_bytes.data_ptr()
        else:
            job.bytes = f["bytes"].ctypes.data
        self.mem = MEM_DEVICE if self.device else MEM_HOST
        self._bind(None)

    def bounds(self):
        """tracyhip_read_bound per file: (sample_cap, call_cap) arrays"""
        b = [read_bound(int(n)) for n in self.flat["file_len"][:self.nt]]
        return np.array([x[0] for x in b], dtype=np.uint32), np.array([x[1] for x in b], dtype=np.uint32)

    def with_capacity(self, sample_cap, call_cap, fill=None):
        """payload results with room for sample_cap[t] samples per channel and call_cap[t] calls of trace t (fill: a value every payload
        element starts with, for tests that check what a call leaves untouched)"""
        from . import hostlib
        return self._take(hostlib.read_alloc(self.nt, self.sample_dtype, sample_cap, call_cap, fill))

    def _host_batch(self, sel):
        """the deferred files are read again from their packed images, not from a sub-batch"""
        from . import hostlib
        f = self.flat
        imgs = [f["bytes"][int(f["file_off"][t]):int(f["file_off"][t]) + int(f["file_len"][t])].tobytes() for t in sel]
        return hostlib.read_batch(imgs, self.sample_dtype)


def _read_traces(self, files, sample_dtype=np.int16, device=False, asynchronous=False):
    """tracyhip_read_traces.  files: paths or file images (bytes).  device=False: host buffers -- the sizes-only call, buffers of exactly
    those sizes (regions that follow each other come back as one copy), the call; returns the per-trace results (PreparedRead.results).
    device=True: capacities from tracyhip_read_bound, one call and one synchronisation; returns the PreparedRead holding torch tensors on
    the GPU, which Context.basecall_traces takes as it stands.  asynchronous: the call is queued (tracyhip_read_traces_async); results
    are final after Context.synchronize()."""
    p = PreparedRead(files, sample_dtype, device)
    p.with_capacity(*(p.bounds() if p.device else p.sizes(self))).run(self, asynchronous)
    return p if (p.device or asynchronous) else p.results()


Context.read_traces = _read_traces


# ---- gapped chromatograms along alignment rows on the device (tracyhip_pad_traces) -----------------------------------------------------
PAD_OK, PAD_DEFERRED, PAD_TOO_SMALL = 0, 1, 2


class PadJob(C.Structure):
    _fields_ = [("ntraces", C.c_uint32), ("signal", C.c_void_p), ("signal_offset", C.POINTER(C.c_uint64)), ("nsamples", C.POINTER(C.c_uint32)),
                ("sample_bytes", C.c_uint32), ("bcpos", C.c_void_p), ("primary", C.c_void_p), ("secondary", C.c_void_p), ("consensus", C.c_void_p),
                ("estqual", C.c_void_p), ("bc_offset", C.POINTER(C.c_uint64)), ("bc_len", C.POINTER(C.c_uint32)), ("rows", C.c_void_p),
                ("row_offset", C.POINTER(C.c_uint64)), ("row_len", C.POINTER(C.c_uint32)), ("trim_left_each", C.POINTER(C.c_uint32)),
                ("trim_right_each", C.POINTER(C.c_uint32)), ("reverse", C.POINTER(C.c_uint8))]


class PadResult(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("nsamples_out", C.POINTER(C.c_uint32)), ("ncalls_out", C.POINTER(C.c_uint32)),
                ("leading_gaps", C.POINTER(C.c_uint32)), ("trailing_gaps", C.POINTER(C.c_uint32)), ("step", C.POINTER(C.c_uint32)),
                ("signal", C.c_void_p), ("sample_offset", C.POINTER(C.c_uint64)), ("sample_cap", C.POINTER(C.c_uint32)), ("bcpos", C.c_void_p),
                ("primary", C.c_void_p), ("secondary", C.c_void_p), ("consensus", C.c_void_p), ("estqual", C.c_void_p),
                ("call_offset", C.POINTER(C.c_uint64)), ("call_cap", C.POINTER(C.c_uint32))]


_PAD_BC = ("bcpos", "primary", "secondary", "consensus", "estqual")
_PAD_META = ("nsamples_out", "ncalls_out", "leading_gaps", "trailing_gaps", "step")


def _flatten_traces(signals, bc, sample_dtype):
    """signals (int32 or int16 [4][ns] per trace; sample_dtype None: int16 if all are, else int32) and bc (per trace a dict of bcpos,
    primary, secondary, consensus, estqual) as the flattened input arrays of hostlib.pad_batch / render_batch: (sample dtype, dict)"""
    nt = len(signals)
    if sample_dtype is None:
        sample_dtype = np.int16 if nt and all(np.asarray(s).dtype == np.int16 for s in signals) else np.int32
    dt = np.dtype(sample_dtype)
    f = {}
    f["nsamples"] = np.array([np.asarray(s).shape[1] for s in signals] + [0], dtype=np.uint32)
    f["bc_len"] = np.array([len(b["bcpos"]) for b in bc] + [0], dtype=np.uint32)
    f["sig_off"] = np.zeros(nt + 1, np.uint64)
    f["bc_off"] = np.zeros(nt + 1, np.uint64)
    f["sig_off"][1:] = np.cumsum(4 * f["nsamples"][:nt].astype(np.uint64))
    f["bc_off"][1:] = np.cumsum(f["bc_len"][:nt].astype(np.uint64))
    f["signal"] = np.concatenate([np.ascontiguousarray(s, dtype=dt).reshape(-1) for s in signals] + [np.zeros(1, dt)])
    f["bcpos"] = np.concatenate([np.ascontiguousarray(b["bcpos"], dtype=np.int32).reshape(-1) for b in bc] + [np.zeros(1, np.int32)])
    for k in _PAD_BC[1:]:
        f[k] = np.concatenate([np.frombuffer(bytes(b[k]), np.uint8) if isinstance(b[k], (bytes, bytearray))
                               else np.ascontiguousarray(b[k], dtype=np.uint8).reshape(-1) for b in bc] + [np.zeros(1, np.uint8)])
    return dt, f


def _adopt_basecalls(f, device_bc):
    """the input side over a PreparedBasecall(device=True) that has run: its offsets and lengths into `f`; returns its chromatogram and
    basecall tensors as they stand"""
    f.update(sig_off=device_bc.sig_off, nsamples=device_bc.nsamples, bc_off=device_bc.pos_off, bc_len=device_bc.meta["bc_len"])
    return dict(signal=device_bc.d_signal, **{k: device_bc.payload[k] for k in _PAD_BC})


def _flat_trims(f, nt, trim_left, trim_right):
    """the per-trace trims into `f` (trim_l, trim_r), both or neither"""
    if (trim_left is None) != (trim_right is None):
        raise ValueError("trim_left and trim_right go together: both or neither")
    if trim_left is not None:
        f["trim_l"] = np.append(np.ascontiguousarray(trim_left, dtype=np.uint32)[:nt], np.uint32(0))
        f["trim_r"] = np.append(np.ascontiguousarray(trim_right, dtype=np.uint32)[:nt], np.uint32(0))


def _point_at_traces(job, f, ptr, sample_dtype):
    """the chromatogram, basecall and trim fields that PadJob and RenderJob share, over `f` and the payload pointers ptr(key)"""
    job.signal, job.sample_bytes = ptr("signal"), sample_dtype.itemsize
    job.signal_offset, job.nsamples = _u64p(f["sig_off"]), _u32p(f["nsamples"])
    for k in _PAD_BC:
        setattr(job, k, ptr(k))
    job.bc_offset, job.bc_len = _u64p(f["bc_off"]), _u32p(f["bc_len"])
    if "trim_l" in f:
        job.trim_left_each, job.trim_right_each = _u32p(f["trim_l"]), _u32p(f["trim_r"])


class PreparedPad(_TwoPassCall):
    """job / result structs of tracyhip_pad_traces.  signals: int32 or int16 [4][ns] per trace; bc: per trace a dict of bcpos, primary,
    secondary, consensus, estqual; rows: the row of each trace as bytes, or (data, row_offset, row_len) with data a numpy array or a torch
    tensor on the GPU holding rows of some alignment result as they stand.  device_bc: a PreparedBasecall(device=True) that has run -- its
    chromatogram and basecall tensors are taken as they stand (signals and bc are then ignored).  With device=True (implied by device_bc)
    the payloads are torch tensors on the GPU.  Everything the structs point to is kept alive by this object.

    The result side starts as the sizes-only form; with_capacity() allocates the payload results.  sizes(): (nsamples_out, ncalls_out).
    results(): per trace dict(status, signal [4][ns'], bcPos, primary, secondary, consensus, estQual, leadingGaps, trailingGaps, step);
    deferred traces are filled in by the host chain (hostlib.pad_batch), except those the reference's loops cannot run either
    (`unreadable`: status stays DEFERRED)."""
    _stem, _result, _host, DEFERRED = "pad_traces", PadResult, "pad", PAD_DEFERRED
    _meta = _PAD_META + ("status",)
    _sizes = ("nsamples_out", "ncalls_out")
    _caps = ("sample_offset", "sample_cap", "call_offset", "call_cap")
    _pay = ("signal",) + _PAD_BC
    _flat_dev = ("signal",) + _PAD_BC + ("rows",)
    _gather = ("sig_off", "nsamples", "bc_off", "bc_len", "row_off", "row_len")
    _gather_opt = ("trim_l", "trim_r", "reverse")

    def __init__(self, signals, bc, rows, trim_left=None, trim_right=None, reverse=None, device=False, device_bc=None, sample_dtype=None):
        self.device = device = bool(device or device_bc is not None)
        self.device_bc = device_bc
        f = self.flat = {}  # host copies in the layout of hostlib.pad_batch (of a device_bc: fetched when a deferred trace needs them)
        if device_bc is not None:
            nt = self.nt = device_bc.nt
            self.sample_dtype = device_bc.sample_dtype
            self.d = _adopt_basecalls(f, device_bc)
        else:
            nt = self.nt = len(signals)
            self.sample_dtype, flat = _flatten_traces(signals, bc, sample_dtype)
            f.update(flat)
        f["nt"] = nt
        if isinstance(rows, tuple):
            data, roff, rlen = rows
            f["row_off"] = np.append(np.ascontiguousarray(roff, dtype=np.uint64)[:nt], np.uint64(0))
            f["row_len"] = np.append(np.ascontiguousarray(rlen, dtype=np.uint32)[:nt], np.uint32(0))
            self._rows_in = data
            if isinstance(data, np.ndarray):
                f["rows"] = np.ascontiguousarray(data, dtype=np.uint8)
        else:
            f["row_len"] = np.array([len(r) for r in rows] + [0], dtype=np.uint32)
            f["row_off"] = np.zeros(nt + 1, np.uint64)
            f["row_off"][1:] = np.cumsum(f["row_len"][:nt].astype(np.uint64))
            f["rows"] = np.frombuffer(b"".join(bytes(r) for r in rows) + b"\0", np.uint8).copy()
            self._rows_in = f["rows"]
        _flat_trims(f, nt, trim_left, trim_right)
        if reverse is not None:
            f["reverse"] = np.append(np.array([1 if x else 0 for x in reverse], dtype=np.uint8)[:nt], np.uint8(0))
        if device:
            import torch
            if device_bc is None:
                self.d = {k: torch.from_numpy(f[k]).cuda() for k in ("signal",) + _PAD_BC}
            self.d["rows"] = self._rows_in if not isinstance(self._rows_in, np.ndarray) else torch.from_numpy(f["rows"]).cuda()
            torch.cuda.synchronize()
            ptr = lambda k: self.d[k].data_ptr()
        else:
            if not isinstance(self._rows_in, np.ndarray):
                raise ValueError("rows on the device need device=True")
            ptr = lambda k: f[k].ctypes.data
        job = self.job = PadJob()
        job.ntraces = nt
        _point_at_traces(job, f, ptr, self.sample_dtype)
        job.rows, job.row_offset, job.row_len = ptr("rows"), _u64p(f["row_off"]), _u32p(f["row_len"])
        if reverse is not None:
            job.reverse = f["reverse"].ctypes.data_as(C.POINTER(C.c_uint8))
        self.mem = MEM_DEVICE if device else MEM_HOST
        self._bind(None)

    def with_capacity(self, sample_cap, call_cap, fill=None):
        """payload results with room for sample_cap[t] samples per channel and call_cap[t] calls of trace t (fill: a value every payload
        element starts with, for tests that check what a call leaves untouched)"""
        from . import hostlib
        o = hostlib.pad_alloc(dict(nt=self.nt, signal=np.zeros(0, self.sample_dtype)), sample_cap, call_cap)
        if fill is not None:
            for k in self._pay:
                o[k][:] = fill
        return self._take(o)

    def _batch(self, sub):
        from . import hostlib
        return hostlib.pad_batch(sub)


def _pad_traces(self, signals, bc, rows, trim_left=None, trim_right=None, reverse=None, device=False, device_bc=None, asynchronous=False):
    """tracyhip_pad_traces: the sizes-only call, buffers of exactly those sizes, the call.  device=False: host buffers, returns the
    per-trace results (PreparedPad.results).  device=True or device_bc: returns the PreparedPad holding torch tensors on the GPU.
    asynchronous: the second call is queued (tracyhip_pad_traces_async); results are final after Context.synchronize()."""
    p = PreparedPad(signals, bc, rows, trim_left, trim_right, reverse, device, device_bc)
    p.with_capacity(*p.sizes(self)).run(self, asynchronous)
    return p if (p.device or asynchronous) else p.results()


Context.pad_traces = _pad_traces


# ---- the text of the writers on the device (tracyhip_render_traces) ---------------------------------------------------------------------
RENDER_TSV, RENDER_JSON, RENDER_GAPPED = 0, 1, 2
RENDER_OK, RENDER_DEFERRED, RENDER_TOO_SMALL = 0, 1, 2


class RenderJob(C.Structure):
    _fields_ = [("ntraces", C.c_uint32), ("form", C.c_uint32), ("signal", C.c_void_p), ("signal_offset", C.POINTER(C.c_uint64)),
                ("nsamples", C.POINTER(C.c_uint32)), ("sample_bytes", C.c_uint32), ("bcpos", C.c_void_p), ("primary", C.c_void_p),
                ("secondary", C.c_void_p), ("consensus", C.c_void_p), ("estqual", C.c_void_p), ("bc_offset", C.POINTER(C.c_uint64)),
                ("bc_len", C.POINTER(C.c_uint32)), ("trim_left_each", C.POINTER(C.c_uint32)), ("trim_right_each", C.POINTER(C.c_uint32))]


class RenderResult(C.Structure):
    _fields_ = [("status", C.POINTER(C.c_int32)), ("text_len", C.POINTER(C.c_uint32)), ("text", C.c_void_p),
                ("text_offset", C.POINTER(C.c_uint64)), ("text_cap", C.POINTER(C.c_uint64))]


def render_bound(form, nsamples, bc_len, sample_bytes):
    """tracyhip_render_bound: an upper bound of text_len for a trace of these sizes; needs no device"""
    return int(lib().tracyhip_render_bound(C.c_uint32(form), C.c_uint32(nsamples), C.c_uint32(bc_len), C.c_uint32(sample_bytes)))


class PreparedRender(_TextCall):
    """job / result structs of tracyhip_render_traces.  form: RENDER_TSV / RENDER_JSON / RENDER_GAPPED.  The traces come from one of
      signals, bc   int32 or int16 [4][ns] per trace; per trace a dict of bcpos, primary, secondary, consensus, estqual (host arrays;
                    device=True uploads them once)
      device_bc     a PreparedBasecall(device=True) that has run: its chromatogram and basecall tensors are taken as they stand
      device_pad    a PreparedPad(device=True) that has run with payload results: the padded chromatograms and basecalls as they stand
    No payload is copied to the host for the last two.  trim_left / trim_right: the per-trace trims of the TSV's trim column.
    Everything the structs point to is kept alive by this object.

    The result side starts as the sizes-only form; with_capacity() allocates the text.  sizes(): text_len.  results(): per trace
    dict(status, text_len, text); deferred traces are printed by the host writers (hostlib.render_batch), except those the reference's
    loops cannot run either (`unreadable`: status stays DEFERRED)."""
    _stem, _result, _host, DEFERRED = "render_traces", RenderResult, "render", RENDER_DEFERRED
    _flat_dev = ("signal",) + _PAD_BC
    _gather = ("sig_off", "nsamples", "bc_off", "bc_len")
    _gather_opt = ("trim_l", "trim_r")

    def __init__(self, form, signals=None, bc=None, trim_left=None, trim_right=None, device=False, device_bc=None, device_pad=None,
                 sample_dtype=None):
        self.form = int(form)
        self.device = device = bool(device or device_bc is not None or device_pad is not None)
        f = self.flat = {}  # host copies in the layout of hostlib.render_batch (device sources: fetched when a deferred trace needs them)
        if device_bc is not None:
            nt = self.nt = device_bc.nt
            self.sample_dtype = device_bc.sample_dtype
            self.d = _adopt_basecalls(f, device_bc)
        elif device_pad is not None:
            if not device_pad.device or device_pad.o is None:
                raise ValueError("device_pad: a PreparedPad(device=True) with payload results")
            nt = self.nt = device_pad.nt
            self.sample_dtype = device_pad.sample_dtype
            f.update(sig_off=device_pad.o["sample_offset"], nsamples=device_pad.meta["nsamples_out"], bc_off=device_pad.o["call_offset"],
                     bc_len=device_pad.meta["ncalls_out"])
            self.d = {k: device_pad.o[k] for k in ("signal",) + _PAD_BC}
        else:
            nt = self.nt = len(signals)
            self.sample_dtype, flat = _flatten_traces(signals, bc, sample_dtype)
            f.update(flat)
            if device:
                import torch
                self.d = {k: torch.from_numpy(f[k]).cuda() for k in ("signal",) + _PAD_BC}
                torch.cuda.synchronize()
        f["nt"] = nt
        _flat_trims(f, nt, trim_left, trim_right)
        job = self.job = RenderJob()
        job.ntraces, job.form = nt, self.form
        _point_at_traces(job, f, (lambda k: self.d[k].data_ptr()) if device else (lambda k: f[k].ctypes.data), self.sample_dtype)
        self.mem = MEM_DEVICE if device else MEM_HOST
        self._bind(None)

    def bounds(self):
        """tracyhip_render_bound per trace: capacities that need no sizes-only call"""
        f = self.flat
        return np.array([render_bound(self.form, int(f["nsamples"][t]), int(f["bc_len"][t]), self.sample_dtype.itemsize) for t in range(self.nt)],
                        dtype=np.uint64)

    def _batch(self, sub):
        from . import hostlib
        return hostlib.render_batch(sub, self.form)


def _render_traces(self, form, signals=None, bc=None, trim_left=None, trim_right=None, device=False, device_bc=None, device_pad=None,
                   asynchronous=False):
    """tracyhip_render_traces: the sizes-only call, a buffer of exactly those sizes, the call.  Host arrays with device=False: returns the
    per-trace results (PreparedRender.results).  device=True, device_bc or device_pad: returns the PreparedRender holding the text as a
    torch tensor on the GPU.  asynchronous: the second call is queued (tracyhip_render_traces_async); results are final after
    Context.synchronize()."""
    p = PreparedRender(form, signals, bc, trim_left, trim_right, device, device_bc, device_pad)
    p.with_capacity(p.sizes(self)).run(self, asynchronous)
    return p if (p.device or asynchronous) else p.results()


Context.render_traces = _render_traces


# ---- the text printed from alignment rows on the device (tracyhip_render_alignments) and the oriented reference slices in front of the
# rows (tracyhip_reference_slices) -------------------------------------------------------------------------------------------------------
ALNTEXT_PLOT, ALNTEXT_FASTA, ALNTEXT_JSON = 0, 1, 2
ALNTEXT_OK, ALNTEXT_DEFERRED, ALNTEXT_TOO_SMALL = 0, 1, 2


class AlnTextJob(C.Structure):
    _fields_ = [("n", C.c_uint32), ("form", C.c_uint32), ("key", C.c_uint32), ("linelimit", C.c_uint32), ("rows0", C.c_void_p), ("rows1", C.c_void_p),
                ("rows_offset", C.POINTER(C.c_uint64)), ("cols", C.POINTER(C.c_uint32)), ("names", C.c_void_p),
                ("name0_offset", C.POINTER(C.c_uint64)), ("name0_len", C.POINTER(C.c_uint32)), ("name1_offset", C.POINTER(C.c_uint64)),
                ("name1_len", C.POINTER(C.c_uint32)), ("ref_pos", C.POINTER(C.c_int32)), ("ref_len", C.POINTER(C.c_uint32)),
                ("forward", C.POINTER(C.c_uint8)), ("score", C.POINTER(C.c_int32))]


class SlicesJob(C.Structure):
    _fields_ = [("n", C.c_uint32), ("refs", SeqSet), ("ref_index", C.POINTER(C.c_uint32)), ("forward", C.POINTER(C.c_uint8)),
                ("slice_begin", C.POINTER(C.c_uint32)), ("slice_len", C.POINTER(C.c_uint32))]


def alntext_bound(form, linelimit, cols, name0_len, name1_len):
    """tracyhip_render_alignments_bound: an upper bound of text_len for an alignment of these sizes; needs no device"""
    return int(lib().tracyhip_render_alignments_bound(C.c_uint32(form), C.c_uint32(linelimit), C.c_uint32(cols), C.c_uint32(name0_len),
                                                      C.c_uint32(name1_len)))


class PreparedAlnText(_TextCall):
    """job / result structs of tracyhip_render_alignments.  form: ALNTEXT_PLOT / ALNTEXT_FASTA / ALNTEXT_JSON.  The rows come from
      rows0, rows1   lists of bytes, one pair per alignment (device=True uploads them once), or
      device_rows    (rows0, rows1, rows_offset, cols): two torch tensors on the GPU as tracyhip_alignment_rows / tracyhip_align_traces
                     left them and their two host arrays; taken as they stand (no payload is copied to the host)
    name0 / name1: lists of bytes, the caller's text (hostlib.alntext_pack says which per form).  ref_pos, ref_len, forward, score: per
    alignment.  Everything the structs point to is kept alive by this object.

    The result side starts as the sizes-only form; with_capacity() allocates the text.  sizes(): text_len.  results(): per alignment
    dict(status, text_len, text); deferred alignments are printed by the host writers (hostlib.alntext_batch) and marked
    deferred=True."""
    _stem, _result, _host, DEFERRED = "render_alignments", RenderResult, "alntext", ALNTEXT_DEFERRED
    _flat_dev = ("rows0", "rows1")
    _gather = ("rows_off", "cols", "name0_off", "name0_len", "name1_off", "name1_len", "ref_pos", "ref_len", "forward", "score")

    def __init__(self, form, rows0=None, rows1=None, name0=None, name1=None, ref_pos=None, ref_len=None, forward=None, score=None, key=0,
                 linelimit=60, device=False, device_rows=None):
        from . import hostlib
        self.form, self.key, self.linelimit = int(form), int(key), int(linelimit)
        self.device = device = bool(device or device_rows is not None)
        if device_rows is not None:
            d0, d1, roff, cols = device_rows
            nt = len(name1)
            f = self.flat = hostlib.alntext_pack([b""] * nt, [b""] * nt, name0 if name0 is not None else [b""] * nt, name1, ref_pos, ref_len,
                                                 forward, score)
            del f["rows0"], f["rows1"]  # (host copies: fetched when a deferred alignment needs them)
            f["rows_off"] = np.append(np.ascontiguousarray(roff, dtype=np.uint64)[:nt], np.uint64(0))
            f["cols"] = np.append(np.ascontiguousarray(cols, dtype=np.uint32)[:nt], np.uint32(0))
            self.d = dict(rows0=d0, rows1=d1)
        else:
            nt = len(rows0)
            f = self.flat = hostlib.alntext_pack(rows0, rows1, name0 if name0 is not None else [b""] * nt, name1, ref_pos, ref_len, forward, score)
            self.d = {}
        self.nt = nt
        if device:
            import torch
            for k in ("rows0", "rows1", "names"):
                if k not in self.d:
                    self.d[k] = torch.from_numpy(f[k]).cuda()
            torch.cuda.synchronize()
        ptr = (lambda k: self.d[k].data_ptr()) if device else (lambda k: f[k].ctypes.data)
        job = self.job = AlnTextJob()
        job.n, job.form, job.key, job.linelimit = nt, self.form, self.key, self.linelimit
        job.rows0, job.rows1, job.names = ptr("rows0"), ptr("rows1"), ptr("names")
        job.rows_offset, job.cols = _u64p(f["rows_off"]), _u32p(f["cols"])
        job.name0_offset, job.name0_len = _u64p(f["name0_off"]), _u32p(f["name0_len"])
        job.name1_offset, job.name1_len = _u64p(f["name1_off"]), _u32p(f["name1_len"])
        job.ref_pos = f["ref_pos"].ctypes.data_as(C.POINTER(C.c_int32))
        job.ref_len = _u32p(f["ref_len"])
        job.forward = f["forward"].ctypes.data_as(C.POINTER(C.c_uint8))
        job.score = f["score"].ctypes.data_as(C.POINTER(C.c_int32))
        self.mem = MEM_DEVICE if device else MEM_HOST
        self._bind(None)

    def bounds(self):
        """tracyhip_render_alignments_bound per alignment: capacities that need no sizes-only call"""
        f = self.flat
        return np.array([alntext_bound(self.form, self.linelimit, int(f["cols"][t]), int(f["name0_len"][t]), int(f["name1_len"][t]))
                         for t in range(self.nt)], dtype=np.uint64)

    def stats(self, ctx):
        st = AlnTextStats()
        _check(lib().tracyhip_last_alntext_stats(ctx._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in AlnTextStats._fields_}

    def _batch(self, sub):
        from . import hostlib
        return hostlib.alntext_batch(sub, self.form, self.key, self.linelimit)

    def _filled(self, mine, r):
        """the host writers answer whatever the device defers: the answer marked, else the item as it was"""
        return dict(r, deferred=True) if r["status"] == 0 else mine


def _render_alignments(self, form, rows0=None, rows1=None, name0=None, name1=None, ref_pos=None, ref_len=None, forward=None, score=None, key=0,
                       linelimit=60, device=False, device_rows=None, asynchronous=False):
    """tracyhip_render_alignments: the sizes-only call, a buffer of exactly those sizes, the call.  Host rows with device=False: returns
    the per-alignment results (PreparedAlnText.results: deferred alignments are filled in by the host batch).  device=True or
    device_rows: returns the PreparedAlnText holding the text as a torch tensor on the GPU.  asynchronous: the second call is queued
    (tracyhip_render_alignments_async); results are final after Context.synchronize()."""
    p = PreparedAlnText(form, rows0, rows1, name0, name1, ref_pos, ref_len, forward, score, key, linelimit, device, device_rows)
    p.with_capacity(p.sizes(self)).run(self, asynchronous)
    return p if (p.device or asynchronous) else p.results()


Context.render_alignments = _render_alignments


class PreparedSlices:
    """job of tracyhip_reference_slices: refs a list of bytes or a PackedSeqs of kind CHAR (device_refs: a torch tensor that holds its
    data on the GPU already); forward, slice_begin, slice_len the arrays tracyhip_align_traces returned.  The slices lie back to back in
    `out` (a numpy array, or a torch tensor with device=True) at out_offset."""

    def __init__(self, refs, forward, slice_begin, slice_len, ref_index=None, device=False, device_refs=None):
        pr = self.refs = refs if isinstance(refs, PackedSeqs) else PackedSeqs(refs, SEQ_CHAR)
        self.device = device = bool(device or device_refs is not None)
        nt = self.nt = len(forward)
        self.forward = np.append(np.ascontiguousarray(forward, dtype=np.uint8)[:nt], np.uint8(0))
        self.begin = np.append(np.ascontiguousarray(slice_begin, dtype=np.uint32)[:nt], np.uint32(0))
        self.len = np.append(np.ascontiguousarray(slice_len, dtype=np.uint32)[:nt], np.uint32(0))
        self.out_offset = np.zeros(nt + 1, np.uint64)
        self.out_offset[1:] = np.cumsum(self.len[:nt].astype(np.uint64))
        job = self.job = SlicesJob()
        job.n = nt
        if device:
            import torch
            self.d_refs = device_refs if device_refs is not None else torch.from_numpy(pr.data).cuda()
            self.out = torch.zeros(max(int(self.out_offset[nt]), 1), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            job.refs = pr.seqset(self.d_refs.data_ptr())
        else:
            self.out = np.zeros(max(int(self.out_offset[nt]), 1), np.uint8)
            job.refs = pr.seqset()
        if ref_index is not None:
            self.ref_index = np.ascontiguousarray(ref_index, dtype=np.uint32)
            job.ref_index = _u32p(self.ref_index)
        job.forward = self.forward.ctypes.data_as(C.POINTER(C.c_uint8))
        job.slice_begin, job.slice_len = _u32p(self.begin), _u32p(self.len)
        self.mem = MEM_DEVICE if device else MEM_HOST

    def out_ptr(self):
        return self.out.data_ptr() if self.device else self.out.ctypes.data

    def validate(self):
        return lib().tracyhip_reference_slices_validate(C.byref(self.job), self.mem, C.c_void_p(self.out_ptr()), _u64p(self.out_offset))

    def run(self, ctx, asynchronous=False):
        fn = lib().tracyhip_reference_slices_async if asynchronous else lib().tracyhip_reference_slices
        _check(fn(ctx._h, C.byref(self.job), self.mem, C.c_void_p(self.out_ptr()), _u64p(self.out_offset)))
        return self

    def slices(self):
        """the slices as bytes (a device result is copied back)"""
        o = self.out.cpu().numpy() if self.device else self.out
        return [o[int(self.out_offset[t]):int(self.out_offset[t]) + int(self.len[t])].tobytes() for t in range(self.nt)]

    def seqset(self):
        """the slices as the CHAR seqset tracyhip_alignment_rows takes them by (kept alive by this object)"""
        s = SeqSet()
        s.kind, s.data, s.count = SEQ_CHAR, self.out_ptr(), self.nt
        s.offset, s.length = _u64p(self.out_offset), _u32p(self.len)
        return s


def _reference_slices(self, refs, forward, slice_begin, slice_len, ref_index=None, device=False, device_refs=None, asynchronous=False):
    """tracyhip_reference_slices.  Host references with device=False: returns the slices as a list of bytes.  device=True or
    device_refs: returns the PreparedSlices holding them as a torch tensor on the GPU (PreparedSlices.seqset() hands them to
    tracyhip_alignment_rows).  asynchronous: queued; final after Context.synchronize()."""
    p = PreparedSlices(refs, forward, slice_begin, slice_len, ref_index, device, device_refs).run(self, asynchronous)
    return p if (p.device or asynchronous) else p.slices()


Context.reference_slices = _reference_slices


# ---- the text printed from the decompose results on the device (tracyhip_render_decompositions) ------------------------------------------
DCPTEXT_DECOMP, DCPTEXT_JSON, DCPTEXT_VCF = 0, 1, 2
DCPTEXT_OK, DCPTEXT_DEFERRED, DCPTEXT_TOO_SMALL = 0, 1, 2


class DcpTextJob(C.Structure):
    _fields_ = [("n", C.c_uint32), ("form", C.c_uint32), ("qual_cut", C.c_uint32), ("dcp_indel", C.c_void_p), ("dcp_err", C.c_void_p),
                ("dcp_offset", C.POINTER(C.c_uint64)), ("dcp_rows", C.POINTER(C.c_uint32)), ("rows0", C.c_void_p * 3), ("rows1", C.c_void_p * 3),
                ("rows_offset", C.POINTER(C.c_uint64) * 3), ("cols", C.POINTER(C.c_uint32) * 3), ("bcpos", C.c_void_p), ("estqual", C.c_void_p),
                ("bc_offset", C.POINTER(C.c_uint64)), ("bc_len", C.POINTER(C.c_uint32)), ("var", C.c_void_p), ("var_text", C.c_void_p),
                ("var_n", C.c_void_p), ("max_variants", C.c_uint32), ("max_text", C.c_uint32), ("var_index", C.POINTER(C.c_uint32)), ("ref_pos", C.POINTER(C.c_uint32) * 2),
                ("forward", C.POINTER(C.c_uint8)), ("score", C.POINTER(C.c_int32) * 3), ("breakpoint", C.POINTER(C.c_uint32)),
                ("indelshift", C.POINTER(C.c_uint8)), ("trim_left", C.POINTER(C.c_uint32)), ("trim_right", C.POINTER(C.c_uint32)),
                ("names", C.c_void_p), ("chr_offset", C.POINTER(C.c_uint64) * 2), ("chr_len", C.POINTER(C.c_uint32) * 2),
                ("frac_offset", C.POINTER(C.c_uint64) * 2), ("frac_len", C.POINTER(C.c_uint32) * 2)]


class DcpTextShape(C.Structure):
    _fields_ = [("dcp_rows", C.c_uint32), ("cols", C.c_uint32 * 3), ("chr_len", C.c_uint32 * 2), ("frac_len", C.c_uint32 * 2),
                ("max_variants", C.c_uint32), ("max_text", C.c_uint32)]


class DcpTextStats(C.Structure):
    """tracyhip_dcptext_stats: the counters of tracyhip_render_decompositions, in a struct of their own as RenderStats"""
    _fields_ = [("dcptext_chunks", C.c_uint32), ("dcptext_deferred", C.c_uint32), ("dcptext_too_small", C.c_uint32)]


def dcptext_bound(form, dcp_rows=0, cols=(0, 0, 0), chr_len=(0, 0), frac_len=(0, 0), max_variants=1, max_text=2):
    """tracyhip_render_decompositions_bound: an upper bound of text_len for a trace of these sizes; needs no device"""
    fn = lib().tracyhip_render_decompositions_bound
    fn.restype = C.c_uint64
    sh = DcpTextShape(dcp_rows, (C.c_uint32 * 3)(*cols), (C.c_uint32 * 2)(*chr_len), (C.c_uint32 * 2)(*frac_len), max_variants, max_text)
    return int(fn(C.c_uint32(form), C.byref(sh)))


class PreparedDcpText(_TextCall):
    """job / result structs of tracyhip_render_decompositions.  form: DCPTEXT_DECOMP / DCPTEXT_JSON / DCPTEXT_VCF.  flat: the arrays of
    hostlib.dcptext_pack (host metadata and host payloads).  device=True uploads the payloads once; device_arrays: torch tensors on the
    GPU by payload name (hostlib.DCPTEXT_PAYLOADS) that are taken as they stand in place of flat's -- the tables of
    decompose_traces(device_bc=...), the rows of tracyhip_alignment_rows, the basecalls, the four arrays of a VariantBuffers(device=True);
    no payload is copied to the host for them, and flat need not hold them.  Everything the structs point to is kept alive by this object.

    The result side starts as the sizes-only form; with_capacity() allocates the text.  sizes(): text_len.  results(): per trace
    dict(status, text_len, text); deferred traces are printed by the host writers (hostlib.dcptext_batch) and marked deferred=True, except
    those the writers cannot index either (`unreadable`: status stays DEFERRED)."""
    _stem, _result, _host, DEFERRED = "render_decompositions", RenderResult, "dcptext", DCPTEXT_DEFERRED

    def __init__(self, form, flat, qual_cut=45, device=False, device_arrays=None):
        from . import hostlib
        self.form, self.qual_cut = int(form), int(qual_cut)
        self.device = device = bool(device or device_arrays)
        self.flat = f = dict(flat)
        self.nt = f["nt"]
        self.d = dict(device_arrays or {})
        self._flat_dev = hostlib.DCPTEXT_PAYLOADS
        if device:
            import torch
            for k in hostlib.DCPTEXT_PAYLOADS:
                if k not in self.d:
                    self.d[k] = torch.from_numpy(np.ascontiguousarray(f[k]).view(np.uint8)).cuda()  # (bytes: the job takes addresses)
            torch.cuda.synchronize()
        self.job = hostlib.dcptext_job(f, self.form, self.qual_cut, (lambda k: self.d[k].data_ptr()) if device else (lambda k: f[k].ctypes.data))
        self.mem = MEM_DEVICE if device else MEM_HOST
        self._bind(None)

    def bounds(self):
        """tracyhip_render_decompositions_bound per trace: capacities that need no sizes-only call"""
        f = self.flat
        return np.array([dcptext_bound(self.form, int(f["dcp_rows"][t]), [int(f["cols_%d" % k][t]) for k in range(3)],
                                       [int(f["chr%d_len" % k][t]) for k in (1, 2)], [int(f["frac%d_len" % k][t]) for k in (1, 2)],
                                       f["max_variants"], f["max_text"]) for t in range(self.nt)], dtype=np.uint64)

    def stats(self, ctx):
        st = DcpTextStats()
        _check(lib().tracyhip_last_dcptext_stats(ctx._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in DcpTextStats._fields_}

    def host_flat(self):
        f = dict(self.flat)
        for k, v in self.d.items():
            h = v.cpu().numpy()
            f[k] = h.view(VARIANT_DTYPE) if k == "var" else h.view(np.int32) if k in ("dcp_indel", "dcp_err", "bcpos") else \
                h.view(np.uint32) if k == "var_n" else h
        return f

    def _host_batch(self, sel):
        """(the variants of a trace lie at its index: the host prints the batch and the deferred traces are picked)"""
        from . import hostlib
        res = hostlib.dcptext_batch(self.host_flat(), self.form, self.qual_cut)
        return [res[t] for t in sel]

    def _filled(self, mine, r):
        return dict(r, deferred=True) if r["status"] == 0 else dict(mine, unreadable=True)


def _render_decompositions(self, form, flat, qual_cut=45, device=False, device_arrays=None, asynchronous=False):
    """tracyhip_render_decompositions: the sizes-only call, a buffer of exactly those sizes, the call.  Host arrays with device=False:
    returns the per-trace results (PreparedDcpText.results: deferred traces are filled in by the host batch).  device=True or
    device_arrays: returns the PreparedDcpText holding the text as a torch tensor on the GPU.  asynchronous: the second call is queued
    (tracyhip_render_decompositions_async); results are final after Context.synchronize()."""
    p = PreparedDcpText(form, flat, qual_cut, device, device_arrays)
    p.with_capacity(p.sizes(self)).run(self, asynchronous)
    return p if (p.device or asynchronous) else p.results()


Context.render_decompositions = _render_decompositions
