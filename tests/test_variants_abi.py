"""The argument checks of tracyhip_decompose_variants (tracyhip_decompose_variants_validate) and of the stage tracyhip_call_variants, and
the ABI they add: the record layout and the counters appended to tracyhip_call_stats.  No device is needed."""
import ctypes as C

import numpy as np

from tracy_amd import capi

ERR_ARG, ERR_RANGE = capi.ERR_ARG, capi.ERR_RANGE


class Prepared:
    """a valid job / decompose result / variants result of two traces on host arrays"""

    def __init__(self, nt=2):
        self.keep = k = {}
        k["bc_off"] = np.arange(nt, dtype=np.uint64) * 100
        k["bc_len"] = np.full(max(nt, 1), 100, np.uint32)
        k["pri"] = np.full(max(nt, 1) * 100, ord("A"), np.uint8)
        self.refs = capi.PackedSeqs([b"ACGT" * 50] * nt, capi.SEQ_CHAR)
        self.job = capi.DecomposeJob()
        self.job.ntraces = nt
        self.job.bc.ntraces = nt
        self.job.bc.primary = k["pri"].ctypes.data
        self.job.bc.bc_offset = capi._u64p(k["bc_off"])
        self.job.bc.bc_len = capi._u32p(k["bc_len"])
        self.job.refs = self.refs.seqset()
        self.job.dprm = capi.DecompParams(20, 20, 1000, 5)
        self.res = capi.DecomposeResult()
        for name, dt in (("status", np.int32), ("forward", np.uint8)):
            k[name] = np.zeros(max(nt, 1), dt)
            setattr(self.res, name, k[name].ctypes.data)
        k["sd"] = np.full(max(nt, 1) * 100, ord("A"), np.uint8)
        self.res.secdecomp = k["sd"].ctypes.data
        for a in range(2):
            for name in ("slice_begin", "slice_len", "ref_pos", "ops_len"):
                k[name + str(a)] = np.zeros(max(nt, 1), np.uint32)
                getattr(self.res, name)[a] = k[name + str(a)].ctypes.data
            k["ops" + str(a)] = np.zeros(max(nt, 1) * 300, np.uint8)
            k["off" + str(a)] = np.arange(max(nt, 1), dtype=np.uint64) * 300
            self.res.ops[a] = k["ops" + str(a)].ctypes.data
            self.res.ops_offset[a] = capi._u64p(k["off" + str(a)])
        self.slice_pos = np.zeros(max(nt, 1), np.uint32)
        self.prm = capi.Params(3, -5, -10, -4, 1, 0)
        self.buf = capi.VariantBuffers(nt, 16, 256)
        self.out = self.buf.struct


def check(p, mem=capi.MEM_HOST, job=True, res=True, sp=True, prm=True, out=True):
    return capi.lib().tracyhip_decompose_variants_validate(C.byref(p.job) if job else None, C.byref(p.res) if res else None,
                                                           capi._u32p(p.slice_pos) if sp else None, C.byref(p.prm) if prm else None, mem,
                                                           C.byref(p.out) if out else None)


def last():
    return capi.lib().tracyhip_last_error().decode()


def test_validate_accepts_a_good_call_and_an_empty_one():
    p = Prepared()
    assert check(p) == 0 and check(p, capi.MEM_DEVICE) == 0
    capi.decompose_variants_validate(p.job, p.res, p.slice_pos, p.prm, p.out)
    e = Prepared(0)
    assert check(e) == 0
    e.out.var = None  # nothing is written for no traces
    assert check(e) == 0 and check(e, sp=False) == 0


def test_validate_null_arguments_and_mem():
    p = Prepared()
    assert check(p, mem=2) == ERR_ARG and "mem" in last()
    for kw in ("job", "res", "out", "prm", "sp"):
        assert check(p, **{kw: False}) == ERR_ARG, kw
    assert "slice_pos" in last()
    for field in ("var", "text", "var_n", "var_flags"):
        p = Prepared()
        setattr(p.out, field, None)
        assert check(p) == ERR_ARG and "result arrays" in last(), field


def test_validate_capacities():
    for maxv, code in ((0, ERR_RANGE), (1, 0), (1024, 0), (1025, ERR_RANGE), (1 << 31, ERR_RANGE)):
        p = Prepared()
        p.out.max_variants = maxv
        assert check(p) == code, maxv
        assert code == 0 or "max_variants" in last()
    for maxt, code in ((0, ERR_RANGE), (1, ERR_RANGE), (2, 0)):
        p = Prepared()
        p.out.max_text = maxt
        assert check(p) == code, maxt
        assert code == 0 or "max_text" in last()


def test_validate_a_decompose_result_with_missing_arrays():
    for field in ("status", "forward", "secdecomp"):
        p = Prepared()
        setattr(p.res, field, None)
        assert check(p) == ERR_ARG and field.split("_")[0] in last(), field
    for field in ("slice_begin", "slice_len", "ref_pos", "ops", "ops_len"):
        for a in range(2):
            p = Prepared()
            getattr(p.res, field)[a] = None
            assert check(p) == ERR_ARG and "allele %d" % (a + 1) in last(), (field, a)
    p = Prepared()
    p.res.ops_offset[1] = C.POINTER(C.c_uint64)()
    assert check(p) == ERR_ARG and "ops_offset" in last()
    p = Prepared()  # the third alignment (allele 1 against allele 2) is not read
    p.res.ops[2] = None
    p.res.ops_len[2] = None
    assert check(p) == 0


def test_validate_the_job():
    for field in ("primary", "bc_offset", "bc_len"):
        p = Prepared()
        setattr(p.job.bc, field, None)
        assert check(p) == ERR_ARG and "primary" in last(), field
    for field in ("data", "offset", "length"):
        p = Prepared()
        setattr(p.job.refs, field, None)
        assert check(p) == ERR_ARG and "refs" in last(), field
    p = Prepared()
    p.job.refs.kind = capi.SEQ_PROFILE
    assert check(p) == ERR_ARG
    p = Prepared()
    p.job.dprm.trim_left = -1
    assert check(p) == ERR_ARG and "trim" in last()
    p = Prepared()
    idx = np.array([0, 2], np.uint32)
    p.job.ref_index = capi._u32p(idx)
    assert check(p) == ERR_ARG and "trace 1" in last()


def test_the_calls_answer_the_same_before_they_look_for_a_device():
    lib = capi.lib()
    p = Prepared()
    p.out.max_variants = 2000
    assert lib.tracyhip_decompose_variants(None, C.byref(p.job), C.byref(p.res), capi._u32p(p.slice_pos), C.byref(p.prm), 0, C.byref(p.out)) == ERR_RANGE
    p = Prepared()
    assert lib.tracyhip_decompose_variants(None, C.byref(p.job), C.byref(p.res), capi._u32p(p.slice_pos), C.byref(p.prm), 0, C.byref(p.out)) == ERR_ARG
    assert "context" in last()
    assert lib.tracyhip_decompose_variants_async(None, C.byref(p.job), C.byref(p.res), capi._u32p(p.slice_pos), C.byref(p.prm), 0, C.byref(p.out)) == ERR_ARG
    # the stage: capacities, memory kind and null arrays are refused without a context
    z = np.zeros(8, np.uint8)
    u64, u32, i32 = np.zeros(2, np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.int32)
    b = p.buf.struct
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def stage(maxv=4, maxt=16, mem=0, rows1=z, var=b.var, nt=1):
        return lib.tracyhip_call_variants(None, C.c_uint32(nt), ptr(z), ptr(rows1) if rows1 is not None else None, ptr(u64), ptr(u32), ptr(i32), ptr(z),
                                          ptr(u32), C.c_uint32(20), C.c_uint32(20), C.c_uint32(maxv), C.c_uint32(maxt), mem, C.c_void_p(var),
                                          C.c_void_p(b.text), C.c_void_p(b.var_n), C.c_void_p(b.var_flags))
    assert stage(maxv=0) == ERR_RANGE and stage(maxv=1025) == ERR_RANGE and stage(maxt=1) == ERR_RANGE
    assert stage(mem=3) == ERR_ARG and stage(rows1=None) == ERR_ARG and stage(var=None) == ERR_ARG
    assert stage() == ERR_ARG and "context" in last()


def test_record_layout_and_call_stats():
    assert C.sizeof(capi.Variant) == 32 == capi.VARIANT_DTYPE.itemsize
    assert [n for n, _ in capi.Variant._fields_] == ["pos", "basenum", "gt", "call_index", "ref_off", "ref_len", "alt_off", "alt_len"]
    assert [getattr(capi.Variant, n).offset for n, _ in capi.Variant._fields_] == list(range(0, 32, 4))
    # the four counters come behind denovo_steps, where CallStats ended before them
    assert [n for n, _ in capi.CallStatsVariants._fields_] == ["var_traces", "var_realigned", "var_truncated", "var_chunks"]
    assert capi.CallStatsVariants.var_traces.offset == C.sizeof(capi.CallStats) == capi.CallStats.denovo_steps.offset + 4
    assert C.sizeof(capi.CallStatsVariants) == C.sizeof(capi.CallStats) + 16


def test_host_batch_entry_points_against_the_oracle():
    """tracyhost_call_variants_batch / tracyhost_revcomp_batch (the command line's host path behind a C entry point, which
    tools/variants_device_line.py times beside the device call): the named cases and random pairs, in the device call's record layout"""
    import variants_cases as vc
    from sage_oracle import revcomp
    from tracy_amd import hostlib
    hl = hostlib.lib()
    named = vc.named_cases()
    cases = [named[k] for k in sorted(named)] + vc.random_cases(40)
    nt = len(cases)
    rows = [(a[0], a[1]) for c in cases for a in (c["a"], c["b"])]
    r0, r1, off, lens = capi._pack_rows(rows)
    pos = np.array([a[2] for c in cases for a in (c["a"], c["b"])], np.int32)
    fwd = np.array([c["forward"] for c in cases], np.uint8)
    bl = np.array([c["bc_len"] for c in cases], np.uint32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    for maxv, maxt in ((128, 4096), (2, 4096), (128, 6)):
        b = capi.VariantBuffers(nt, maxv, maxt, fill=0xA5)
        s = b.struct
        assert hl.tracyhost_call_variants_batch(C.c_uint32(nt), ptr(r0), ptr(r1), capi._u64p(off), capi._u32p(lens), ptr(pos), ptr(fwd), capi._u32p(bl),
                                                C.c_uint32(vc.TRIMS[0]), C.c_uint32(vc.TRIMS[1]), C.c_uint32(maxv), C.c_uint32(maxt), C.c_void_p(s.var),
                                                C.c_void_p(s.text), C.c_void_p(s.var_n), C.c_void_p(s.var_flags), C.c_uint32(3)) == 0
        got, flags = b.lists()
        for t, c in enumerate(cases):
            want, n1, n2, text = vc.expected(c)
            fits = len(want) <= maxv and text <= maxt  # (the host code merges as it goes: only the merged list and its text count)
            assert int(flags[t]) == (0 if fits else 1) and got[t] == (want if fits else []), (t, maxv, maxt)
    seqs = [b"ACGTNacgtn", b"", b"A", b"GATTACA" * 30]
    src = np.frombuffer(b"".join(seqs) + b"\0", np.uint8).copy()
    ln = np.array([len(x) for x in seqs], np.uint32)
    so = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    dst = np.zeros(len(src), np.uint8)
    assert hl.tracyhost_revcomp_batch(ptr(src), capi._u64p(so), capi._u32p(ln), C.c_uint32(len(seqs)), ptr(dst), capi._u64p(so), C.c_uint32(2)) == 0
    for i, x in enumerate(seqs):
        assert dst[int(so[i]):int(so[i]) + len(x)].tobytes() == revcomp(x.upper()), i
