"""Per-trace trims (trim_left_each / trim_right_each of tracyhip_align_job, tracyhip_decompose_job and tracyhip_seed_params) on a
machine without a GPU: the layout of the three structs as a C compiler sees them against the ctypes structs, the argument rules of
tracyhip_align_validate / tracyhip_decompose_validate / tracyhip_decompose_variants_validate, and the Python argument forms.  (That
the wave bodies and planning rules kept their signatures is what the unchanged tests/test_emu_variants.py, test_emu_decomp*.py and
test_plan_rules_host.py show: their sources compile against the changed headers.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tracy_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = capi.ERR_ARG
STRUCTS = (("tracyhip_align_job", capi.AlignJob), ("tracyhip_decompose_job", capi.DecomposeJob), ("tracyhip_seed_params", capi.SeedParams))


def last():
    return capi.lib().tracyhip_last_error().decode()


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every offsetof of the three changed structs, printed by a C program compiled against include/tracy_hip.h"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tracy_hip.h"', 'int main(void) {']
    for cname, ct in STRUCTS:
        lines.append('  printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f, _ in ct._fields_:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for (cname, ct), line in zip(STRUCTS, out):
        w = line.split()
        assert w[0] == cname
        assert int(w[1]) == C.sizeof(ct), cname
        assert [int(x) for x in w[2:]] == [getattr(ct, f).offset for f, _ in ct._fields_], cname
    # appended: the fields every struct had keep their places, the two arrays are its last two members
    for _, ct in STRUCTS:
        assert [f for f, _ in ct._fields_][-2:] == ["trim_left_each", "trim_right_each"]


# ---- tracyhip_align_validate ---------------------------------------------------------------------------------------------------------
class Align:
    """a well-formed align job of `nt` traces on host arrays"""

    def __init__(self, nt=3, trims=(50, 50)):
        rng = np.random.default_rng(3)
        profs = [np.ascontiguousarray(rng.random((6, 120), dtype=np.float32)) for _ in range(nt)]
        self.p = capi.PreparedAlign(profs, [b"ACGT" * 100] * nt, (3, -5, -10, -4), trims[0], trims[1])

    def check(self, mem=capi.MEM_HOST, job=True, prm=True, out=True):
        p = self.p
        return capi.lib().tracyhip_align_validate(C.byref(p.job) if job else None, C.byref(p.prm) if prm else None, mem, C.byref(p.out) if out else None)


def test_align_validate_accepts_scalars_arrays_and_an_empty_job():
    assert Align().check() == 0 and Align().check(capi.MEM_DEVICE) == 0
    a = Align(3, ([0, 10, 77], [20, 0, 90]))
    assert a.check() == 0
    assert [a.p.job.trim_left_each[i] for i in range(3)] == [0, 10, 77] and [a.p.job.trim_right_each[i] for i in range(3)] == [20, 0, 90]
    assert Align(3, (7, [1, 2, 3])).check() == 0  # an int beside an array is repeated
    assert Align(0).check() == 0
    big = Align(2, ([1 << 31, 0xFFFFFFFF], [0, 0]))  # an align trim is uint32: any value is an argument (createProfile's clamp takes it)
    assert big.check() == 0


def test_align_validate_one_array_without_the_other():
    for keep in ("trim_left_each", "trim_right_each"):
        a = Align(3, ([1, 2, 3], [4, 5, 6]))
        setattr(a.p.job, "trim_right_each" if keep == "trim_left_each" else "trim_left_each", C.POINTER(C.c_uint32)())
        assert a.check() == ERR_ARG and "together" in last(), keep
        e = Align(0)  # ... whatever the number of traces
        setattr(e.p.job, keep, capi._u32p(np.zeros(1, np.uint32)))
        assert e.check() == ERR_ARG and "together" in last(), keep


def test_align_validate_null_arguments_and_arrays():
    a = Align()
    assert a.check(mem=2) == ERR_ARG and "mem" in last()
    for kw in ("job", "prm", "out"):
        assert a.check(**{kw: False}) == ERR_ARG, kw
    for field in ("score_fwd", "score_rev", "forward", "slice_begin", "slice_len", "ref_pos", "score_final", "ops", "ops_len"):
        a = Align()
        setattr(a.p.out, field, None)
        assert a.check() == ERR_ARG and "result" in last(), field
    a = Align()
    a.p.out.ops_offset = C.POINTER(C.c_uint64)()
    assert a.check() == ERR_ARG
    a = Align()
    a.p.out.score_prelim = None  # optional
    assert a.check() == 0
    for field in ("offset", "length"):
        for which in ("profiles", "refs"):
            a = Align()
            setattr(getattr(a.p.job, which), field, None)
            assert a.check() == ERR_ARG and "sequence sets" in last(), (which, field)


def test_a_job_with_arrays_and_no_context_is_refused_for_the_context():
    """the compute call itself still needs a context, with or without arrays: only the validate calls work without a device"""
    a = Align(3, ([1, 2, 3], [4, 5, 6]))
    assert capi.lib().tracyhip_align_traces(None, C.byref(a.p.job), C.byref(a.p.prm), 0, C.byref(a.p.out)) == ERR_ARG and "context" in last()


# ---- tracyhip_decompose_validate / tracyhip_decompose_variants_validate ----------------------------------------------------------------
class Decompose:
    """a well-formed decompose job of `nt` traces of 100 basecalls on host arrays (peak-table form), and a variants call over it"""

    def __init__(self, nt=2, trims=None):
        from test_variants_abi import Prepared
        v = self.v = Prepared(nt)
        k = v.keep
        n = max(nt, 1)
        rng = np.random.default_rng(4)
        self.profs = capi.PackedSeqs([np.ascontiguousarray(rng.random((6, 100), dtype=np.float32)) for _ in range(nt)], capi.SEQ_PROFILE)
        job, res = self.job, self.res = v.job, v.res
        job.profiles = self.profs.seqset()
        k["sec"] = np.full(n * 100, ord("C"), np.uint8)
        k["peaks"] = np.zeros(n * 400, np.int32)
        job.bc.secondary = k["sec"].ctypes.data
        job.bc.peaks = k["peaks"].ctypes.data
        k["bp"] = (capi.Breakpoint * n)()
        k["dst"] = (capi.DecompStatus * n)()
        res.bp, res.dstatus = C.addressof(k["bp"]), C.addressof(k["dst"])
        for name, dt, per in (("score_fwd", np.int32, 1), ("score_rev", np.int32, 1), ("score_trim", np.int32, 1), ("dcp_indel", np.int32, 2002),
                              ("dcp_err", np.int32, 2002), ("fractions", np.float64, 2)):
            k[name] = np.zeros(n * per, dt)
            setattr(res, name, k[name].ctypes.data)
        k["dcp_off"] = np.arange(n, dtype=np.uint64) * 2002
        res.dcp_offset = capi._u64p(k["dcp_off"])
        for a in range(3):
            k["score%d" % a] = np.zeros(n, np.int32)
            res.score[a] = k["score%d" % a].ctypes.data
        k["ops2"], k["off2"], k["len2"] = np.zeros(n * 300, np.uint8), np.arange(n, dtype=np.uint64) * 300, np.zeros(n, np.uint32)
        res.ops[2], res.ops_offset[2], res.ops_len[2] = k["ops2"].ctypes.data, capi._u64p(k["off2"]), k["len2"].ctypes.data
        if trims is not None:
            job.dprm = capi.DecompParams(0, 0, 1000, 5)
            k["trims"] = capi.trims_each(job, trims[0], trims[1], nt)

    def check(self, mem=capi.MEM_HOST, job=True, prm=True, out=True):
        return capi.lib().tracyhip_decompose_validate(C.byref(self.job) if job else None, C.byref(self.v.prm) if prm else None, mem,
                                                      C.byref(self.res) if out else None)

    def check_variants(self):
        from test_variants_abi import check
        return check(self.v)


def test_decompose_validate_accepts_scalars_arrays_and_an_empty_job():
    d = Decompose()
    assert d.check() == 0 and d.check(capi.MEM_DEVICE) == 0 and d.check_variants() == 0
    d = Decompose(2, ([0, 77], [90, 0]))
    assert d.check() == 0 and d.check_variants() == 0
    d = Decompose(2, ([0x7FFFFFFF, 0], [0, 0x7FFFFFFF]))  # INT32_MAX itself is a trim
    assert d.check() == 0 and d.check_variants() == 0
    assert Decompose(0).check() == 0


def test_decompose_validate_one_array_without_the_other():
    for drop in ("trim_left_each", "trim_right_each"):
        d = Decompose(2, ([1, 2], [3, 4]))
        setattr(d.job, drop, C.POINTER(C.c_uint32)())
        assert d.check() == ERR_ARG and "together" in last(), drop
        assert d.check_variants() == ERR_ARG and "together" in last(), drop


@pytest.mark.parametrize("side", [0, 1])
def test_decompose_validate_a_trim_of_two_to_the_31(side):
    """IndigoConfig holds the trims as int: a per-trace value above INT32_MAX is the per-trace form of a negative trim"""
    for value in (1 << 31, 0xFFFFFFFF):
        trims = [[5, 6], [7, 8]]
        trims[side][1] = value
        d = Decompose(2, trims)
        assert d.check() == ERR_ARG and "trace 1" in last(), value
        assert d.check_variants() == ERR_ARG and "trace 1" in last(), value
    d = Decompose(2, ([5, 6], [7, 8]))
    d.job.dprm.trim_left = -1  # with arrays the scalars are ignored
    assert d.check() == 0 and d.check_variants() == 0


def test_decompose_validate_null_arguments_and_arrays():
    d = Decompose()
    assert d.check(mem=2) == ERR_ARG and "mem" in last()
    for kw in ("job", "prm", "out"):
        assert d.check(**{kw: False}) == ERR_ARG, kw
    for field in ("bp", "status", "score_fwd", "score_rev", "forward", "score_trim", "dcp_indel", "dcp_err", "dstatus", "secdecomp", "fractions"):
        d = Decompose()
        setattr(d.res, field, None)
        assert d.check() == ERR_ARG and "result" in last(), field
    for field in ("primary", "secondary", "bc_offset", "bc_len", "peaks"):  # (peaks: no signal + bcpos to build the table from either)
        d = Decompose()
        setattr(d.job.bc, field, None)
        assert d.check() == ERR_ARG and "basecall" in last(), field
    for a in range(3):
        for field in ("score", "ops", "ops_len"):
            d = Decompose()
            getattr(d.res, field)[a] = None
            assert d.check() == ERR_ARG and "allele" in last(), (field, a)
    for a in range(2):
        for field in ("slice_begin", "slice_len", "ref_pos"):
            d = Decompose()
            getattr(d.res, field)[a] = None
            assert d.check() == ERR_ARG and "slice" in last(), (field, a)


# ---- the Python argument forms -----------------------------------------------------------------------------------------------------
def test_trims_each_argument_forms():
    job = capi.AlignJob()
    assert capi.trims_each(job, 50, 60, 4) == () and (job.trim_left, job.trim_right) == (50, 60) and not job.trim_left_each
    keep = capi.trims_each(job, np.array([1, 2, 3, 4]), (9, 8, 7, 6), 4)
    assert [job.trim_left_each[i] for i in range(4)] == [1, 2, 3, 4] and [job.trim_right_each[i] for i in range(4)] == [9, 8, 7, 6]
    assert len(keep) == 2 and all(a.dtype == np.uint32 for a in keep)
    with pytest.raises(ValueError):
        capi.trims_each(capi.AlignJob(), [1, 2, 3], 5, 4)
    dj = capi.DecomposeJob()
    capi.trims_each(dj, 20, 30, 2)
    assert (dj.dprm.trim_left, dj.dprm.trim_right) == (20, 30)
    sp = capi.SeedParams(0, 0, 15, 3, 1000)
    keep = capi.trims_each(sp, [14, 50], [50, 13], 2)
    assert sp.trim_left_each[0] == 14 and sp.trim_right_each[1] == 13
