"""The argument rules of a wildtype job (tracyhip_align_job::refs of kind PROFILE, tracyhip_align_result::rows0 / rows1) as
tracyhip_align_validate states them, on a machine without a GPU: the validate call touches no device.  Also the layout of the job
(which must not have grown), of the grown result struct and of tracyhip_call_stats as a C compiler sees them against the ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np

from tracy_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = capi.ERR_ARG
SCORE = (3, -5, -10, -4)


def last():
    return capi.lib().tracyhip_last_error().decode()


def profiles(n, cols=120, seed=3):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.random((6, cols), dtype=np.float32)) for _ in range(n)]


def wildtype_job(nt=3, nw=None, ref_index=None, rows=True):
    return capi.PreparedAlign(profiles(nt), None, SCORE, 50, 50, ref_index=ref_index, ref_profiles=profiles(nt if nw is None else nw, 110, 4), rows=rows)


def fasta_job(nt=3):
    return capi.PreparedAlign(profiles(nt), [b"ACGT" * 100] * nt, SCORE, 50, 50)


def validate(p, mem=capi.MEM_HOST):
    return capi.lib().tracyhip_align_validate(C.byref(p.job), C.byref(p.prm), mem, C.byref(p.out))


def test_layout_matches_the_header(tmp_path):
    structs = (("tracyhip_align_job", capi.AlignJob), ("tracyhip_align_result", capi.AlignResult), ("tracyhip_call_stats", capi.CallStatsWildtype))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tracy_hip.h"', 'int main(void) {']
    for cname, ct in structs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
    lines.append('  printf("%zu %zu %zu %zu\\n", offsetof(tracyhip_align_job, refs), offsetof(tracyhip_align_result, rows0),'
                 ' offsetof(tracyhip_align_result, rows1), offsetof(tracyhip_call_stats, wt_chunks));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for (cname, ct), line in zip(structs, out):
        assert line.split() == [cname, str(C.sizeof(ct))]
    assert [int(x) for x in out[3].split()] == [capi.AlignJob.refs.offset, capi.AlignResult.rows0.offset, capi.AlignResult.rows1.offset,
                                                capi.CallStatsWildtype.wt_chunks.offset]
    # the job has not grown (a wildtype job is told by the kind of refs): 136 bytes, the trim arrays its last members; the new members of
    # the other two are appended behind what was the last before
    assert C.sizeof(capi.AlignJob) == 136 == capi.AlignJob.trim_right_each.offset + 8
    assert capi.AlignResult.rows0.offset == capi.AlignResult.ops_len.offset + 8
    assert capi.CallStatsWildtype.wt_chunks.offset == C.sizeof(capi.CallStatsSeed)


def test_a_wildtype_job_validates():
    assert validate(wildtype_job()) == 0 and validate(wildtype_job(), capi.MEM_DEVICE) == 0
    assert validate(wildtype_job(rows=False)) == 0                                   # the rows are optional
    assert validate(wildtype_job(5, 2, ref_index=[0, 1, 1, 0, 1])) == 0              # shared wildtypes
    assert validate(wildtype_job(3, 5)) == 0                                         # more wildtypes than traces, identity
    assert wildtype_job().job.refs.kind == capi.SEQ_PROFILE                          # what makes it a wildtype job
    assert validate(wildtype_job(0)) == 0


def test_a_zero_initialised_tail_is_todays_job():
    p = fasta_job()
    assert p.job.refs.kind == capi.SEQ_CHAR and not p.out.rows0 and not p.out.rows1
    assert validate(p) == 0
    job, out = capi.AlignJob(), capi.AlignResult()
    assert capi.lib().tracyhip_align_validate(C.byref(job), C.byref(p.prm), capi.MEM_HOST, C.byref(out)) == 0  # no traces


def test_wildtype_profiles_marked_as_kind_char():
    """the same payload under kind CHAR is a FASTA job: the rows are refused for it (without them it would be read as letters)"""
    p = wildtype_job()
    p.job.refs.kind = capi.SEQ_CHAR
    assert validate(p) == ERR_ARG and "wildtype" in last() and "PROFILE" in last()
    p.job.refs.kind = 7
    assert validate(p) == ERR_ARG


def test_wildtype_profiles_without_offsets_lengths_or_payload():
    for field in ("offset", "length"):
        p = wildtype_job()
        setattr(p.job.refs, field, None)
        assert validate(p) == ERR_ARG and "sequence sets" in last(), field
    p = wildtype_job()
    p.job.refs.data = None
    assert validate(p) == ERR_ARG and "payload" in last()


def test_fewer_wildtypes_than_traces_without_ref_index():
    p = wildtype_job(3, 2, ref_index=[0, 1, 1])
    assert validate(p) == 0
    p.job.ref_index = C.POINTER(C.c_uint32)()
    assert validate(p) == ERR_ARG and "ref_index" in last()


def test_rows_on_a_fasta_job():
    p = fasta_job()
    keep = np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)
    p.out.rows0, p.out.rows1 = keep[0].ctypes.data, keep[1].ctypes.data
    assert validate(p) == ERR_ARG and "wildtype" in last()


def test_one_row_array_without_the_other():
    for drop in ("rows0", "rows1"):
        p = wildtype_job()
        setattr(p.out, drop, None)
        assert validate(p) == ERR_ARG and "together" in last(), drop
        f = fasta_job()
        keep = np.zeros(4096, np.uint8)
        setattr(f.out, drop, keep.ctypes.data)
        assert validate(f) == ERR_ARG and "together" in last(), drop


# ---- tracyhip_decompose_validate: ref_profiles, with and without `oriented` ----------------------------------------------------------
def decompose_job(nt=2):
    """a well-formed decompose job (tests/test_trims_each_host.py) with a wildtype profile per reference, of each reference's length"""
    from test_trims_each_host import Decompose
    d = Decompose(nt)
    lens = [int(d.job.refs.length[i]) for i in range(d.job.refs.count)]
    d.wt = capi.PackedSeqs(profiles(len(lens), 1, 5) if not lens else [np.ascontiguousarray(np.full((6, n), 0.1, np.float32)) for n in lens],
                           capi.SEQ_PROFILE)
    d.job.ref_profiles = d.wt.seqset()
    return d


def test_decompose_ref_profiles_without_oriented_validates():
    d = decompose_job()
    assert not d.job.oriented
    assert d.check() == 0 and d.check(capi.MEM_DEVICE) == 0
    keep = np.ones(2, np.uint8)
    d.job.oriented = keep.ctypes.data_as(C.POINTER(C.c_uint8))  # with `oriented`, as it was
    assert d.check() == 0


def test_decompose_ref_profiles_that_do_not_match_refs():
    d = decompose_job()
    d.wt.length[1] += 1
    assert d.check() == ERR_ARG and "differ in length" in last()
    d = decompose_job()
    d.job.ref_profiles.kind = capi.SEQ_CHAR
    assert d.check() == ERR_ARG and "PROFILE" in last()
    for field in ("offset", "length"):
        d = decompose_job()
        setattr(d.job.ref_profiles, field, None)
        assert d.check() == ERR_ARG and "ref_profiles" in last(), field
    d = decompose_job()
    d.job.ref_profiles.count = 1
    assert d.check() == ERR_ARG and "parallel" in last()
