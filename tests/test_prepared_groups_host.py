"""PreparedAssemble / PreparedDenovo (tracy_amd/capi.py) on ragged groups, without a GPU: group_first, the per-group offsets and the
array sizes against the capacities include/tracy_hip.h asks for, restated here --
    assemble: (K + 1) * (n_ref + sum_len) bytes of rows and n_ref + sum_len columns per group,
    de novo:  K * sum_len bytes of rows and sum_len columns per group
-- and tracyhip_assemble_validate / tracyhip_denovo_validate (which touch no device) accept every one."""
import ctypes as C

import numpy as np
import pytest

SCORE = (3, -5, -10, -4)
# trace lengths per group: groups of 0, 1 and 3 traces of 5 .. 40 columns, the empty group first, in the middle, last
SHAPES = {
    "empty_first": ((), (17,), (5, 40, 23)),
    "empty_middle": ((9, 31, 12), (), (40,)),
    "empty_last": ((5,), (28, 6, 33), ()),
    "two_empty": ((), (7, 19, 40), (), (11,)),
    "none_empty": ((40, 5, 5), (13,)),
}
REF_LENS = (21, 8, 37, 14)


def profiles(lens):
    return [np.full((6, n), 0.1, np.float32) for n in lens]


def expected(shape, rows_of, cols_of):
    """first, roff, coff and the totals from the formulas of the header: rows_of(K), cols_of(g, sum_len)"""
    first, roff, coff, rtot, ctot = [0], [], [], 0, 0
    for g, lens in enumerate(shape):
        first.append(first[-1] + len(lens))
        roff.append(rtot)
        coff.append(ctot)
        rtot += rows_of(len(lens)) * cols_of(g, sum(lens))
        ctot += cols_of(g, sum(lens))
    return first, roff, coff, rtot, ctot


def check_layout(p, shape, trace_fields, rows_of, cols_of):
    first, roff, coff, rtot, ctot = expected(shape, rows_of, cols_of)
    ng, nt = len(shape), first[-1]
    assert (p.ng, p.nt) == (ng, nt) and p.job.ngroups == ng
    assert p.first.dtype == np.uint32 and p.first.tolist() == first
    assert [p.job.group_first[g] for g in range(ng + 1)] == first
    assert p.roff.dtype == np.uint64 and p.roff.tolist() == roff and p.coff.dtype == np.uint64 and p.coff.tolist() == coff
    assert [p.out.rows_offset[g] for g in range(ng)] == roff and [p.out.col_offset[g] for g in range(ng)] == coff
    assert set(p.res) == set(trace_fields) | {"nrows", "ncol", "cons_len", "rows", "gapped", "cons", "qual"}
    assert p.res["rows"].nbytes == max(rtot, 1)
    for k in ("gapped", "cons", "qual"):
        assert p.res[k].nbytes == max(ctot, 1), k
    for k in trace_fields:
        assert len(p.res[k]) == max(nt, 1), k
    for k in ("nrows", "ncol", "cons_len"):
        assert len(p.res[k]) == max(ng, 1) and p.res[k].dtype == np.uint32, k
    for k, v in p.res.items():  # the result struct points at these arrays
        assert getattr(p.out, k) == v.ctypes.data, k
    r = p.results()  # nothing ran: every group comes back without rows
    assert all(len(r[k]) == nt for k in trace_fields) and all(len(r[k]) == ng for k in ("nrows", "ncol", "cons_len"))
    assert r["rows"] == [[] for _ in range(ng)] and r["gapped"] == [b""] * ng and r["cons"] == [b""] * ng and r["qual"] == [b""] * ng


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("shared_reference", [False, True])
def test_assemble_layout_and_validation(name, shared_reference):
    from tracy_amd import capi
    shape = SHAPES[name]
    groups = [profiles(lens) for lens in shape]
    if shared_reference:  # every group on reference 1 of two
        refs, ridx = profiles(REF_LENS[:2]), [1] * len(shape)
        n_ref = lambda g: REF_LENS[1]
    else:
        refs, ridx = profiles(REF_LENS[:len(shape)]), None
        n_ref = lambda g: REF_LENS[g]
    p = capi.PreparedAssemble(groups, refs, SCORE, ref_index=ridx)
    check_layout(p, shape, ("score_fwd", "score_rev", "forward", "rank"), lambda K: K + 1, lambda g, s: n_ref(g) + s)
    assert (p.ridx is None) == (not shared_reference)
    for mem in (capi.MEM_HOST, capi.MEM_DEVICE):
        assert capi.lib().tracyhip_assemble_validate(C.byref(p.job), C.byref(p.prm), mem, C.byref(p.out)) == 0, capi.lib().tracyhip_last_error()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_denovo_layout_and_validation(name):
    from tracy_amd import capi
    shape = SHAPES[name]
    p = capi.PreparedDenovo([profiles(lens) for lens in shape], SCORE)
    check_layout(p, shape, ("forward", "partner", "row"), lambda K: K, lambda g, s: s)
    for mem in (capi.MEM_HOST, capi.MEM_DEVICE):
        assert capi.lib().tracyhip_denovo_validate(C.byref(p.job), C.byref(p.prm), mem, C.byref(p.out)) == 0, capi.lib().tracyhip_last_error()
