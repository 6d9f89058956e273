"""The variant-calling wave body of `tracy decompose -v` (tracy_amd/csrc/variants_wave.h: var_scan, var_merge, var_sort, call_index) on
the 64-fiber host wave against tests/indigo_oracle.py (call_variants over both alleles, sort_variants) -- every field, the text byte
by byte, the bytes around records and text untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import indigo_oracle as io
import variants_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 0xA5
REC = np.dtype([("pos", "<i4"), ("basenum", "<i4"), ("gt", "<i4"), ("call_index", "<u4"), ("ref_off", "<u4"), ("ref_len", "<u4"),
                ("alt_off", "<u4"), ("alt_len", "<u4")])


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_variants.so")
    srcs = [os.path.join(HERE, "emu", "emu_variants.cpp"), os.path.join(HERE, "emu", "host_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/variants_wave.h"), os.path.join(ROOT, "tracy_amd/csrc/dp_lane.h"),
            os.path.join(ROOT, "include/tracy_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]])
    lib = C.CDLL(so)
    lib.emu_var_scan.restype = C.c_uint32
    return lib


def _buf(b):
    return np.frombuffer(bytes(b) + b"\0", dtype=np.uint8).copy()


def run_case(emu, c, max_variants=64, max_text=1024, trims=vc.TRIMS):
    """-> (list of dicts as variants_cases.expected gives them, flags); checks the guard bytes around records and text"""
    pad = 4
    var = np.full((max_variants + 2 * pad) * REC.itemsize, GUARD, np.uint8)
    text = np.full(max_text + 64, GUARD, np.uint8)
    n = np.full(3, 0x5a5a5a5a, np.uint32)
    fl = np.full(3, 0x5a5a5a5a, np.uint32)
    bufs = [_buf(x) for x in (c["a"][0], c["a"][1], c["b"][0], c["b"][1])]
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    rc = emu.emu_variants(p(bufs[0]), p(bufs[1]), C.c_uint32(len(c["a"][0])), C.c_int32(c["a"][2]), p(bufs[2]), p(bufs[3]),
                          C.c_uint32(len(c["b"][0])), C.c_int32(c["b"][2]), C.c_uint32(int(c["forward"])), C.c_uint32(c["bc_len"]),
                          C.c_uint32(trims[0]), C.c_uint32(trims[1]), C.c_uint32(max_variants), C.c_uint32(max_text),
                          p(var, pad * REC.itemsize), p(text, 32), p(n, 4), p(fl, 4))
    assert rc == 0
    assert n[0] == 0x5a5a5a5a and n[2] == 0x5a5a5a5a and fl[0] == 0x5a5a5a5a and fl[2] == 0x5a5a5a5a
    recs = var[pad * REC.itemsize:(pad + max_variants) * REC.itemsize].view(REC)
    body = text[32:32 + max_text]
    got, used = decode(recs, body, int(n[1]))
    assert (var[:pad * REC.itemsize] == GUARD).all() and (var[(pad + max_variants) * REC.itemsize:] == GUARD).all(), "records: guard"
    assert (var[(pad + int(n[1])) * REC.itemsize:] == GUARD).all(), "records behind var_n"
    assert (text[:32] == GUARD).all() and (text[32 + used:] == GUARD).all(), "text: guard"
    return got, int(fl[1])


def decode(recs, body, n):
    """records + text region of one trace -> the dicts; checks the packing (ref then alt, record after record from 0)"""
    got, at = [], 0
    for r in recs[:n]:
        assert int(r["ref_off"]) == at and int(r["alt_off"]) == at + int(r["ref_len"]), "text packing"
        ref = body[at:at + int(r["ref_len"])].tobytes()
        alt = body[int(r["alt_off"]):int(r["alt_off"]) + int(r["alt_len"])].tobytes()
        at += int(r["ref_len"]) + int(r["alt_len"])
        got.append(dict(pos=int(r["pos"]), basenum=int(r["basenum"]), gt=int(r["gt"]), ref=ref, alt=alt, call_index=int(r["call_index"])))
    return got, at


NAMED = vc.named_cases()


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case(emu, name):
    c = NAMED[name]
    want = vc.expected(c)[0]
    got, flags = run_case(emu, c)
    assert flags == 0 and got == want, (name, got, want)


def test_fixture_named_cases_say_what_their_names_say():
    """A check of the FIXTURES, not of the code under test (it runs the oracle only): every named case of tests/variants_cases.py holds the
    event, the drop or the tie its name promises, so that test_named_case compares the wave body on the situations the names list."""
    ex = lambda n: vc.expected(NAMED[n])[0]
    assert ex("no_base_in_row0") == [] and ex("zero_length") == []
    assert [(v["pos"], v["basenum"]) for v in ex("snv_first_last_of_span")] == [(13, 1), (17, 5)]
    assert ex("leading_insertion_dropped") == [dict(pos=13, basenum=5, gt=1, ref=b"C", alt=b"A", call_index=24)]
    assert [(v["ref"], v["alt"]) for v in ex("trailing_insertion_never_flushed")] == [(b"C", b"G")]
    assert [v["pos"] for v in ex("leading_reference_columns")] == [106]
    assert [(v["ref"], v["alt"]) for v in ex("deletion_after_insertion")] == [(b"C", b"CGG"), (b"CTT", b"C")]
    assert [(v["ref"], v["alt"]) for v in ex("insertion_after_deletion")] == [(b"CTT", b"C"), (b"T", b"TGG")]
    assert [(v["ref"], len(v["alt"])) for v in ex("deletion_after_long_insertion")] == [(b"C", 81), (b"CACG", 1)]
    assert [(v["ref"], v["alt"]) for v in ex("n_in_ref_of_snv")] == [(b"G", b"C")]
    assert ex("n_inside_deletion") == [] and ex("n_as_deletion_anchor") == []
    assert [(v["ref"], v["alt"]) for v in ex("n_in_alt_kept")] == [(b"C", b"N"), (b"T", b"TNN")]
    assert ex("pos0_zero_event_at_zero") == [dict(pos=4, basenum=4, gt=1, ref=b"A", alt=b"T", call_index=23)]
    assert [v["pos"] for v in ex("negative_pos_dropped")] == [2]
    assert all(v["pos"] > (1 << 30) for v in ex("pos0_large")) and {v["gt"] for v in ex("pos0_large")} == {2}
    same = ex("same_on_both_alleles")
    assert [v["gt"] for v in same if len(v["ref"]) > 1] == [2] and [v["gt"] for v in same if (v["ref"], v["alt"]) == (b"C", b"G")] == [2]
    assert [v["basenum"] for v in same if v["gt"] == 2] == [7, 10]  # allele 1's, allele 2 counts its two inserted bases on top
    tie = ex("two_snvs_one_pos_tie")
    assert [(v["pos"], v["basenum"], v["alt"]) for v in tie] == [(45, 5, b"C"), (45, 5, b"G")]
    many = ex("more_than_16_with_ties")
    assert len(many) == 40 and [v["alt"] for v in many] == [b"C", b"T"] * 20
    assert [v["call_index"] for v in ex("reverse_strand_call_index")] == [321 - 25, 321 - 25, 321 - 27]


@pytest.mark.parametrize("name,c,max_variants,max_text,fits", vc.capacity_cases(), ids=[x[0] for x in vc.capacity_cases()])
def test_capacity(emu, name, c, max_variants, max_text, fits):
    assert vc.fits(c, max_variants, max_text) == fits
    got, flags = run_case(emu, c, max_variants, max_text)  # (the guard bytes are checked in there)
    if fits:
        assert flags == 0 and got == vc.expected(c)[0]
    else:
        assert flags == 1 and got == []


def test_push_order_of_one_alignment(emu):
    """an insertion that closes on the column of an SNV is pushed first (variants.h:88-104)"""
    row0, row1 = b"ACGGTCA", b"AC--GCA"
    own = []
    io.call_variants(row0, row1, "chr", 10, own)
    assert [(v["ref"], v["alt"]) for v in own] == [("C", "CGG"), ("G", "T")]
    out = np.zeros(4 * 8, np.int32)
    b0, b1 = _buf(row0), _buf(row1)
    n = emu.emu_var_scan(C.c_void_p(b0.ctypes.data), C.c_void_p(b1.ctypes.data), C.c_uint32(len(row0)), C.c_int32(10), C.c_uint32(8),
                         C.c_void_p(out.ctypes.data))
    assert n == 2
    assert out[:8].reshape(2, 4).tolist() == [[v["pos"], v["basenum"], len(v["ref"]), len(v["alt"])] for v in own]


def test_random_pairs(emu):
    cases = vc.random_cases(300)
    events = 0
    for i, c in enumerate(cases):
        want = vc.expected(c)[0]
        got, flags = run_case(emu, c, max_variants=128, max_text=4096)
        assert flags == 0 and got == want, (i, c)
        events += len(want)
    assert events > 2000 and any(v["gt"] == 2 for c in cases for v in vc.expected(c)[0])
