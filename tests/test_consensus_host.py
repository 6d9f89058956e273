"""The consensus column body of consensus_kernel (tracy_amd/csrc/consensus.h), built for the host with its own small g++ step: the gq
table against consensus_oracle.gt_letter, letters and qualities against the host gtLetter (consensus_out.hpp) on a million random and
adversarial weight vectors, and the fix-up screen under a log10 that differs from glibc's in the last ulps (the device's may)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "consensus_column.cpp")


@pytest.fixture(scope="module")
def cc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cons") / "consensus_column.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, SRC],
                   check=True, timeout=300)
    return C.CDLL(so)


def gq_table(cc):
    tab = np.zeros(10001, np.uint16)
    cc.cc_gq_table(tab.ctypes.data_as(C.c_void_p))
    return tab


def screen(cc, cl, iupac, ulps=0):
    cl = np.ascontiguousarray(cl, np.float32)
    n = cl.shape[0]
    letter, qual, flag = np.zeros(n, np.uint8), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    cc.cc_screen(C.c_uint64(n), cl.ctypes.data_as(C.c_void_p), C.c_int(int(iupac)), C.c_int(ulps), letter.ctypes.data_as(C.c_void_p),
                 qual.ctypes.data_as(C.c_void_p), flag.ctypes.data_as(C.c_void_p))
    return letter, qual, flag.astype(bool)


def host_gt(cc, cl, iupac):
    cl = np.ascontiguousarray(cl, np.float32)
    n = cl.shape[0]
    letter, qual = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    cc.cc_gt_letter(C.c_uint64(n), cl.ctypes.data_as(C.c_void_p), C.c_int(int(iupac)), letter.ctypes.data_as(C.c_void_p),
                    qual.ctypes.data_as(C.c_void_p))
    return letter, qual


def random_columns(n, seed):
    """trace-like and hostile class weights (A C G T N -) as float32"""
    rng = np.random.default_rng(seed)
    parts = []
    k = n // 8
    parts.append(rng.random((k, 6), dtype=np.float32))                                          # anything
    x = rng.random((k, 6), dtype=np.float32)
    x[:, 4:] = 0
    parts.append(x / x.sum(1, keepdims=True))                                                     # normalised trace columns
    x = rng.random((k, 6), dtype=np.float32) * (rng.random((k, 6)) < 0.4)
    parts.append(x.astype(np.float32))                                                            # zeros, all-zero columns
    x = np.zeros((k, 6), np.float32)
    x[np.arange(k), rng.integers(0, 6, k)] = 1
    x[np.arange(k), rng.integers(0, 6, k)] += rng.integers(0, 2, k).astype(np.float32)
    parts.append(x)                                                                               # one-hot, aligned one-hot sums
    x = rng.integers(0, 4, (k, 6)).astype(np.float32) / 4
    parts.append(x)                                                                               # equal classes, ties
    x = rng.random((k, 6), dtype=np.float32)
    x[:, :4] *= 0.05
    parts.append(x)                                                                               # N / gap-heavy columns
    # secondPL on a half-integer: two classes with ratio 10^(-(p + 0.5) / 10), and the float neighbours of the smaller
    p = rng.integers(0, 60, k)
    big = rng.integers(0, 4, k)
    sm = (big + 1 + rng.integers(0, 5, k)) % 6
    r = (10.0 ** (-(p + 0.5) / 10)).astype(np.float32)
    r = np.where(rng.random(k) < 0.5, np.nextafter(r, np.float32(1)), r)
    x = np.zeros((k, 6), np.float32)
    x[np.arange(k), big] = 1
    x[np.arange(k), sm] = r
    parts.append(x)
    # gl[second] = -1: a second class with a tenth of the column's weight
    a = rng.integers(1, 50, k).astype(np.float32)
    x = np.zeros((k, 6), np.float32)
    b1 = rng.integers(0, 4, k)
    b2 = (b1 + 1 + rng.integers(0, 3, k)) % 4
    x[np.arange(k), b1] = 9 * a
    x[np.arange(k), b2] = a
    parts.append(x)
    return np.concatenate(parts)


def _round(x):
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def test_gq_table_matches_oracle(cc):
    """the host gq table against consensus_oracle.gt_letter: every secondPL a column can reach through gt_letter itself, the rest
    through the oracle's own expression (gl >= -324 for any positive ratio, so PL 3240 .. 9999 has no column)"""
    import consensus_oracle as co
    tab = gq_table(cc)
    seen = set()
    for s in list(range(0, 3240)) + [10000]:
        cl = [1.0, 10.0 ** (-s / 10.0) if s < 10000 else 0.0, 0.0, 0.0, 0.0, 0.0]
        tot = sum(cl)
        gl = [max(math.log10(c / tot), -1000.0) if c > 0 else -1000.0 for c in cl]
        spl = int(_round(-10 * (gl[1] - gl[0])))
        _, q = co.gt_letter(cl, False)
        assert int(tab[spl]) == q, (s, spl)
        seen.add(spl)
    assert set(range(0, 3000)) <= seen and 10000 in seen
    for spl in range(10001):
        x = 1 - 1 / (math.pow(10.0, -0.0) + math.pow(10.0, -(spl / 10.0)))
        like = max(math.log10(x) if x > 0 else float("-inf"), -1000.0)
        assert int(tab[spl]) == max(int(_round(-10 * like)), 0), spl


@pytest.mark.parametrize("iupac", [False, True])
def test_letters_equal_gtletter_with_the_same_log10(cc, iupac):
    """with glibc's log10 on both sides the column body IS gtLetter: every column, flagged or not"""
    cl = random_columns(1 << 20, 7 + iupac)
    letter, qual, flag = screen(cc, cl, iupac)
    hl, hq = host_gt(cc, cl, iupac)
    assert np.array_equal(letter, hl)
    assert np.array_equal(qual.astype(np.uint32), hq)
    assert hq.max() <= 10000
    # the screen is narrow: random columns are almost never sent to the host
    assert flag[: 1 << 17].mean() < 1e-3


@pytest.mark.parametrize("iupac", [False, True])
@pytest.mark.parametrize("ulps", [1, 4])
def test_screen_catches_every_log10_difference(cc, iupac, ulps):
    """a log10 off by up to `ulps` ulps: every column matches gtLetter or is flagged, and the fixed-up result matches"""
    cl = random_columns(1 << 20, 100 + ulps + iupac)
    letter, qual, flag = screen(cc, cl, iupac, ulps)
    hl, hq = host_gt(cc, cl, iupac)
    differ = (letter != hl) | (qual.astype(np.uint32) != hq)
    assert not np.any(differ & ~flag), np.flatnonzero(differ & ~flag)[:10]
    fixed_l = np.where(flag, hl, letter)
    fixed_q = np.where(flag, hq, qual.astype(np.uint32))
    assert np.array_equal(fixed_l, hl) and np.array_equal(fixed_q, hq)
    # the adversarial blocks do reach the screen (half-integer PL, gl = -1 with IUPAC)
    k = (1 << 20) // 8
    assert flag[6 * k: 7 * k].any()
    if iupac:
        assert flag[7 * k:].mean() > 0.5


def test_hostile_columns(cc):
    """NaN, infinities, negative weights, huge and denormal values: flagged (or harmless), never a wrong unflagged letter"""
    f32 = np.finfo(np.float32)
    rows = [[0, 0, 0, 0, 0, 0], [np.nan, 1, 0, 0, 0, 0], [np.inf, 1, 0, 0, 0, 0], [-1, 2, 0, 0, 0, 0], [f32.max] * 6,
            [f32.tiny / 8, 0, 0, 0, 0, 0], [f32.tiny / 8, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 1e-30]]
    cl = np.array(rows, np.float32)
    for iupac in (False, True):
        letter, qual, flag = screen(cc, cl, iupac, 4)
        hl, hq = host_gt(cc, cl, iupac)
        for i in range(len(rows)):
            assert flag[i] or (letter[i] == hl[i] and qual[i] == hq[i]), (rows[i], iupac)
        assert flag[1] and flag[2] and flag[3]
