"""The counting hash table that device seeding spills its votes into (tracy_amd/csrc/seed.h: seed_table_capacity, seed_slot_of,
seed_table_insert, seed_table_best, the tie rule seed_better), built for the host with its own small g++ step and run on one thread
through the plain memory policy: (frequency, value) must be findMaxFreq's (tracy_amd/host/seed.hpp) on every list -- empty and single
lists, all equal, all distinct, 30-way ties (the smallest value wins), values down to -65 535 and near 2^62, values that all start
their probe in one slot, tables of the minimum 64 slots and of exactly 2 n, and every insertion order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "seed_mode.cpp")
FAR = 1 << 62


@pytest.fixture(scope="module")
def sm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("seedmode") / "seed_mode.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                    "-o", so, SRC, "-lz"], check=True, timeout=300)
    lib = C.CDLL(so)
    lib.sm_capacity.restype = C.c_uint64
    lib.sm_slot_of.restype = C.c_uint64
    lib.sm_empty.restype = C.c_int64
    lib.sm_run_all.restype = C.c_uint64
    return lib


def table(sm, votes, capacity=0):
    v = np.ascontiguousarray(votes, dtype=np.int64)
    out = np.zeros(2, np.int64)
    ok = sm.sm_table_mode(C.c_uint64(len(v)), v.ctypes.data_as(C.c_void_p), C.c_uint64(capacity), out.ctypes.data_as(C.c_void_p))
    assert ok == 1, "a vote found no slot"
    return int(out[0]), int(out[1])


def host(sm, votes):
    v = np.ascontiguousarray(votes, dtype=np.int64)
    out = np.zeros(2, np.int64)
    sm.sm_host_mode(C.c_uint64(len(v)), v.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1])


def stated(votes):
    """findMaxFreq in words: the count of the most frequent value and the smallest value with that count; (0, 0) for no votes"""
    if len(votes) == 0:
        return 0, 0
    vals, counts = np.unique(np.asarray(votes, dtype=np.int64), return_counts=True)
    return int(counts.max()), int(vals[counts == counts.max()].min())


def colliding(sm, capacity, slot, start, n):
    out, v = [], start
    while len(out) < n:
        if sm.sm_slot_of(C.c_int64(v), C.c_uint64(capacity)) == slot:
            out.append(v)
        v += 1
    return out


def test_capacity_and_marker(sm):
    assert sm.sm_empty() == -(1 << 63)
    for votes, want in [(0, 64), (1, 64), (32, 64), (33, 128), (2048, 4096), (2049, 8192), (14160, 32768), (46658, 131072)]:
        assert sm.sm_capacity(C.c_uint64(votes)) == want, votes


def test_small_lists(sm):
    for votes in ([], [0], [-65535], [FAR], [5, 5], [5, 4], [4, 5], [7, 7, 3, 3], [3, 3, 7, 7, 7], [-1, -2, -2, -1]):
        assert table(sm, votes) == host(sm, votes) == stated(votes), votes


def test_all_equal_and_all_distinct(sm):
    for n in (2, 31, 32, 33, 1000, 5000):
        for value in (-65535, 0, 12345, FAR):
            assert table(sm, [value] * n) == host(sm, [value] * n) == (n, value)
        d = np.arange(n, dtype=np.int64) * 7 - 65535
        assert table(sm, d[::-1]) == host(sm, d) == (1, -65535)
        assert table(sm, d + FAR) == (1, FAR - 65535)


def test_thirty_way_ties_smallest_wins(sm):
    rng = np.random.default_rng(20261019)
    for base in (-65535, 0, 123456789, FAR - 70000):
        for top in (400, 472):
            copies = base + np.arange(30, dtype=np.int64) * 601
            votes = np.concatenate([np.repeat(copies, top), base + rng.integers(0, 20000, 500)])
            want = stated(votes)
            assert want[0] >= top and want[1] <= base + 29 * 601
            for order in (votes, votes[::-1], np.sort(votes), rng.permutation(votes), rng.permutation(votes)):
                assert table(sm, order) == want == host(sm, order)


def test_probe_chains_in_one_slot(sm):
    """every value starts in the same slot: the chain is n long, and from the last slot it wraps; 64 slots and exactly 2 n"""
    for capacity in (64, 256):  # (4096 in the built-in suite below: finding its values takes millions of calls from here)
        n = capacity // 2
        assert sm.sm_capacity(C.c_uint64(n)) == capacity
        for slot in (0, capacity - 1, capacity // 2):
            for start in (-65535, FAR):
                v = colliding(sm, capacity, slot, start, n)
                assert table(sm, v, capacity) == (1, v[0]) == host(sm, v)
                w = list(v)
                for i in range(n // 4):
                    w[n - 1 - i] = v[i % 3]
                rng = np.random.default_rng(capacity + slot)
                for order in (w, w[::-1], list(rng.permutation(w))):
                    assert table(sm, order, capacity) == stated(w) == host(sm, w)


def test_seeded_lists_any_order(sm):
    rng = np.random.default_rng(7)
    for rep in range(300):
        n = int(rng.integers(0, 700))
        span = int(rng.integers(1, 8 if rep % 2 else 4000))
        base = (-65535, FAR, int(rng.integers(0, 50_000_000)), 0)[rep % 4]
        votes = base + rng.integers(0, span, n)
        want = stated(votes)
        assert host(sm, votes) == want
        assert table(sm, votes) == want and table(sm, rng.permutation(votes)) == want and table(sm, np.sort(votes)[::-1]) == want


def test_built_in_suite(sm):
    """the lists of tests/cpp/seed_mode_cases.h, which the stand-alone sanitizer program runs too"""
    lists = C.c_uint64(0)
    assert sm.sm_run_all(C.c_uint32(20261019), C.byref(lists)) == 0
    assert lists.value > 1000
