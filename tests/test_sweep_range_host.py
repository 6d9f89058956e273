"""The period of the offset form of the 16-bit sweeps (tracy_amd/csrc/sweep_range.h, sweep_diag_period_rule), built for the host
with its own small g++ step and checked against a direct statement of its arithmetic: on 10^5 seeded parameter sets and on the
edges -- |ge| where a period of 64 just fits and just does not, Q raised by what a launch reported, strips of one row, 1 024 rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sweep_range.cpp")
N = 100_000


@pytest.fixture(scope="module")
def sr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("range") / "sweep_range.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-o", so, SRC],
                   check=True, timeout=300)
    return C.CDLL(so)


def rules(sr, rows):
    x = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 10))
    out = np.zeros((x.shape[0], 2), np.int64)
    sr.sr_rules(C.c_uint64(x.shape[0]), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def period_stated(match, mismatch, go, ge, hfree, vfree, K, lanes, Q):
    """The live values of a wave step are true values -- inside (-low, high), the interval narrow_ok bounds for lanes x K rows --
    under offsets that span g ((K - 1)(lanes - 1) + K + 1) across the wave, reach (K - 1) g below the base and grow by g per step of
    a period.  Largest power of two from 64 on that keeps them inside int16 (narrow_ok's ceiling of 30 000, less a cell's own
    excursion of |go| + g + Q where that is the tighter one; 64 + g of room at the bottom), else 0."""
    if not hfree or vfree or go > 0 or ge >= 0:
        return 0
    g, o, Q = -ge, -go, max(Q, abs(match), abs(mismatch))
    rows = lanes * K
    low = o + rows * g + 2 * (o + g) + 2 * Q
    high = rows * Q
    if low + (K - 1) * g + g + 64 >= 32768:
        return 0
    top = min(30000, 32767 - 64 - (o + g + Q))
    best = 0
    for e in range(6, 16):
        if high + g * ((K - 1) * (lanes - 1) + K + 1 + (1 << e)) < top:
            best = 1 << e
    return best


def test_period_against_its_statement(sr):
    rng = np.random.default_rng(20261019)
    match = rng.integers(0, 40, N)
    mismatch = -rng.integers(0, 40, N)
    go = -rng.integers(0, 200, N)
    ge = -rng.integers(0, 40, N) + (rng.random(N) < 0.02)  # (some at 0 / +1: outside the domain)
    hfree = (rng.random(N) < 0.97).astype(np.int64)
    vfree = (rng.random(N) < 0.03).astype(np.int64)
    K = rng.choice([1, 4, 8, 15, 16], N)
    lanes = rng.choice([1, 8, 16, 64], N)
    Q = np.where(rng.random(N) < 0.3, rng.integers(0, 400, N), 0)
    maxm = lanes * K
    got = rules(sr, np.stack([match, mismatch, go, ge, hfree, vfree, maxm, K, lanes, Q], axis=1))[:, 1]
    want = np.array([period_stated(*[int(v) for v in r]) for r in zip(match, mismatch, go, ge, hfree, vfree, K, lanes, Q)])
    assert np.array_equal(got, want)
    assert (got > 0).sum() > N // 3 and (got == 0).sum() > N // 20 and len(np.unique(got)) >= 6  # (both outcomes, many periods)


def test_period_edges(sr):
    def one(sc, K=15, lanes=64, Q=0, maxm=None):
        return [int(v) for v in rules(sr, [sc[0], sc[1], sc[2], sc[3], 1, 0, maxm or lanes * K, K, lanes, Q])[0]]
    # the benchmark's scoring at 960 rows: thousands of steps between two re-bases
    assert one((3, -5, -10, -4)) == [1, 4096]
    assert one((3, -5, -10, -4), K=16) == [1, 4096]
    # |ge| where 64 just fits and just does not (960 rows: 25 200 - 962 g > 0 ... the floor decides first: low + 15 g + 64 < 32768)
    g = 1
    while one((3, -5, -10, -(g + 1)))[1]:
        g += 1
    assert one((3, -5, -10, -g))[1] >= 64 and one((3, -5, -10, -(g + 1)))[1] == 0
    assert period_stated(3, -5, -10, -g, 1, 0, 15, 64, 0) == one((3, -5, -10, -g))[1]
    # Q raised by what a launch reported: the period shrinks, then there is none
    # (960 Q + 4 (898 + period) < 30 000: Q = 20 leaves 1 024, Q = 27 leaves 64, Q = 30 nothing -- while narrow_ok still holds: 960 Q < 30 000)
    assert one((3, -5, -10, -4), Q=20) == [1, 1024] and one((3, -5, -10, -4), Q=27) == [1, 64] and one((3, -5, -10, -4), Q=30) == [1, 0]
    # strips of one row; 1 024 rows
    assert one((3, -5, -10, -4), K=1, lanes=1)[1] == 4096
    assert one((3, -5, -10, -4), K=16, lanes=64, maxm=1024) == [1, 4096]
    # the prefix shapes: sixteen lanes of eight rows, eight of sixteen
    assert one((3, -5, -10, -4), K=8, lanes=16)[1] == 4096 and one((3, -5, -10, -4), K=16, lanes=8)[1] == 4096
    # outside the domain
    assert rules(sr, [3, -5, -10, -4, 0, 0, 960, 15, 64, 0])[0, 1] == 0 and rules(sr, [3, -5, -10, 0, 1, 0, 960, 15, 64, 0])[0, 1] == 0
