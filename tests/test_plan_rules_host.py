"""The per-trace planning rules both pipelines call (tracy_amd/csrc/stream_plan.h: the host-planned tiers of pipeline.hip and the
planning kernels of stream.hip), built for the host with their own small g++ step and checked against a direct statement of the
arithmetic in their comments: on 10^5 seeded random inputs per rule and on the edges (g at 2^20, no loss, a clamped to 0, empty
pairs, the LDS limit, the final band's clamps, W at its cap, the trim's left edge and negative reverse offset, the vote's ties and
thresholds, a strand's bound equal to the other's score and at INT32_MAX)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "plan_rules.cpp")
N = 100_000


@pytest.fixture(scope="module")
def pr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("plan") / "plan_rules.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-o", so, SRC],
                   check=True, timeout=300)
    return C.CDLL(so)


def call(pr, name, cols, nout):
    """rows of int64 arguments -> rows of int64 results"""
    x = np.ascontiguousarray(np.stack([np.asarray(c, np.int64) for c in cols], axis=1))
    out = np.zeros((x.shape[0], nout), np.int64)
    getattr(pr, name)(C.c_uint64(x.shape[0]), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def consts(pr):
    out = np.zeros(3, np.int64)
    pr.pr_consts(out.ctypes.data_as(C.c_void_p))
    return [int(v) for v in out]


def u32(x):
    return np.asarray(x, np.int64) & 0xFFFFFFFF


def i32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def tdiv(a, b):
    """C integer division (toward zero)"""
    a = np.asarray(a, np.int64)
    return np.sign(a) * (np.abs(a) // b)


def pick_k(dlo, dhi):
    """smallest strip height K of 4 / 8 / 12 whose K + width steps fit fifteen blocks of K + 1; 0: too wide"""
    w = np.asarray(dhi, np.int64) - np.asarray(dlo, np.int64)
    k = np.where(4 + w <= 75, 4, np.where(8 + w <= 135, 8, np.where(12 + w <= 195, 12, 0)))
    return np.where(w < 0, 0, k)


def fits_lds(n, k):
    """the codes of four pairs (n + 7 rounded down to 4 bytes each) + 6 codes x K rows x 64 lanes of int16 within 60 KiB"""
    n = np.asarray(n, np.int64)
    return 4 * ((n + 7) & ~3) + 6 * np.asarray(k, np.int64) * 64 * 2 <= 60 * 1024


def end_band(m, ce, g):
    gg = np.minimum(g, 1 << 20)
    d1 = np.asarray(ce, np.int64) - m
    dlo, dhi = d1 - gg - 1, d1 + gg + 1
    return dlo, dhi, pick_k(dlo, dhi)


def check(got, *want):
    for j, w in enumerate(want):
        w = np.broadcast_to(np.asarray(w, np.int64), got[:, j].shape)
        bad = np.nonzero(got[:, j] != w)[0]
        assert bad.size == 0, (j, bad[:5], got[bad[:5]], w[bad[:5]])


# ---- R9: trimReferenceSlice's last step ----

def trim_ref(ri, risize, n, tl, tr, fwd):
    ri, risize, n = u32(ri), u32(risize), u32(n)
    left = ri >= tl
    ri, risize = np.where(left, u32(ri - tl), ri), np.where(left, u32(risize + tl), risize)
    risize = np.where(u32(ri + risize + tr) < n, u32(risize + tr), risize)
    length = np.where(ri <= n, np.minimum(risize, u32(n - ri)), 0)
    offset = i32(i32(i32(n) - i32(ri)) - i32(risize))
    pos = np.where(fwd != 0, ri, np.where(offset >= 0, offset, 0))
    return ri, length, pos, 0


def test_trim_finish(pr):
    rng = np.random.default_rng(9)
    n = rng.integers(0, 5000, N)
    ri = rng.integers(0, 5200, N)
    risize = rng.integers(0, 5200, N)
    tl, tr, fwd = rng.integers(0, 120, N), rng.integers(0, 120, N), rng.integers(0, 2, N)
    edges = np.array([
        # ri risize n tl tr fwd
        [10, 100, 1000, 50, 50, 1],    # ri < trim_left: no widening on the left
        [10, 100, 1000, 50, 50, 0],
        [50, 100, 1000, 50, 50, 0],    # ri == trim_left
        [900, 200, 1000, 50, 50, 0],   # negative reverse offset: pos stays 0
        [900, 200, 1000, 50, 50, 1],
        [1200, 10, 1000, 0, 0, 1],     # ri past the end: empty slice
        [0, 0, 0, 0, 0, 0],
        [0xFFFFFFF0, 0x20, 100, 0, 0, 0],  # the unsigned wrap of ri + risize + trim_right
    ])
    cols = [np.concatenate([c, edges[:, j]]) for j, c in enumerate((ri, risize, n, tl, tr, fwd))]
    got = call(pr, "pr_trim_finish", cols, 4)
    check(got, *trim_ref(*cols))
    assert got[N + 3, 2] == 0 and got[N + 4, 2] == 850


# ---- R2 / R1: eligibility of the pruned sweep, class from the votes ----

def test_front_ok(pr):
    R, K, HW = consts(pr)
    assert (K, HW) == (12, 90)
    rng = np.random.default_rng(2)
    m = np.concatenate([rng.integers(0, 3000, N), [0, R, R + 2 * K, R + 2 * K + 1, 20000, 40000]])
    n = np.concatenate([rng.integers(0, 3000, N), [5, 5, 5, 0, 5, 5]])
    sc = np.array([[3, -5, -10, -4, 1, 0], [1, -1, -2, -1, 1, 0], [3, -5, -10, -4, 0, 0], [3, -5, -10, -4, 1, 1], [3, -5, 1, -4, 1, 0]])
    for row in sc:
        cols = [np.full(m.size, v) for v in row] + [m, n]
        got = call(pr, "pr_front_ok", cols, 3)
        check(got[:, :1], np.where((row[4] != 0) & (row[5] == 0), got[:, 1], 0))  # origin16_ok: b16_origin_ok in AlignConfig<true,false>
        want_cols = [np.full(m.size, v) for v in row] + [m, m - R + 2 * HW + 16]
        origin = call(pr, "pr_front_ok", want_cols, 3)[:, 0]
        check(got[:, 2:], (m > R + 2 * K) & (n >= 1) & (origin != 0))
    # the host wrote `m - R > 2 kFrontK` under `m > R` (unsigned), the device `m > R + 2 kFrontK`: the same for every m
    mm = np.concatenate([np.arange(0, 1 << 16), (1 << 32) - np.arange(1, 1 << 10)]).astype(np.int64)
    assert np.array_equal((mm > R) & (u32(mm - R) > 2 * K), mm > R + 2 * K)


def test_orient_class(pr):
    R = consts(pr)[0]
    rng = np.random.default_rng(1)
    vf, vr = rng.integers(0, 200, N), rng.integers(0, 200, N)
    vr[: N // 4] = vf[: N // 4] // 2  # at and around the 2:1 majority
    vr[N // 4: N // 3] = vf[N // 4: N // 3]
    m = rng.integers(R - 3, R + 4000, N)
    m[:100] = R
    fok, exact = rng.integers(0, 2, N), rng.integers(0, 2, N)
    edges = np.array([[32, 16, R + 1, 1, 0], [31, 15, R + 1, 1, 0], [32, 17, R + 1, 1, 0], [16, 32, R + 1, 1, 0], [32, 16, R, 1, 0],
                      [0, 0, R + 500, 1, 1], [64, 0, R + 500, 0, 1], [64, 0, R + 500, 0, 0]])
    cols = [np.concatenate([c, edges[:, j]]) for j, c in enumerate((vf, vr, m, fok, exact))]
    vf, vr, m, fok, exact = cols
    got = call(pr, "pr_orient_class", cols, 3)
    g = np.where(vf >= vr, 0, 1)
    hi, lo = np.maximum(vf, vr), np.minimum(vf, vr)
    both = np.where((m > R) & (hi >= 32) & (hi >= 2 * lo), 0, 1)
    cls = np.where((both == 0) & (fok != 0), 0, np.where((exact != 0) | (both != 0), 1, 2))
    check(got, g, both, cls)
    assert list(got[N:, 2]) == [0, 1, 1, 0, 1, 1, 1, 2]


# ---- R10 / R11: the clear vote, strand by certificate ----

def test_clear_vote(pr):
    """every (vf, vr) of a grid that holds the ties hi == 32, hi == 2 lo and vf == vr, for both strands a sweep can ask about"""
    v = np.concatenate([np.arange(0, 140), [255, 256, 1000, 2000, 2001, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]])
    vf, vr, orient = (a.ravel() for a in np.meshgrid(v, v, [0, 1], indexing="ij"))
    got = call(pr, "pr_clear_vote", [vf, vr, orient], 3)
    g = np.where(vf >= vr, 0, 1)  # a tie votes forward
    hi, lo = np.maximum(vf, vr), np.minimum(vf, vr)
    clear = (hi >= 32) & (hi >= u32(2 * lo))  # (32-bit unsigned arithmetic, as the kernels')
    check(got, g, clear, clear & (orient != g))
    at = {(int(a), int(b)): i for i, (a, b, o) in enumerate(zip(vf, vr, orient)) if o == 0}
    for (a, b), want in {(32, 16): (0, 1), (16, 32): (1, 1), (31, 0): (0, 0), (32, 17): (0, 0), (64, 32): (0, 1), (64, 33): (0, 0),
                         (40, 40): (0, 0), (0, 0): (0, 0), (33, 16): (0, 1), (32, 0): (0, 1), (0, 32): (1, 1)}.items():
        assert tuple(got[at[(a, b)], :2]) == want, (a, b)


def test_strand_by_bound(pr):
    """voted forward: bound < S_g; voted reverse: bound <= S_g (gsFwd > gsRev, sage.h:247: the tie goes to reverse); the stored
    bound is min(prefix + ub, INT32_MAX).  Around bound == S_g for both g, with negative scores, and at the clamp."""
    rng = np.random.default_rng(12)
    big = (1 << 31) - 1
    pre = np.concatenate([rng.integers(-4000, 4000, N), [-1000000, -1, 0, 1, big - 1, big, big, big, -(1 << 31)]])
    ub = np.concatenate([rng.integers(0, 3000, N), [0, 0, 0, 0, 1, 0, 1, big, big]])
    n = pre.size
    cols, want_c, want_b = [], [], []
    for g in (0, 1):
        for delta in (-2, -1, 0, 1, 2):  # S_g - bound
            s_g = pre + ub + delta
            cols.append([np.full(n, g), pre, ub, s_g])
            want_c.append(np.full(n, delta > 0 if g == 0 else delta >= 0))
            want_b.append(np.minimum(pre + ub, big))
    cols = [np.concatenate([c[j] for c in cols]) for j in range(4)]
    got = call(pr, "pr_strand_by_bound", cols, 2)
    check(got, np.concatenate(want_c), np.concatenate(want_b))
    one = lambda *row: list(call(pr, "pr_strand_by_bound", [[x] for x in row], 2)[0])
    assert one(0, -50, 10, -40) == [0, -40] and one(1, -50, 10, -40) == [1, -40]  # the tie, negative scores
    assert one(0, -50, 10, -39) == [1, -40] and one(1, -50, 10, -41) == [0, -40]
    assert one(0, big, 5, 1 << 40) == [1, big] and one(1, big, 1, big) == [0, big]  # the stored bound is clamped, the comparison is not
    assert one(1, big, 0, big) == [1, big]


# ---- R3 / R4: sub-window and band from a score; LDS fit ----

def test_sub_window(pr):
    rng = np.random.default_rng(3)
    m = rng.integers(1, 3000, N)
    ce = rng.integers(1, 5000, N)
    ge = -rng.integers(1, 10, N)
    top = rng.integers(0, 20000, N)
    sstar = top - rng.integers(-50, 1200, N)  # loss <= 0 for some
    edges = []
    for g in ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 24):
        edges.append([1000, 3000, g * 3 + 10, 10, -3])                  # g at and above 2^20
    edges += [[1000, 1200, 5000, 5000, -4], [1000, 1200, 5000, 6000, -4],  # loss 0, loss < 0
              [1000, 900, 100, 0, -1], [1, 1, 0, 0, -1], [100, 5000, 1000, 0, -2]]  # a clamped to 0; a > 0
    edges = np.array(edges)
    cols = [np.concatenate([c, edges[:, j]]) for j, c in enumerate((m, ce, top, sstar, ge))]
    m, ce, top, sstar, ge = cols
    got = call(pr, "pr_sub_window", cols, 6)
    loss = top - sstar
    g = np.where(loss > 0, loss // -ge, 0)
    a = np.maximum(ce - m - g - 2, 0)
    nn = ce - a
    dlo, dhi, k = end_band(m, nn, g)
    check(got, g, a, nn, dlo, dhi, k)
    assert got[N + 1, 0] == 1 << 20 and got[N + 1, 5] == 0 and got[N + 2, 5] == 0
    assert got[N + 6, 1] == 0 and got[N + 8, 1] > 0


def test_end_band(pr):
    rng = np.random.default_rng(4)
    m, ce = rng.integers(0, 3000, N), rng.integers(0, 3000, N)
    g = rng.integers(0, 120, N)
    g[:100] = rng.integers((1 << 20) - 2, (1 << 20) + 3, 100)
    got = call(pr, "pr_end_band", [m, ce, g], 3)
    check(got, *end_band(m, ce, g))


def test_fits_lds(pr):
    rng = np.random.default_rng(5)
    n = rng.integers(0, 20000, N)
    k = rng.choice([4, 8, 12], N)
    edge_n, edge_k = [], []
    for K in (4, 8, 12):
        last = max(x for x in range(20000) if 4 * ((x + 7) & ~3) + 768 * K <= 60 * 1024)
        assert 4 * ((last + 7) & ~3) + 768 * K == 60 * 1024  # exactly at the limit ...
        edge_n += [last, last + 1]  # ... and one past it
        edge_k += [K, K]
    n, k = np.concatenate([n, edge_n]), np.concatenate([k, edge_k])
    got = call(pr, "pr_fits_lds", [n, k], 1)
    check(got, fits_lds(n, k))
    assert list(got[N:, 0]) == [1, 0, 1, 0, 1, 0]


# ---- R5 / R6: the final alignment's band and certificate ----

def final_band_ref(m, n, want):
    over = n - m
    aover = np.abs(over)
    fit = tdiv(195 - 12 - aover, 2)
    w = np.where((want > fit) & (fit >= 24), fit, want)
    dlo, dhi = -w - np.maximum(-over, 0), w + np.maximum(over, 0)
    k = pick_k(dlo, dhi)
    ok = (m != 0) & (n != 0) & fits_lds(n, 12)
    return np.where(ok, w, 0), np.where(ok, dlo, 0), np.where(ok, dhi, 0), np.where(ok, k, 0)


def test_final_width(pr):
    gap = np.concatenate([np.random.default_rng(6).integers(0, 200, N), [0, 47, 48, 49, 0x7FFFFFFF]])
    got = call(pr, "pr_final_width", [gap], 1)
    check(got, np.clip(gap + 48, 32, 96))
    assert list(got[N:, 0]) == [48, 95, 96, 96, 96]


def test_final_band(pr):
    rng = np.random.default_rng(7)
    m = rng.integers(0, 3000, N)
    n = m + rng.integers(-200, 200, N)
    n[: N // 10] = rng.integers(12000, 14000, N // 10)  # around the LDS limit of K = 12
    n = np.maximum(n, 0)
    want = np.where(rng.random(N) < 0.8, np.clip(rng.integers(0, 200, N) + 48, 32, 96), rng.integers(0, 4097, N))
    lim = max(x for x in range(20000) if fits_lds(x, 12))
    edges = np.array([
        [0, 100, 96], [100, 0, 96],                      # m or n = 0
        [1000, 1135, 96], [1000, 1134, 96],              # fit = 24: narrowed to 24
        [1000, 1136, 96], [1000, 1137, 96],              # fit = 23 (just under 24): not narrowed, too wide
        [1135, 1000, 96],                                # ... on the other side
        [lim, lim, 48], [lim + 1, lim + 1, 48],          # the LDS limit of the K = 12 tables
        [1000, 1000, 32], [1000, 1000, 96], [1000, 1000, 200],
    ])
    cols = [np.concatenate([c, edges[:, j]]) for j, c in enumerate((m, n, want))]
    got = call(pr, "pr_final_band", cols, 4)
    check(got, *final_band_ref(*cols))
    e = got[N:]
    assert e[0, 3] == 0 and e[1, 3] == 0
    assert e[2, 0] == 24 and e[2, 3] == 12 and e[3, 0] == 24
    assert e[4, 0] == 96 and e[4, 3] == 0 and e[6, 0] == 24
    assert e[7, 3] != 0 and e[8, 3] == 0
    assert e[11, 0] == 91 and e[11, 3] == 12


def test_final_certified(pr):
    rng = np.random.default_rng(8)
    top = rng.integers(-1000, 5000, N)
    ge = -rng.integers(1, 10, N)
    w = rng.integers(24, 97, N)
    lose = -ge * (w + 1)
    sb = top - lose + rng.integers(-3, 4, N)  # at, just above and just below the bound
    ops = np.where(rng.random(N) < 0.1, 0, rng.integers(1, 5000, N))
    got = call(pr, "pr_final_certified", [sb, top, ge, w, ops], 1)
    check(got, (sb > top - lose) & (ops != 0))


# ---- R7: allele vs trimmed slice ----

def slice_band_ref(m, n, ce, g, narrow, lead, ri):
    ok = (g >= 0) & (m != 0) & (n != 0) & (ce >= 1) & (ce <= n)
    dlo, dhi, _ = end_band(m, ce, g)
    gg = np.minimum(g, 1 << 20)
    d1 = ce - m
    d0 = lead - ri
    delta = np.abs(d1 - d0)
    nar = (narrow != 0) & (lead >= ri) & (delta <= gg)
    s = (gg - delta) // 2
    dlo = np.where(nar, np.minimum(d0, d1) - s - 1, dlo)
    dhi = np.where(nar, np.maximum(d0, d1) + s + 1, dhi)
    k = pick_k(dlo, dhi)
    return np.where(ok, dlo, 0), np.where(ok, dhi, 0), np.where(ok, k, 0)


def test_slice_band(pr):
    rng = np.random.default_rng(10)
    m = rng.integers(0, 2000, N)
    n = np.maximum(m + rng.integers(-50, 150, N), 0)
    ce = n - rng.integers(-3, 60, N)
    g = rng.integers(-1, 110, N)
    narrow = rng.integers(0, 2, N)
    ri = rng.integers(0, 300, N)
    lead = ri + rng.integers(-20, 120, N)
    lead = np.maximum(lead, 0)
    edges = np.array([[500, 600, 550, 40, 1, 5, 10],          # lead < ri: not narrowed
                      [500, 600, 550, 40, 1, 60, 10],         # narrowed: d0 = 50 = d1
                      [500, 600, 550, 40, 0, 60, 10],         # the host's: not narrowed
                      [500, 600, 550, 40, 1, 200, 10],        # |d1 - d0| > g: not narrowed
                      [0, 600, 550, 40, 1, 60, 10], [500, 0, 550, 40, 1, 60, 10], [500, 600, 0, 40, 1, 60, 10],
                      [500, 600, 601, 40, 1, 60, 10], [500, 600, 550, -1, 1, 60, 10],
                      [500, 600, 550, 1 << 20, 1, 60, 10], [500, 600, 550, (1 << 20) + 5, 0, 60, 10]])
    cols = [np.concatenate([c, edges[:, j]]) for j, c in enumerate((m, n, ce, g, narrow, lead, ri))]
    got = call(pr, "pr_slice_band", cols, 3)
    check(got, *slice_band_ref(*cols))
    e = got[N:]
    assert list(e[0]) == [9, 91, 8] and list(e[1]) == [29, 71, 4] and list(e[2]) == [9, 91, 8] and list(e[3]) == [9, 91, 8]
    assert all(e[i, 2] == 0 for i in range(4, 11))


# ---- R8: allele 1 vs allele 2 ----

def a12_band_ref(ln, best, go, ge, sc1, sc2):
    """W, bound of s_a12_band for alleles of ln > 0 bases (also what test_gpu_decompose.py expects of the band's certificate)"""
    lost = np.maximum(best * ln - sc1, 0) + np.maximum(best * ln - sc2, 0)
    per = best - 2 * ge
    W = np.minimum((5 * lost // 2 + 40) // np.where(per > 0, per, 1) + 2, 90)
    return W, best * (ln - (W + 1)) + ge * 2 * (W + 1) + 2 * go


def test_a12_band(pr):
    rng = np.random.default_rng(11)
    ln = rng.integers(0, 3000, N)
    best = rng.integers(0, 6, N)
    go, ge = -rng.integers(0, 15, N), -rng.integers(1, 8, N)
    sc1 = best * ln - rng.integers(-20, 400, N)
    sc2 = best * ln - rng.integers(-20, 400, N)
    sc2[:100] = -1_000_000  # W at its cap of 90
    edges = np.array([[0, 1, -10, -4, 0, 0], [1000, 1, -10, -4, -1_000_000, 0], [1000, 1, -10, -4, 1000, 1000], [1000, 0, 0, -1, 0, 0]])
    cols = [np.concatenate([c, edges[:, j]]) for j, c in enumerate((ln, best, go, ge, sc1, sc2))]
    ln, best, go, ge, sc1, sc2 = cols
    got = call(pr, "pr_a12_band", cols, 4)
    W, bound = a12_band_ref(ln, best, go, ge, sc1, sc2)
    z = ln == 0
    check(got, np.where(z, 0, -W), np.where(z, 0, W), np.where(z, 0, pick_k(-W, W)), np.where(z, 0, bound))
    e = got[N:]
    assert list(e[0]) == [0, 0, 0, 0]
    assert list(e[1][:3]) == [-90, 90, 12] and e[1, 3] == 1000 - 91 - 4 * 2 * 91 - 20
    assert list(e[2][:3]) == [-6, 6, 4]  # nothing lost: W = 40 // (1 + 2 * 4) + 2


# ---- R12 / R13: the certificates of the bands whose score is known beforehand / bounded (both also need a walk that stayed inside) ----

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def test_exact_certified(pr):
    """sb == S* and ops_len != 0: every S* of a grid with negative scores and the ends of the int32 range, the banded score at it and
    at both neighbours (where they are int32 values), and INT32_MIN / INT32_MAX as banded scores against every S*"""
    rng = np.random.default_rng(13)
    sstar = np.concatenate([rng.integers(-5000, 5000, 1000), [-1, 0, 1, -300, I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX]])
    cols = []
    for delta in (-1, 0, 1):
        sb = sstar + delta
        keep = (sb >= I32_MIN) & (sb <= I32_MAX)
        cols.append((sb[keep], sstar[keep]))
    for edge in (I32_MIN, I32_MAX):
        cols.append((np.full(sstar.size, edge), sstar))
    sb, sstar = (np.concatenate([c[j] for c in cols]) for j in range(2))
    for ops in (0, 1, 4000):
        got = call(pr, "pr_exact_certified", [sb, sstar, np.full(sb.size, ops)], 1)
        check(got, (sb == sstar) & (ops != 0))
    one = lambda *row: int(call(pr, "pr_exact_certified", [[x] for x in row], 1)[0, 0])
    assert one(-40, -40, 1) == 1 and one(-40, -40, 0) == 0 and one(-41, -40, 1) == 0 and one(-39, -40, 1) == 0
    assert one(I32_MIN, I32_MIN, 1) == 1 and one(I32_MAX, I32_MAX, 1) == 1 and one(I32_MIN, I32_MAX, 1) == 0 and one(I32_MAX, I32_MIN, 1) == 0


def test_a12_certified(pr):
    """sb > bound and ops_len != 0 (the bound is 64-bit: the comparison must not narrow it): the banded score at the bound and at both
    neighbours, negative scores, INT32_MIN / INT32_MAX as banded scores, bounds just outside and far outside the int32 range"""
    rng = np.random.default_rng(14)
    bound = np.concatenate([rng.integers(-5000, 5000, 1000), [-61, -1, 0, 1, I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX]])
    cols = []
    for delta in (-1, 0, 1):
        sb = bound + delta
        keep = (sb >= I32_MIN) & (sb <= I32_MAX)
        cols.append((sb[keep], bound[keep]))
    wide = np.array([I32_MIN - 1, I32_MIN - (1 << 32), -(1 << 62), I32_MAX + 1, I32_MAX + (1 << 32), 1 << 62,
                     (1 << 32) - 5, -(1 << 32) + 5])  # (the last two: what a 32-bit comparison would read as -5 / 5)
    for edge in (I32_MIN, -108, -5, 0, 5, I32_MAX):
        cols.append((np.full(bound.size, edge), bound))
        cols.append((np.full(wide.size, edge), wide))
    sb, bound = (np.concatenate([c[j] for c in cols]) for j in range(2))
    for ops in (0, 1, 4000):
        got = call(pr, "pr_a12_certified", [sb, bound, np.full(sb.size, ops)], 1)
        check(got, (sb > bound) & (ops != 0))
    one = lambda *row: int(call(pr, "pr_a12_certified", [[x] for x in row], 1)[0, 0])
    assert one(-60, -61, 1) == 1 and one(-61, -61, 1) == 0 and one(-62, -61, 1) == 0 and one(-60, -61, 0) == 0
    assert one(I32_MIN, I32_MIN - 1, 1) == 1 and one(I32_MAX, I32_MAX + 1, 1) == 0 and one(I32_MAX, I32_MAX, 1) == 0
    assert one(0, (1 << 32) - 5, 1) == 0 and one(0, -(1 << 32) + 5, 1) == 1
