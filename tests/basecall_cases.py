"""Inputs and expected outputs of the device basecalling tests (test_emu_basecall.py on the host wave, test_gpu_basecall.py through the C
ABI): synthetic chromatograms, crafted corner cases, the traces the device must defer, and the host / reference chain they are held to."""
import ctypes as C

import numpy as np

import pyoracle as orc
from sage_oracle import find_best_trace_section, trim_trace as oracle_trim_trace
from tracy_amd import hostlib

SIGRATIOS = (0.33, 0.1, 0.5, 0.9)


def synthetic(count=200, seed0=1000):
    """`count` traces of hostlib.synth_decompose: all four kinds, 120 .. 1100 bases; (name, signal int32 [4][ns], positions)"""
    out = []
    for i in range(count):
        mf = 120 + (i * 4903) % 981
        _, sig, pos, _ = hostlib.synth_decompose(seed0 + i, mf + 400, mf, 30, i % 4, 0.6 if i % 3 else 0.5)
        out.append(("synth%d" % (seed0 + i), sig, pos))
    return out


def _base(seed=77, mf=200):
    _, sig, pos, _ = hostlib.synth_decompose(seed, mf + 400, mf, 30, 0, 0.6)
    return sig.copy(), pos.copy()


def crafted():
    """(name, signal, positions) of the corner cases; every one is inside what the device answers"""
    cases = []
    sig, pos = _base()
    p = pos.copy()
    p[51] = p[52] = p[50]  # three equal positions: windows 51 and 52 are empty, bc_len = npos - 2
    cases.append(("equal_positions", sig, p))
    p = pos.copy()
    p[10:14] = p[10]
    p[150:153] = p[152]
    cases.append(("equal_positions_twice", sig, p))

    s = sig.copy()  # no local maximum in three windows: a ramp, a constant, a falling edge -> the midpoint is called
    a, b = int(pos[79]), int(pos[82])
    s[:, a:b] = np.arange(b - a, dtype=np.int32)[None, :] * np.array([[3], [1], [2], [0]], np.int32) + 5
    a, b = int(pos[99]), int(pos[101])
    s[:, a:b] = np.array([[400], [20], [30], [10]], np.int32)
    a, b = int(pos[119]), int(pos[121])
    s[:, a:b] = (np.arange(b - a, 0, -1, dtype=np.int32) * 7)[None, :]
    cases.append(("no_peak_windows", s, pos))

    s = sig.copy()  # all four channels carry the same peak: N
    for i in (40, 41, 90):
        a, b = int(pos[i]) - 5, int(pos[i]) + 6
        s[:, a:b] = s[:, a:b].max(axis=0)[None, :]
    cases.append(("four_channels", s, pos))

    s = sig.copy()  # exact ties of the ratios: two and three channels with the same peak (the last one wins), and a tie at sigratio itself
    for i, chans in ((30, (0, 2)), (31, (1, 3)), (60, (0, 1, 3)), (61, (2, 3))):
        a, b = int(pos[i]) - 5, int(pos[i]) + 6
        top = s[:, a:b].max(axis=0)
        for k in chans:
            s[k, a:b] = top
    a, b = int(pos[140]) - 5, int(pos[140]) + 6
    s[:, a:b] = 0
    s[0, int(pos[140])] = 1000
    s[3, int(pos[140]) + 1] = 500  # ratio 0.5 exactly: heterozygous at sigratio 0.5
    s[1, int(pos[140]) - 1] = 330
    cases.append(("ratio_ties", s, pos))

    cases.append(("all_zero", np.zeros_like(sig), pos))  # top = 1, every ratio 0
    flat = np.zeros((4, 400), np.int32)
    cases.append(("all_zero_regular", flat, np.arange(6, 390, 12, dtype=np.int32)))  # equal spacing: every penalty 0, qualities from NaN

    for n in (1, 2, 4, 5, 9, 10, 11, 12):  # the wrapped loops of findBestTraceSection
        cases.append(("short%d" % n, sig[:, :int(pos[n]) + 1].copy(), pos[:n].copy()))

    ns = int(pos[-1]) + 1  # the last position is the last sample
    cases.append(("last_sample", sig[:, :ns].copy(), pos))
    cases.append(("first_sample", sig, np.concatenate([np.zeros(1, np.int32), pos])))

    m = int(np.abs(sig).max())  # values at the ends of int16
    s = (sig.astype(np.int64) * 32767 // max(m, 1)).astype(np.int32)
    s[1, 500:520] = -32768
    s[2, 900:905] = 32767
    s[3, 1200:1260] -= 300
    cases.append(("int16_range", np.clip(s, -32768, 32767), pos))

    rng = np.random.default_rng(5)  # noise: irregular peaks, plateaus (small integers repeat), negative values
    s = rng.integers(-3, 40, size=(4, 3000)).astype(np.int32)
    p = np.sort(rng.choice(np.arange(3, 2990), size=260, replace=False)).astype(np.int32)
    cases.append(("noise", s, p))
    p = np.sort(rng.integers(0, 3000, size=700)).astype(np.int32)  # many repeated and adjacent positions
    cases.append(("noise_dense", s, p))
    p = np.array([5, 900, 905, 906, 2600, 2999], np.int32)  # windows wider than one LDS tile
    cases.append(("wide_windows", s, p))
    return cases


def deferred():
    """(name, signal, positions) the device must hand back: status DEFERRED, bc_len 0"""
    sig, pos = _base()
    out = []
    p = pos.copy(); p[100] = p[99] - 1
    out.append(("decreasing", sig, p))
    p = pos.copy(); p[-1] = sig.shape[1]
    out.append(("beyond_samples", sig, p))
    p = pos.copy(); p[0] = -1
    out.append(("negative", sig, p))
    out.append(("no_positions", sig, pos[:0].copy()))
    out.append(("two_samples", sig[:, :2].copy(), np.array([0, 1], np.int32)))
    return out


def ref_basecall_qual(sig, pos, sigratio):
    """the reference's own basecall() + estimateQualities() (oracle/_ref), None where that library was never built"""
    ref = orc.ref_lib()
    if ref is None:
        return None
    sig = np.ascontiguousarray(sig, dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    n = len(pos)
    pri, sec, con = (C.create_string_buffer(n + 1) for _ in range(3))
    bc = np.zeros(max(n, 1), np.int32)
    q = np.zeros(max(n, 1), np.uint8)
    fn = ref.ref_basecall_qual
    fn.restype = C.c_size_t
    k = fn(sig.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(sig.shape[1]), pos.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(n),
           C.c_float(sigratio), pri, sec, con, bc.ctypes.data_as(C.POINTER(C.c_int32)), q.ctypes.data_as(C.POINTER(C.c_uint8)))
    return pri.raw[:k], sec.raw[:k], con.raw[:k], bc[:k].copy(), q[:k].copy()


def expected(sig, pos, sigratio, stringencies=()):
    """every output field of the host chain; the reference and the Python restatements are checked against it on the way"""
    pri, sec, con, bcpos, qual = hostlib.basecall_qual(sig, pos, sigratio)
    ref = ref_basecall_qual(sig, pos, sigratio)
    if ref is not None:
        assert ref[:3] == (pri, sec, con) and np.array_equal(ref[3], bcpos) and np.array_equal(ref[4], qual)
    n = len(pri)
    prof = hostlib.create_profile(sig, bcpos, pri, sec) if n else np.zeros((6, 0), np.float32)
    peaks = np.ascontiguousarray(sig[:, bcpos].T, dtype=np.int32) if n else np.zeros((0, 4), np.int32)
    best = find_best_trace_section(sec, [int(x) for x in bcpos])[1]
    trims = {}
    for s in stringencies:
        l, r = hostlib.trim_trace(sig, pos, sigratio, float(s))
        assert (l, r) == tuple(oracle_trim_trace(float(s), sec, [int(x) for x in bcpos])), s
        trims[s] = (l & 0xFFFF, r & 0xFFFF)
    return dict(primary=pri, secondary=sec, consensus=con, bcpos=bcpos, estqual=qual, profile=prof, peaks=peaks, best_section=best,
                trims=trims, bc_len=n)


def compare(got, want, stringency, where):
    """exact equality of every field (profile: float bits)"""
    assert got["status"] == 0, where
    assert got["bc_len"] == want["bc_len"], where
    for k in ("primary", "secondary", "consensus"):
        assert bytes(got[k]) == want[k], (where, k)
    for k in ("bcpos", "estqual", "peaks"):
        assert np.array_equal(np.asarray(got[k]), want[k]), (where, k)
    assert np.array_equal(np.asarray(got["profile"], dtype=np.float32).view(np.uint32), want["profile"].view(np.uint32)), (where, "profile")
    assert got["best_section"] == want["best_section"], (where, "best_section")
    if stringency:
        assert (got["trim_left"], got["trim_right"]) == want["trims"][stringency], (where, "trims", stringency)
    else:
        assert (got["trim_left"], got["trim_right"]) == (0, 0), where
