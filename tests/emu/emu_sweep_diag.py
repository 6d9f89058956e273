"""ctypes driver of emu_sweep_diag.cpp: the 16-bit query-profile sweep in either form on the host wave (tests only)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "libemu_sweep_diag.so")
        srcs = [os.path.join(_HERE, "emu_sweep_diag.cpp"), os.path.join(_HERE, "host_wave.h")] + \
               [os.path.join(_ROOT, "tracy_amd/csrc", f) for f in ("dp_kernels.h", "dp_lane.h", "sweep_range.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-pthread", "-ffp-contract=off",
                                   "-o", so, srcs[0]], stderr=subprocess.DEVNULL)
        _LIB = C.CDLL(so)
        _LIB.emu_diag_period.restype = C.c_uint32
    return _LIB


def sweep(a1, ref, score, K, period=0, ckpt=False, B=64, revcomp=False):
    """a1: float32 [6][m] profile or bytes (strings); ref: bytes.  Returns (score, err flags, row m, checkpoint records):
    row m as uint32 [n + 1] (column c at index c: E' in the high half, H in the low one), the records as int32 [nrec][K + 1][64]."""
    strings = isinstance(a1, (bytes, bytearray))
    if strings:
        b1 = np.frombuffer(bytes(a1) + b"\0", dtype=np.uint8).copy()
        m = stride = len(a1)
    else:
        b1 = np.ascontiguousarray(a1, dtype=np.float32)
        m = stride = b1.shape[1]
    b2 = np.frombuffer(bytes(ref) + b"\0", dtype=np.uint8).copy()
    n = len(ref)
    nrec = (n + 64) // B + 2
    lastrow = np.full(n + 2, 0x7f7f7f7f, np.int32)
    rec = np.full((nrec, K + 1, 64), 0x7f7f7f7f, np.int32)
    sc = C.c_int32(0)
    err = (C.c_int32 * 2)()
    rc = lib().emu_sweep(K, int(strings), C.c_uint32(period), int(ckpt), C.c_uint32(B), C.c_void_p(b1.ctypes.data), m, stride,
                         C.c_void_p(b2.ctypes.data), n, int(revcomp), *[int(x) for x in score], C.byref(sc),
                         C.c_void_p(lastrow.ctypes.data), C.c_void_p(rec.ctypes.data), C.c_uint32(nrec), err)
    assert rc == 0, rc
    return sc.value, (err[0], err[1]), lastrow.view(np.uint32), rec


def narrow_ok(score, maxm, K, Q=0):
    return bool(lib().emu_narrow_ok(*[int(x) for x in score], C.c_uint32(maxm), K, C.c_int64(Q)))


def diag_period(score, K, lanes=64, Q=0):
    return int(lib().emu_diag_period(*[int(x) for x in score], K, lanes, C.c_int64(Q)))


def prefix(profiles, refs, score, K, GL, period=0, revcomp=None, skip=None):
    """the prefix rows of up to 64 / GL pairs on one wave.  Returns (bounds, kept rows, err): kept[i] = uint32 [n_i + 1], column c at index c."""
    npairs = len(profiles)
    assert npairs <= 64 // GL
    a1 = np.concatenate([np.ascontiguousarray(p, dtype=np.float32).ravel() for p in profiles])
    m = np.array([p.shape[1] for p in profiles], np.uint32)
    n = np.array([len(r) for r in refs], np.uint32)
    a1_off = np.concatenate([[0], np.cumsum(6 * m.astype(np.uint64))[:-1]]).astype(np.uint64)
    a2 = np.frombuffer(b"".join(bytes(r) for r in refs) + b"\0", dtype=np.uint8).copy()
    a2_off = np.concatenate([[0], np.cumsum(n.astype(np.uint64))[:-1]]).astype(np.uint64)
    kept_off = np.concatenate([[0], np.cumsum(n.astype(np.uint64) + 8)[:-1]]).astype(np.uint64)
    flags = np.array([(1 if (revcomp and revcomp[i]) else 0) | (2 if (skip and skip[i]) else 0) for i in range(npairs)], np.uint32)
    out = np.full(npairs, 0x7f7f7f7f, np.int32)
    kept = np.full(int(kept_off[-1] + n[-1] + 8), 0x7f7f7f7f, np.int32)
    err = (C.c_int32 * 2)()
    P = lambda x: C.c_void_p(x.ctypes.data)
    rc = lib().emu_prefix_diag(K, GL, C.c_uint32(period), C.c_uint32(npairs), P(a1), P(a1_off), P(m), P(a2), P(a2_off), P(n), P(flags), P(kept_off),
                               *[int(x) for x in score], P(out), P(kept), err)
    assert rc == 0, rc
    rows = [kept.view(np.uint32)[int(kept_off[i]):int(kept_off[i]) + int(n[i]) + 1].copy() for i in range(npairs)]
    return out, rows, (err[0], err[1])
