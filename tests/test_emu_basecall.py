"""basecall_wave_body (tracy_amd/csrc/basecall_wave.h: basecall + qualities + best section + trims + profile of one trace on one wave) on
the 64-fiber host wave, every output field against the reference's abif.h (oracle/_ref), the host chain (hostlib) and the restatements of
tests/sage_oracle.py -- exact equality, profile floats bit for bit.  Plus the argument checks of tracyhip_basecall_traces, which need no
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import basecall_cases as bcs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_basecall.so")
    srcs = [os.path.join(HERE, "emu", "emu_basecall.cpp"), os.path.join(HERE, "emu", "host_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/basecall_wave.h"), os.path.join(ROOT, "tracy_amd/csrc/dp_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]],
                              stderr=subprocess.DEVNULL)
    return C.CDLL(so)


def run(emu, sig, pos, sigratio=0.33, stringency=0, int16=False):
    sig = np.ascontiguousarray(sig, dtype=np.int16 if int16 else np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    n = len(pos)
    cap = max(n, 1)
    pri, sec, con, q = (np.full(cap, 0x7e, np.uint8) for _ in range(4))
    bcpos = np.full(cap, -7, np.int32)
    peaks = np.full(4 * cap, -7, np.int32)
    prof = np.full(6 * cap, -7.0, np.float32)
    out = (C.c_int32 * 5)()
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = emu.emu_basecall(p(sig), 2 if int16 else 4, C.c_uint32(sig.shape[1]), p(pos), C.c_uint32(n), C.c_float(sigratio), C.c_float(stringency),
                          p(pri), p(sec), p(con), p(bcpos), p(q), p(peaks), p(prof), out)
    assert rc == 0
    k = out[1]
    untouched = (pri[k:] == 0x7e).all() and (bcpos[k:] == -7).all() and (peaks[4 * k:] == -7).all() and (prof[6 * k:] == -7.0).all()
    return dict(status=out[0], bc_len=k, trim_left=out[2], trim_right=out[3], best_section=out[4], primary=pri[:k].tobytes(),
                secondary=sec[:k].tobytes(), consensus=con[:k].tobytes(), bcpos=bcpos[:k], estqual=q[:k], peaks=peaks[:4 * k].reshape(k, 4),
                profile=prof[:6 * k].reshape(6, k), untouched=bool(untouched))


def test_synthetic_traces_match_the_reference_chain(emu):
    het = 0
    for i, (name, sig, pos) in enumerate(bcs.synthetic()):
        strs = tuple(range(1, 10)) if i < 24 else ((i % 9) + 1,)
        want = bcs.expected(sig, pos, 0.33, strs)
        assert want["bc_len"] == len(pos), name  # (the generator's positions drop no window)
        het += sum(1 for a, b in zip(want["primary"], want["secondary"]) if a != b)
        for s in strs:
            got = run(emu, sig, pos, 0.33, s, int16=(i % 2 == 1))
            bcs.compare(got, want, s, name)  # status 0: none of the synthetic traces is deferred
            assert got["untouched"], name
    assert het > 10000


def test_crafted_corner_cases(emu):
    seen = set()
    for name, sig, pos in bcs.crafted():
        for ratio in bcs.SIGRATIOS:
            strs = (0, 1, 4, 9) if ratio != 0.33 else tuple(range(0, 10))
            want = bcs.expected(sig, pos, ratio, [s for s in strs if s])
            for s in strs:
                for i16 in (False, True):
                    got = run(emu, sig, pos, ratio, s, int16=i16)
                    bcs.compare(got, want, s, (name, ratio, i16))
                    assert got["untouched"], name
            if want["bc_len"] < len(pos):
                seen.add("skipped_window")
            if b"N" in want["primary"]:
                seen.add("N")
            if any(a != b for a, b in zip(want["primary"], want["secondary"])):
                seen.add("het")
            if want["bc_len"] and not want["estqual"].any():
                seen.add("zero_quality")
    assert seen == {"skipped_window", "N", "het", "zero_quality"}


def test_signals_without_optional_outputs(emu):
    """every payload pointer may be null: the per-trace results stay the same"""
    name, sig, pos = bcs.synthetic(1, 1234)[0]
    want = bcs.expected(sig, pos, 0.33, (4,))
    pos = np.ascontiguousarray(pos, np.int32)
    sig = np.ascontiguousarray(sig, np.int32)
    out = (C.c_int32 * 5)()
    rc = emu.emu_basecall(C.c_void_p(sig.ctypes.data), 4, C.c_uint32(sig.shape[1]), C.c_void_p(pos.ctypes.data), C.c_uint32(len(pos)),
                          C.c_float(0.33), C.c_float(4), None, None, None, None, None, None, None, out)
    assert rc == 0
    assert (out[0], out[1], (out[2], out[3]), out[4]) == (0, want["bc_len"], want["trims"][4], want["best_section"])


def test_deferred_traces_are_exactly_the_crafted_ones(emu):
    for name, sig, pos in bcs.deferred():
        for i16 in (False, True):
            got = run(emu, sig, pos, 0.33, 4, int16=i16)
            assert (got["status"], got["bc_len"]) == (1, 0), name
            assert got["untouched"], name


def _job(nt=2, ns=100, npos=5):
    from tracy_amd import capi
    sig = np.zeros((nt, 4, ns), np.int32)
    pos = np.tile(np.arange(10, 10 + 12 * npos, 12, dtype=np.int32), nt)
    job = capi.BasecallJob()
    keep = dict(sig=sig, pos=pos, soff=np.arange(nt, dtype=np.uint64) * 4 * ns, nsamp=np.full(nt, ns, np.uint32),
                poff=np.arange(nt, dtype=np.uint64) * npos, npos=np.full(nt, npos, np.uint32))
    job.ntraces = nt
    job.signal = keep["sig"].ctypes.data
    job.signal_offset = keep["soff"].ctypes.data_as(C.POINTER(C.c_uint64))
    job.nsamples = keep["nsamp"].ctypes.data_as(C.POINTER(C.c_uint32))
    job.sample_bytes = 4
    job.basecallpos = keep["pos"].ctypes.data
    job.pos_offset = keep["poff"].ctypes.data_as(C.POINTER(C.c_uint64))
    job.npos = keep["npos"].ctypes.data_as(C.POINTER(C.c_uint32))
    job.sigratio = 0.33
    job.trim_stringency = 0
    res = capi.BasecallResult()
    keep["meta"] = [np.zeros(nt, np.int32)] + [np.zeros(nt, np.uint32) for _ in range(4)]
    res.status = keep["meta"][0].ctypes.data_as(C.POINTER(C.c_int32))
    for f, a in zip(("bc_len", "trim_left", "trim_right", "best_section"), keep["meta"][1:]):
        setattr(res, f, a.ctypes.data_as(C.POINTER(C.c_uint32)))
    return job, res, keep


def test_argument_validation_needs_no_device():
    """tracyhip_basecall_validate: what tracyhip_basecall_traces checks before it touches a device"""
    from tracy_amd import capi
    lib = capi.lib()
    ERR_ARG = -1
    job, res, keep = _job()
    assert lib.tracyhip_basecall_validate(C.byref(job), 0, C.byref(res)) == 0
    assert lib.tracyhip_basecall_validate(C.byref(job), 1, C.byref(res)) == 0
    assert lib.tracyhip_basecall_validate(None, 0, C.byref(res)) == ERR_ARG
    assert lib.tracyhip_basecall_validate(C.byref(job), 0, None) == ERR_ARG
    assert lib.tracyhip_basecall_validate(C.byref(job), 2, C.byref(res)) == ERR_ARG  # mem
    for field, bad in (("sample_bytes", 3), ("sample_bytes", 0), ("sigratio", float("nan")), ("trim_stringency", float("nan")),
                       ("trim_stringency", -1.0), ("signal", None), ("basecallpos", None), ("signal_offset", None), ("nsamples", None),
                       ("pos_offset", None), ("npos", None)):
        job, res, keep = _job()
        setattr(job, field, bad)
        assert lib.tracyhip_basecall_validate(C.byref(job), 0, C.byref(res)) == ERR_ARG, field
    for field in ("status", "bc_len", "trim_left", "trim_right", "best_section"):
        job, res, keep = _job()
        setattr(res, field, None)
        assert lib.tracyhip_basecall_validate(C.byref(job), 0, C.byref(res)) == ERR_ARG, field
    job, res, keep = _job()  # int16 samples at an odd byte address cannot be read
    job.sample_bytes = 2
    job.signal = keep["sig"].ctypes.data + 1
    assert lib.tracyhip_basecall_validate(C.byref(job), 0, C.byref(res)) == ERR_ARG
    job, res, keep = _job()  # an empty batch is fine
    job.ntraces = 0
    assert lib.tracyhip_basecall_validate(C.byref(job), 0, C.byref(res)) == 0


# ---- basecall_plan.h and ragged_plan.h (chunk cut, descriptors, checks, run-merger) as a program of its own, plain and under the sanitizers ----

PLAN_FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(PLAN_FLAGS))
def test_basecall_plan_program(tmp_path, build):
    exe = tmp_path / ("basecall_plan_" + build)
    # (-Wno-unknown-pragmas: the headers of the wave body, which the plan shares its descriptors with, carry `#pragma unroll` for hipcc)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + PLAN_FLAGS[build] + ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "basecall_plan.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "basecall_plan: ok" in r.stdout


@pytest.mark.parametrize("build", sorted(PLAN_FLAGS))
def test_span_cut_program(tmp_path, build):
    """cut_spans of ragged_plan.h, the one cut behind the five *_cut_chunks, over a toy chunk whose answers can be read off the items"""
    exe = tmp_path / ("span_cut_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + PLAN_FLAGS[build] + ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "span_cut.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "span_cut: ok" in r.stdout
