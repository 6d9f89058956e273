"""pad_wave_body (tracy_amd/csrc/pad_wave.h: hard trim + reverse complement + alignment padding of one trace on one wave) on the 64-fiber
host wave, every output field against the restatements of tests/assemble_oracle.py and tests/sage_oracle.py -- exact equality, buffers
filled with sentinels and checked untouched past the reported sizes.  Plus the argument checks of tracyhip_pad_traces and the stand-alone
program over pad_plan.h, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pad_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENT32, SENT8 = -7777, 0x7e


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_pad.so")
    srcs = [os.path.join(HERE, "emu", "emu_pad.cpp"), os.path.join(HERE, "emu", "host_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/pad_wave.h"), os.path.join(ROOT, "tracy_amd/csrc/dp_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]],
                              stderr=subprocess.DEVNULL)
    lib = C.CDLL(so)
    lib.emu_pad_insert_tile.restype = lib.emu_pad_sample_tile.restype = C.c_uint32
    return lib


def run(emu, c, int16=False, shift=0, sample_cap=None, call_cap=None, sizes_only=False, want=None):
    """want: the payload kinds to ask for (default all).  Capacities default to room for every column of the row as a gap of 224 samples
    (no case here has a larger step), at most 2^16 samples per channel."""
    dt = np.int16 if int16 else np.int32
    sig = np.ascontiguousarray(c["sig"], dtype=dt)
    ns, n = sig.shape[1], len(c["bcpos"])
    pos = np.ascontiguousarray(list(c["bcpos"]) + [0], dtype=np.int32)
    arr = lambda b: np.frombuffer(bytes(b) + b"\0", np.uint8).copy()
    pri, sec, con = arr(c["pri"]), arr(c["sec"]), arr(c["con"])
    q = np.ascontiguousarray(list(c["q"]) + [0], dtype=np.uint8)
    row = arr(c["row"])
    scap = min(ns + 224 * len(c["row"]) + 16, 1 << 16) if sample_cap is None else sample_cap
    ccap = n + len(c["row"]) if call_cap is None else call_cap
    o_sig = np.full(shift + 4 * scap + 8, SENT32, dt)
    o_pos = np.full(ccap + 8, SENT32, np.int32)
    o_b = {k: np.full(ccap + 8, SENT8, np.uint8) for k in ("primary", "secondary", "consensus", "estQual")}
    out = (C.c_int32 * 6)()
    kinds = ("signal", "bcPos", "primary", "secondary", "consensus", "estQual") if want is None else want
    p = lambda a, k: C.c_void_p(a.ctypes.data) if (not sizes_only and k in kinds) else None
    rc = emu.emu_pad(C.c_void_p(sig.ctypes.data), 2 if int16 else 4, C.c_uint32(ns), C.c_void_p(pos.ctypes.data), C.c_void_p(pri.ctypes.data),
                     C.c_void_p(sec.ctypes.data), C.c_void_p(con.ctypes.data), C.c_void_p(q.ctypes.data), C.c_uint32(n), C.c_void_p(row.ctypes.data),
                     C.c_uint32(len(c["row"])), C.c_uint32(c["l"]), C.c_uint32(c["r"]), C.c_uint32(1 if c["reverse"] else 0),
                     p(o_sig, "signal"), C.c_uint64(shift), C.c_uint32(scap), p(o_pos, "bcPos"), p(o_b["primary"], "primary"),
                     p(o_b["secondary"], "secondary"), p(o_b["consensus"], "consensus"), p(o_b["estQual"], "estQual"), C.c_uint32(ccap), out)
    assert rc == 0, "the body wrote past its scratch region"
    status, nso, nco = out[0], out[1], out[2]
    g = dict(status=status, nsamples_out=nso, ncalls_out=nco, leadingGaps=out[3], trailingGaps=out[4], step=out[5])
    wrote = status == pc.OK and not sizes_only
    ks, kc = (4 * nso if wrote and "signal" in kinds else 0), (nco if wrote else 0)
    body = o_sig[shift:shift + ks]
    g["untouched"] = bool((o_sig[:shift] == SENT32).all() and (o_sig[shift + ks:] == SENT32).all()
                          and (o_pos[kc if "bcPos" in kinds else 0:] == SENT32).all()
                          and all((o_b[k][kc if k in kinds else 0:] == SENT8).all() for k in o_b))
    g.update(signal=body.reshape(4, -1) if ks else body, bcPos=o_pos[:kc], primary=o_b["primary"][:kc].tobytes(),
             secondary=o_b["secondary"][:kc].tobytes(), consensus=o_b["consensus"][:kc].tobytes(), estQual=o_b["estQual"][:kc])
    return g


def test_the_three_fixed_cases(emu):
    cases = dict(pc.crafted())
    g = run(emu, cases["adjacent"])
    assert g["bcPos"].tolist() == [5, 6, 7, 8] and g["primary"] == b"--" + cases["adjacent"]["pri"] and g["step"] == 1
    g = run(emu, cases["apart"])
    assert g["bcPos"].tolist() == [5, 7, 10, 14] and g["primary"] == cases["apart"]["pri"][:1] + b"--" + cases["apart"]["pri"][1:] and g["step"] == 3
    assert g["estQual"].tolist()[1:3] == [0, 0] and g["secondary"][1:3] == b"--" and g["consensus"][1:3] == b"--"
    g = run(emu, cases["lead_trail"])
    assert (g["leadingGaps"], g["trailingGaps"], g["nsamples_out"], g["ncalls_out"], g["step"]) == (2, 2, 24, 3, 4)
    assert (g["signal"][:, 8:12] == -99).all() and (g["signal"][:, :8] == cases["lead_trail"]["sig"][:, :8]).all()
    for name in ("adjacent", "apart", "lead_trail"):
        pc.compare(run(emu, cases[name]), pc.expected(cases[name]), name)


def test_crafted_cases_in_both_sample_widths_and_every_alignment(emu):
    cases = pc.crafted(emu.emu_pad_insert_tile(), emu.emu_pad_sample_tile())
    assert emu.emu_pad_insert_tile() == 256 and emu.emu_pad_sample_tile() == 256  # what pad_cases.crafted() takes when nobody tells it
    for i, (name, c) in enumerate(cases):
        want = pc.expected(c)
        for i16 in (False, True):
            for shift in ((0, 1, 2, 3) if len(c["bcpos"]) < 200 else (i % 4,)):  # where the wide stores of each channel begin
                g = run(emu, c, int16=i16, shift=shift)
                pc.compare(g, want, (name, i16, shift))
                assert g["untouched"], (name, i16, shift)
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names)


def test_the_cases_hit_what_they_are_named_for(emu):
    cases = dict(pc.crafted())
    st = emu.emu_pad_sample_tile()
    e = pc.expected(cases["insert_ends_sample_tile"])
    # (the sample at q itself is a source sample; the empty ones follow it)
    assert (e["signal"][:, st:st + e["step"]] == -99).all() and (e["signal"][:, st - 1] == cases["insert_ends_sample_tile"]["sig"][:, st - 1]).all()
    e = pc.expected(cases["insert_opens_sample_tile"])
    assert (e["signal"][:, st + 1:st + 1 + e["step"]] == -99).all() and (e["signal"][:, st] == cases["insert_opens_sample_tile"]["sig"][:, st]).all()
    e = pc.expected(cases["more_inserts_than_a_tile"])
    assert e["primary"].count(b"-") > emu.emu_pad_insert_tile()
    assert pc.expected(cases["mean_not_integer"])["step"] == 5 and pc.expected(cases["one_call"])["step"] == 6
    c = cases["last_possible_insert"]
    assert (c["bcpos"][1] + c["bcpos"][2]) // 2 == c["sig"].shape[1] - 2
    e = pc.expected(cases["reverse_table"])
    tab = pc.COMPLEMENT_FROM + b"Xa"
    assert e["primary"].replace(b"-", b"") == b"TGCANDBKRHVMYASWXa"[::-1] and cases["reverse_table"]["pri"] == tab
    row = cases["run_straddles_63_64"]["row"]
    assert b"-" not in row[:62] and row[62:66] == b"----" and row[66:67] != b"-"
    row = cases["run_ends_at_63"]["row"]
    assert row[62:64] == b"--" and row[64:65] != b"-" and row[61:62] != b"-"


def test_the_deferred_family(emu):
    for name, c in pc.deferred():
        for i16 in (False, True):
            g = run(emu, c, int16=i16)
            assert (g["status"], g["nsamples_out"], g["ncalls_out"]) == (pc.DEFERRED, 0, 0), name
            assert g["untouched"], name
        g = run(emu, c, sizes_only=True)
        assert (g["status"], g["nsamples_out"], g["ncalls_out"]) == (pc.DEFERRED, 0, 0), name


def test_300_random_small_traces(emu):
    inserts = reverses = trims = 0
    for seed in range(300):
        c = pc.random_small(seed)
        want = pc.expected(c)
        g = run(emu, c, int16=bool(seed & 1), shift=seed % 4)
        pc.compare(g, want, seed)  # (status OK: the generator emits only answerable traces)
        assert g["untouched"], seed
        inserts += want["primary"].count(b"-")
        reverses += c["reverse"]
        trims += bool(c["l"] or c["r"])
    assert inserts > 1000 and reverses > 60 and trims > 60


def test_sizes_only_form_equals_the_full_form(emu):
    for name, c in pc.crafted() + [("random%d" % s, pc.random_small(s)) for s in range(40)]:
        full, sizes = run(emu, c), run(emu, c, sizes_only=True)
        for k in ("status", "nsamples_out", "ncalls_out", "leadingGaps", "trailingGaps", "step"):
            assert full[k] == sizes[k], (name, k)
        assert sizes["untouched"], name


def test_too_small_by_one_sample_and_by_one_call(emu):
    for name in ("apart", "lead_trail", "inserts_across_sample_tiles", "reverse_trims"):
        c = dict(pc.crafted())[name]
        want = pc.expected(c)
        nso, nco = want["signal"].shape[1], len(want["bcPos"])
        g = run(emu, c, sample_cap=nso, call_cap=nco)  # exactly enough
        pc.compare(g, want, name)
        assert g["untouched"], name
        for caps in ((nso - 1, nco), (nso, nco - 1)):
            g = run(emu, c, sample_cap=caps[0], call_cap=caps[1])
            assert (g["status"], g["nsamples_out"], g["ncalls_out"]) == (pc.TOO_SMALL, nso, nco), (name, caps)
            assert (g["leadingGaps"], g["trailingGaps"], g["step"]) == (want["leadingGaps"], want["trailingGaps"], want["step"])
            assert g["untouched"], (name, caps)
        # a capacity that is not asked about does not count
        g = run(emu, c, sample_cap=nso, call_cap=0, want=("signal",))
        assert g["status"] == pc.OK and (g["signal"] == want["signal"]).all() and g["untouched"], name
        g = run(emu, c, sample_cap=0, call_cap=nco, want=("bcPos", "estQual"))
        assert g["status"] == pc.OK and (g["bcPos"] == want["bcPos"]).all() and (g["estQual"] == want["estQual"]).all() and g["untouched"], name


# ---- tracyhip_pad_validate: what tracyhip_pad_traces checks before it touches a device -----------------------------------------------


def _job(nt=3, payload=True, trims=True):
    from tracy_amd import capi
    cases = [pc.random_small(s) for s in range(nt)]
    return capi.PreparedPad([c["sig"] for c in cases], [dict(bcpos=c["bcpos"], primary=c["pri"], secondary=c["sec"], consensus=c["con"], estqual=c["q"])
                                                        for c in cases], [c["row"] for c in cases],
                            trim_left=[c["l"] for c in cases] if trims else None, trim_right=[c["r"] for c in cases] if trims else None,
                            reverse=[c["reverse"] for c in cases]).with_capacity([300] * nt, [200] * nt) if payload else \
        capi.PreparedPad([c["sig"] for c in cases], [dict(bcpos=c["bcpos"], primary=c["pri"], secondary=c["sec"], consensus=c["con"], estqual=c["q"])
                                                     for c in cases], [c["row"] for c in cases])


def test_pad_validate_rejections():
    from tracy_amd import capi
    lib = capi.lib()
    check = lambda p, mem=0: lib.tracyhip_pad_validate(C.byref(p.job), mem, C.byref(p.out))
    assert check(_job()) == 0 and check(_job(), 1) == 0 and check(_job(payload=False)) == 0 and check(_job(0)) == 0
    p = _job()
    assert lib.tracyhip_pad_validate(None, 0, C.byref(p.out)) == capi.ERR_ARG and lib.tracyhip_pad_validate(C.byref(p.job), 0, None) == capi.ERR_ARG
    assert check(p, 2) == capi.ERR_ARG and b"mem" in lib.tracyhip_last_error()
    for sb in (0, 1, 3, 8):
        p = _job()
        p.job.sample_bytes = sb
        assert check(p) == capi.ERR_ARG and b"sample_bytes" in lib.tracyhip_last_error()
    for field in ("nsamples", "bcpos", "bc_offset", "bc_len", "rows", "row_offset", "row_len", "signal", "signal_offset", "primary", "estqual"):
        p = _job()
        setattr(p.job, field, None)
        assert check(p) == capi.ERR_ARG, field
    for field in ("status", "nsamples_out", "ncalls_out", "leading_gaps", "trailing_gaps", "step", "sample_offset", "sample_cap", "call_offset", "call_cap"):
        p = _job()
        setattr(p.out, field, None)
        assert check(p) == capi.ERR_ARG, field
    for field in ("trim_left_each", "trim_right_each"):  # both or neither
        p = _job()
        setattr(p.job, field, None)
        assert check(p) == capi.ERR_ARG and b"both or neither" in lib.tracyhip_last_error()
    p = _job()
    p.job.trim_left_each = p.job.trim_right_each = None
    assert check(p) == 0
    p = _job()
    p.job.bcpos += 2
    assert check(p) == capi.ERR_ARG and b"aligned" in lib.tracyhip_last_error()
    p = _job()
    p.out.signal += 1
    assert check(p) == capi.ERR_ARG and b"aligned" in lib.tracyhip_last_error()
    # the sizes-only form needs neither the chromatograms nor any offset or capacity of the results
    p = _job(payload=False)
    p.job.signal = p.job.signal_offset = None
    assert check(p) == 0
    # the call itself answers the same before it looks for a device
    p = _job()
    p.job.sample_bytes = 3
    assert lib.tracyhip_pad_traces(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG
    assert lib.tracyhip_pad_traces_async(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG


# ---- pad_plan.h (chunk cut, descriptors, checks) as a program of its own, plain and under the sanitizers ------------------------------

PLAN_FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(PLAN_FLAGS))
def test_pad_plan_program(tmp_path, build):
    exe = tmp_path / ("pad_plan_" + build)
    # (-Wno-unknown-pragmas: the headers of the wave body, which the plan shares its descriptors with, carry `#pragma unroll` for hipcc)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + PLAN_FLAGS[build] + ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "pad_plan.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pad_plan: ok" in r.stdout
