"""The trace printing bodies (tracy_amd/csrc/render_wave.h: count, scan and emit of the .abif table, the JSON trace body and the gapped
trace) on the 64-fiber host wave, tile after tile: the text against the host writers (hostlib.render_batch) and the independent
restatements of tests/render_cases.py -- equality of bytes, the buffer filled with a sentinel and checked untouched in front of and
behind the text, at every alignment of its first byte.  Plus the argument checks and the bound of tracyhip_render_traces and the
stand-alone program over render_plan.h, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENT = 0x7e


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_render.so")
    srcs = [os.path.join(HERE, "emu", "emu_render.cpp"), os.path.join(HERE, "emu", "host_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/render_wave.h"), os.path.join(ROOT, "tracy_amd/csrc/dp_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]],
                              stderr=subprocess.DEVNULL)
    lib = C.CDLL(so)
    lib.emu_render_tile.restype = lib.emu_render_max_item.restype = C.c_uint32
    return lib


def flat_of(cases, int16=False):
    from tracy_amd import capi
    sigs = [c["sig"].astype(np.int16) if int16 else c["sig"] for c in cases]
    return capi.PreparedRender(rc.TSV, sigs, [rc.bc_of(c) for c in cases], [c["l"] for c in cases], [c["r"] for c in cases],
                               sample_dtype=np.int16 if int16 else np.int32).flat


def run(emu, c, form, int16=False, shift=0, cap=None, sizes_only=False):
    """one trace through the three bodies; the text starts `shift` bytes into a 16-byte aligned buffer of sentinels"""
    dt = np.int16 if int16 else np.int32
    sig = np.ascontiguousarray(c["sig"], dtype=dt)
    ns, n = sig.shape[1], len(c["bcpos"])
    pos = np.ascontiguousarray(list(c["bcpos"]) + [0], dtype=np.int32)
    arr = lambda b: np.frombuffer(bytes(b) + b"\0", np.uint8).copy()
    pri, sec, con = arr(c["pri"]), arr(c["sec"]), arr(c["con"])
    q = np.ascontiguousarray(list(c["q"]) + [0], dtype=np.uint8)
    room = 100 * ns + 40 * n + 400 if cap is None else cap
    raw = np.full(shift + room + 64 + 16, SENT, np.uint8)
    lead = (-raw.ctypes.data) % 16  # the first byte of `buf` is 16-byte aligned: `shift` is the alignment of the text
    buf = raw[lead:lead + shift + room + 48]
    out = (C.c_int32 * 2)()
    r = emu.emu_render(C.c_uint32(form), C.c_void_p(sig.ctypes.data), 2 if int16 else 4, C.c_uint32(ns), C.c_void_p(pos.ctypes.data),
                       C.c_void_p(pri.ctypes.data), C.c_void_p(sec.ctypes.data), C.c_void_p(con.ctypes.data), C.c_void_p(q.ctypes.data), C.c_uint32(n),
                       C.c_uint32(c["l"]), C.c_uint32(c["r"]), None if sizes_only else C.c_void_p(buf.ctypes.data), C.c_uint64(shift), C.c_uint64(room), out)
    assert r == 0, "an item longer than the LDS image allows" if r == 1 else "a body wrote past the tile scratch"
    status, ln = out[0], out[1]
    wrote = ln if (status == rc.OK and not sizes_only) else 0
    return dict(status=status, text_len=ln, text=buf[shift:shift + wrote].tobytes(),
                untouched=bool((raw[:lead + shift] == SENT).all() and (raw[lead + shift + wrote:] == SENT).all()))


def test_the_tile_is_what_the_cases_assume(emu):
    assert emu.emu_render_tile() == 256 and emu.emu_render_max_item() >= 75


@pytest.mark.parametrize("form", rc.FORMS)
def test_crafted_cases_against_the_host_writers_and_the_restatements(emu, form):
    from tracy_amd import hostlib
    for wide in (False, True):
        cases = rc.crafted(emu.emu_render_tile(), wide)
        host = hostlib.render_batch(flat_of([c for _, c in cases], int16=not wide), form, 2)
        for i, ((name, c), h) in enumerate(zip(cases, host)):
            want = rc.expected(c, form)
            assert h["status"] == rc.OK and h["text"] == want, (name, "host")
            g = run(emu, c, form, int16=not wide, shift=i % 16)
            assert g["status"] == rc.OK and g["text_len"] == len(want), name
            assert g["text"] == want, name
            assert g["untouched"], name
            assert len(want) <= hostlib_bound(form, c, 4 if wide else 2), name
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names)


def hostlib_bound(form, c, sb):
    from tracy_amd import capi
    return capi.render_bound(form, c["sig"].shape[1], len(c["bcpos"]), sb)


@pytest.mark.parametrize("form", rc.FORMS)
def test_every_alignment_of_the_first_byte_and_short_texts(emu, form):
    """texts shorter than one 16-byte word, texts that end on a word boundary, every head and tail"""
    cases = dict(rc.crafted(emu.emu_render_tile()))
    for name in ("ns1", "ns63", "one_call_at_0", "gap_beside_letter"):
        want = rc.expected(cases[name], form)
        for shift in range(16):
            g = run(emu, cases[name], form, shift=shift)
            assert (g["status"], g["text"]) == (rc.OK, want), (name, shift)
            assert g["untouched"], (name, shift)


def test_the_long_trace_in_the_table_form(emu):
    """100 002 samples: "pos" goes from 99 999 to 100 000, where the host writer leaves its five-digit path"""
    from tracy_amd import hostlib
    c = rc.long_trace()
    want = rc.expected(c, rc.TSV)
    assert b"\n99999\t" in want and b"\n100000\t" in want
    assert hostlib.render_batch(flat_of([c]), rc.TSV, 1)[0]["text"] == want
    g = run(emu, c, rc.TSV, shift=5)
    assert (g["status"], g["text"]) == (rc.OK, want) and g["untouched"]


def test_the_cases_hit_what_they_are_named_for(emu):
    T = emu.emu_render_tile()
    cases = dict(rc.crafted(T))
    c = cases["calls_fill_a_tile"]
    assert set(range(T, 2 * T)) <= set(c["bcpos"])
    assert len(cases["more_calls_than_a_tile"]["bcpos"]) > T and len(cases["gaps_across_call_tiles"]["bcpos"]) > T
    assert cases["gaps_across_call_tiles"]["pri"][T - 5:T + 5] == b"-" * 10
    assert set(cases["all_gaps"]["pri"]) == {ord("-")}
    assert b"\"-\"" in rc.expected(cases["gap_runs"], rc.GAPPED) and b":A|-\"" in rc.expected(cases["gap_beside_letter"], rc.GAPPED)
    assert b", 9999, 10000, " in rc.expected(cases["pos_digits_10000"], rc.JSON)
    t = rc.expected(cases["trim_right_beyond"], rc.TSV)
    assert b"\tN\n" not in t and b"\tY\n" in t
    t = rc.expected(cases["trim_left_beyond"], rc.TSV)
    assert b"\tN\n" not in t
    t = rc.expected(cases["trim_0_0"], rc.TSV)
    assert b"\tY\n" not in t
    j = rc.expected(cases["ns257"], rc.JSON)
    for exp in (b"|A|G\"", b"|C|T\"", b"|C|G\"", b"|A|T\"", b"|G|T\"", b"|A|C\"", b"|N\""):
        assert exp in j, exp
    wide = rc.expected(dict(rc.crafted(T, True))["ns257"], rc.TSV)
    for v in (b"\t2147483647\t", b"\t-2147483648\t", b"\t99999\t", b"\t100000\t", b"\t-32768\t", b"\t32767\t"):
        assert v in wide, v
    for q in (b"\t0\t", b"\t9\t", b"\t10\t", b"\t99\t", b"\t100\t", b"\t255\t"):
        assert q in wide, q
    assert b"\"1\":\"1:A\"" in rc.expected(cases["primary_equals_secondary"], rc.JSON)


def test_the_deferred_family(emu):
    from tracy_amd import hostlib
    items = rc.deferred()
    for form in rc.FORMS:
        host = hostlib.render_batch(flat_of([c for _, c in items]), form, 2)
        for (name, c), h in zip(items, host):
            assert (h["status"], h["text_len"]) == (rc.DEFERRED, 0), (name, "host")
            for int16 in (False, True):
                g = run(emu, c, form, int16=int16, shift=3)
                assert (g["status"], g["text_len"]) == (rc.DEFERRED, 0), name
                assert g["untouched"], name
            g = run(emu, c, form, sizes_only=True)
            assert (g["status"], g["text_len"]) == (rc.DEFERRED, 0), name


def test_sizes_only_and_too_small(emu):
    cases = dict(rc.crafted(emu.emu_render_tile()))
    for form in rc.FORMS:
        for name in ("ns65", "gap_runs", "trim_3_5"):
            want = rc.expected(cases[name], form)
            g = run(emu, cases[name], form, sizes_only=True)
            assert (g["status"], g["text_len"]) == (rc.OK, len(want)) and g["untouched"], name
            g = run(emu, cases[name], form, shift=7, cap=len(want))  # exactly enough
            assert (g["status"], g["text"]) == (rc.OK, want) and g["untouched"], name
            g = run(emu, cases[name], form, shift=7, cap=len(want) - 1)
            assert (g["status"], g["text_len"]) == (rc.TOO_SMALL, len(want)) and g["untouched"], name


def test_300_random_small_traces(emu):
    from tracy_amd import hostlib
    rng = np.random.default_rng(5)
    cases = []
    for seed in range(300):
        ns = int(rng.integers(1, 400))
        n = int(rng.integers(1, min(ns, 120) + 1))
        pos = np.sort(rng.choice(ns, n, replace=False))
        gaps = tuple(int(x) for x in rng.choice(n, int(rng.integers(0, n // 2 + 1)), replace=False)) if seed % 3 == 0 else ()
        cases.append(rc.make(ns, pos, wide=bool(seed & 1), seed=seed, gaps=gaps, l=int(rng.integers(0, n + 2)), r=int(rng.integers(0, n + 2))))
    for wide in (False, True):
        pick = [c for i, c in enumerate(cases) if bool(i & 1) == wide]
        for form in rc.FORMS:
            host = hostlib.render_batch(flat_of(pick, int16=not wide), form, 2)
            for i, (c, h) in enumerate(zip(pick, host)):
                want = rc.expected(c, form)
                assert h["text"] == want, (i, form, "host")
                if i % 3 == form:  # (every trace through the emulator in one form)
                    g = run(emu, c, form, int16=not wide, shift=i % 16)
                    assert (g["status"], g["text"]) == (rc.OK, want) and g["untouched"], (i, form)


# ---- tracyhip_render_validate / tracyhip_render_bound: what needs no device -------------------------------------------------------------


def _job(nt=3, payload=True, form=rc.TSV, trims=True):
    from tracy_amd import capi
    cases = [c for _, c in rc.crafted()[:nt]]
    p = capi.PreparedRender(form, [c["sig"] for c in cases], [rc.bc_of(c) for c in cases], [c["l"] for c in cases] if trims else None,
                            [c["r"] for c in cases] if trims else None)
    return p.with_capacity(p.bounds()) if payload else p


def test_render_validate_rejections():
    from tracy_amd import capi
    lib = capi.lib()
    check = lambda p, mem=0: lib.tracyhip_render_validate(C.byref(p.job), mem, C.byref(p.out))
    assert check(_job()) == 0 and check(_job(), 1) == 0 and check(_job(payload=False)) == 0 and check(_job(0)) == 0
    p = _job()
    assert lib.tracyhip_render_validate(None, 0, C.byref(p.out)) == capi.ERR_ARG and lib.tracyhip_render_validate(C.byref(p.job), 0, None) == capi.ERR_ARG
    assert check(p, 2) == capi.ERR_ARG and b"mem" in lib.tracyhip_last_error()
    p.job.form = 3
    assert check(p) == capi.ERR_ARG and b"form" in lib.tracyhip_last_error()
    for sb in (0, 1, 3, 8):
        p = _job()
        p.job.sample_bytes = sb
        assert check(p) == capi.ERR_ARG and b"sample_bytes" in lib.tracyhip_last_error()
    for field in ("signal", "signal_offset", "nsamples", "bcpos", "primary", "secondary", "estqual", "bc_offset", "bc_len", "consensus"):
        for payload in (True, False):  # the sizes-only form reads the same arrays
            p = _job(payload=payload)
            setattr(p.job, field, None)
            assert check(p) == capi.ERR_ARG, field
    for form in (rc.JSON, rc.GAPPED):  # the consensus is printed by the table alone
        p = _job(form=form)
        p.job.consensus = None
        assert check(p) == 0
    for field in ("status", "text_len", "text_offset", "text_cap"):
        p = _job()
        setattr(p.out, field, None)
        assert check(p) == capi.ERR_ARG, field
    for field in ("trim_left_each", "trim_right_each"):  # both or neither
        p = _job()
        setattr(p.job, field, None)
        assert check(p) == capi.ERR_ARG and b"both or neither" in lib.tracyhip_last_error()
    p = _job(trims=False)
    assert check(p) == 0
    p = _job()
    p.job.bcpos += 2
    assert check(p) == capi.ERR_ARG and b"aligned" in lib.tracyhip_last_error()
    p = _job()
    p.job.signal += 1
    assert check(p) == capi.ERR_ARG and b"aligned" in lib.tracyhip_last_error()
    # the call itself answers the same before it looks for a device
    p = _job()
    p.job.sample_bytes = 3
    assert lib.tracyhip_render_traces(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG
    assert lib.tracyhip_render_traces_async(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG


def test_render_bound_covers_every_case_and_the_worst_values():
    from tracy_amd import capi
    for wide in (False, True):
        for name, c in rc.crafted(wide=wide) + [("long", rc.long_trace(wide))]:
            for form in rc.FORMS:
                if name == "long" and form != rc.TSV and wide:
                    continue  # (the restatements of the two JSON forms take a while on 100 002 samples: once is enough)
                assert capi.render_bound(form, c["sig"].shape[1], len(c["bcpos"]), 4 if wide else 2) >= len(rc.expected(c, form)), (name, form)
    # every value the most negative one, every quality of three digits, every secondary one that expands to three characters
    ns, n = 1203, 1100
    worst = dict(sig=np.full((4, ns), -2 ** 31, np.int64), bcpos=list(range(ns - n, ns)), pri=b"A" * n, sec=b"R" * n, con=b"A" * n,
                 q=np.full(n, 255, np.uint8), l=0, r=0)
    for form in rc.FORMS:
        b = capi.render_bound(form, ns, n, 4)
        assert len(rc.expected(worst, form)) <= b <= 2 * len(rc.expected(worst, form))
    worst["sig"] = np.full((4, ns), -32768, np.int64)
    for form in rc.FORMS:
        assert len(rc.expected(worst, form)) <= capi.render_bound(form, ns, n, 2)
    assert capi.render_bound(3, 10, 10, 4) == 0
    assert all(capi.render_bound(f, 1 << 23, 131071, 4) < 2 ** 31 for f in rc.FORMS)


# ---- render_plan.h and the sinks of render_wave.h as a program of its own, plain and under the sanitizers ------------------------------

PLAN_FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(PLAN_FLAGS))
def test_render_plan_program(tmp_path, build):
    exe = tmp_path / ("render_plan_" + build)
    # (-Wno-unknown-pragmas: the headers of the wave body, which the plan shares its descriptors with, may carry `#pragma unroll` for hipcc)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + PLAN_FLAGS[build] + ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "render_plan.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "render_plan: ok" in r.stdout
