"""read_scan_body / read_emit_body (tracy_amd/csrc/read_wave.h: ABIF and SCF file images to chromatograms and calls, one wave per file and
per tile) on the 64-fiber host wave, every field against hostlib.read_trace of the same bytes -- exact equality, buffers filled with
sentinels and checked untouched in front of and behind every region.  Plus tracyhost_read_batch, the argument checks and the bound of
tracyhip_read_traces and the stand-alone program over read_plan.h, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import read_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENT, SENT8 = -7777, 0x7e


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_read.so")
    srcs = [os.path.join(HERE, "emu", "emu_read.cpp"), os.path.join(HERE, "emu", "host_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/read_wave.h"), os.path.join(ROOT, "tracy_amd/csrc/dp_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]],
                              stderr=subprocess.DEVNULL)
    lib = C.CDLL(so)
    for f in (lib.emu_read_tile, lib.emu_read_scf_tile, lib.emu_read_bound_samples, lib.emu_read_bound_calls):
        f.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def cases():
    """every named image once, with what the host reader makes of it: dict name -> (image, expected or None)"""
    named = rc.answered() + rc.abif_cases_images() + rc.deferred() + [rc.scf_wide()]
    assert len({n for n, _ in named}) == len(named)
    want = rc.expected([img for _, img in named])
    return {n: (img, w) for (n, img), w in zip(named, want)}


def run(emu, img, int16=False, shift=0, out_shift=0, sample_cap=None, call_cap=None, sizes_only=False, want=None):
    """shift: the image's address mod 4; out_shift: elements in front of the trace's region in every result array (where the wide stores
    begin).  Capacities default to the bound of a file of this length."""
    dt = np.int16 if int16 else np.int32
    buf = np.full(len(img) + 32, 0xEE, np.uint8)
    start = 8 + (shift - (buf.ctypes.data + 8)) % 4
    buf[start:start + len(img)] = np.frombuffer(img, np.uint8)
    scap = emu.emu_read_bound_samples(len(img)) if sample_cap is None else sample_cap
    ccap = emu.emu_read_bound_calls(len(img)) if call_cap is None else call_cap
    o_sig = np.full(out_shift + 4 * scap + 24, SENT, dt)
    o_pos = np.full(out_shift + ccap + 24, SENT, np.int32)
    o_b = {k: np.full(out_shift + ccap + 24, SENT8, np.uint8) for k in ("basecalls1", "basecalls2", "qual")}
    kinds = ("signal", "basecallpos", "basecalls1", "basecalls2", "qual") if want is None else want
    p = lambda a, k: C.c_void_p(a.ctypes.data) if (not sizes_only and k in kinds) else None
    out = (C.c_int32 * 4)()
    emu.emu_read(C.c_void_p(buf.ctypes.data), C.c_uint64(start), C.c_uint32(len(img)), 2 if int16 else 4, p(o_sig, "signal"), C.c_uint64(out_shift),
                 C.c_uint32(scap), p(o_pos, "basecallpos"), p(o_b["basecalls1"], "basecalls1"), p(o_b["basecalls2"], "basecalls2"), p(o_b["qual"], "qual"),
                 C.c_uint64(out_shift), C.c_uint32(ccap), out)
    status, ns, nc = out[0], out[2], out[3]
    g = dict(status=status, format=out[1], nsamples=ns, ncalls=nc)
    wrote = status == rc.OK and not sizes_only
    ks = 4 * ns if wrote and "signal" in kinds else 0
    kc = lambda k: nc if wrote and k in kinds else 0
    g["untouched"] = bool((o_sig[:out_shift] == SENT).all() and (o_sig[out_shift + ks:] == SENT).all()
                          and (o_pos[:out_shift] == SENT).all() and (o_pos[out_shift + kc("basecallpos"):] == SENT).all()
                          and all((o_b[k][:out_shift] == SENT8).all() and (o_b[k][out_shift + kc(k):] == SENT8).all() for k in o_b)
                          and (buf[:start] == 0xEE).all() and (buf[start + len(img):] == 0xEE).all())
    g.update(signal=o_sig[out_shift:out_shift + ks].reshape(4, -1) if ks else o_sig[:0].reshape(4, 0), basecallpos=o_pos[out_shift:out_shift + kc("basecallpos")],
             basecalls1=o_b["basecalls1"][out_shift:out_shift + kc("basecalls1")].tobytes(),
             basecalls2=o_b["basecalls2"][out_shift:out_shift + kc("basecalls2")].tobytes(), qual=o_b["qual"][out_shift:out_shift + kc("qual")])
    return g


ANSWERED = [n for n, _ in rc.answered()] + ["abif_case%d" % i for i in range(5)]
DEFERRED = [n for n, _ in rc.deferred()]


def test_tiles_are_what_the_cases_were_built_for(emu):
    assert emu.emu_read_tile() == rc.ABIF_TILE and emu.emu_read_scf_tile() == rc.SCF_TILE


def test_answered_cases_equal_the_host_reader(emu, cases):
    for i, name in enumerate(ANSWERED):
        img, want = cases[name]
        assert want is not None, name
        every = name.startswith("chan_mod")  # each channel offset mod 4 with the image at each offset mod 4, and where the stores begin
        for i16 in (False, True):
            for shift in ((0, 1, 2, 3) if every else (i % 4,)):
                for out_shift in ((0, 1, 5) if every else (i % 8,)):
                    g = run(emu, img, int16=i16, shift=shift, out_shift=out_shift)
                    assert g["status"] == rc.OK, (name, i16, shift, out_shift)
                    assert rc.same(g, want) is None, (name, i16, shift, out_shift, rc.same(g, want))
                    assert g["untouched"], (name, i16, shift, out_shift)


def test_every_store_alignment_of_a_short_and_a_tile_wide_channel(emu, cases):
    for name in ("abif_ns65", "abif_ns%d" % (rc.ABIF_TILE + 1), "scf_ns65"):
        img, want = cases[name]
        for out_shift in range(8):
            for i16 in (False, True):
                g = run(emu, img, int16=i16, shift=out_shift % 4, out_shift=out_shift)
                assert g["status"] == rc.OK and rc.same(g, want) is None and g["untouched"], (name, out_shift, i16)


def test_the_cases_hit_what_they_are_named_for(cases):
    w = cases["two_calls_in_slots"][1]
    assert w["basecalls1"] == b"AC" and len(w["basecallpos"]) == 2
    assert len(cases["pbas_ends_the_file"][1]["basecallpos"]) == 9
    assert cases["p2ba_absent"][1]["basecalls2"] == bytes(12)
    # (eleven secondaries and the byte past them -- the first quality, which is no letter -- make twelve: the common length stays 12)
    assert len(cases["p2ba_one_shorter"][1]["basecalls1"]) == 12 and cases["p2ba_one_shorter"][1]["basecalls2"][11:] == b"N"
    assert len(cases["more_qualities_than_calls"][1]["qual"]) == 12
    assert cases["primaries_with_N_R_Y"][1]["basecalls1"][3:6] == b"NNN" and cases["primaries_with_N_R_Y"][1]["basecalls2"][:6] == b"NNNNNN"
    assert cases["abif_case1"][1]["signal"].min() == -7
    assert cases["scf_sums_cross_16_bits"][1]["format"] == 1
    for name in DEFERRED:  # what the host reader does with them: refuses, or reads (repeated tags append, a missing dye leaves a channel empty)
        assert (cases[name][1] is None) == (name not in ("repeated_data9", "channels_of_unequal_counts", "fwo_not_a_permutation")), name


def test_golden_files_against_the_reference_s_stored_answers(emu):
    gold = rc.golden_images()
    assert len(gold) >= 4
    for i, (name, img, want) in enumerate(gold):
        for i16 in (False, True):
            g = run(emu, img, int16=i16, shift=i % 4, out_shift=(3 * i) % 8)
            assert g["status"] == rc.OK and rc.same(g, want) is None and g["untouched"], (name, i16, rc.same(g, want))


def test_scf_whose_samples_leave_int16(emu, cases):
    img, want = cases["scf_leaves_int16"]
    assert want is not None and np.abs(want["signal"]).max() > 32767
    g = run(emu, img, int16=False)
    assert g["status"] == rc.OK and rc.same(g, want) is None and g["untouched"]
    g = run(emu, img, int16=True)
    assert (g["status"], g["format"], g["nsamples"], g["ncalls"]) == (rc.DEFERRED, 1, 0, 0) and g["untouched"]


def test_the_deferred_set_is_exactly_the_listed_one(emu, cases):
    got = set()
    for name, (img, _) in cases.items():
        for i16 in (False, True):
            g = run(emu, img, int16=i16)
            if g["status"] == rc.DEFERRED:
                got.add((name, i16))
                assert (g["nsamples"], g["ncalls"]) == (0, 0) and g["untouched"], name
                assert run(emu, img, int16=i16, sizes_only=True)["status"] == rc.DEFERRED
    assert got == {(n, w) for n in DEFERRED for w in (False, True)} | {("scf_leaves_int16", True)}
    assert run(emu, cases["junk_bytes"][0])["format"] == -1 and run(emu, cases["scf_version_2"][0])["format"] == 1
    assert run(emu, cases["repeated_data9"][0])["format"] == 0
    for cut in (0, 3, 4, 33, 39):  # files shorter than their headers
        for magic in (b"ABIF", b".scf"):
            g = run(emu, (magic + bytes(60))[:cut])
            assert g["status"] == rc.DEFERRED and g["untouched"], (cut, magic)


def test_sizes_only_form_equals_the_full_form(emu, cases):
    for name, (img, _) in cases.items():
        full, sizes = run(emu, img), run(emu, img, sizes_only=True)
        for k in ("status", "format", "nsamples", "ncalls"):
            assert full[k] == sizes[k], (name, k)
        assert sizes["untouched"], name


def test_too_small_by_one_sample_and_by_one_call(emu, cases):
    for name in ("chan_mod1", "abif_ns%d" % rc.ABIF_TILE, "scf_ns65", "two_calls_in_slots"):
        img, want = cases[name]
        ns, nc = want["signal"].shape[1], len(want["basecallpos"])
        g = run(emu, img, sample_cap=ns, call_cap=nc)  # exactly enough
        assert g["status"] == rc.OK and rc.same(g, want) is None and g["untouched"], name
        for caps in ((ns - 1, nc), (ns, nc - 1)):
            g = run(emu, img, sample_cap=caps[0], call_cap=caps[1])
            assert (g["status"], g["nsamples"], g["ncalls"]) == (rc.TOO_SMALL, ns, nc) and g["untouched"], (name, caps)
        # a capacity that is not asked about does not count
        g = run(emu, img, sample_cap=ns, call_cap=0, want=("signal",))
        assert g["status"] == rc.OK and np.array_equal(g["signal"], want["signal"]) and g["untouched"], name
        g = run(emu, img, sample_cap=0, call_cap=nc, want=("basecallpos", "qual"))
        assert g["status"] == rc.OK and np.array_equal(g["basecallpos"], want["basecallpos"]) and np.array_equal(g["qual"], want["qual"]) and g["untouched"], name


def test_the_bound_holds_every_answered_case(emu, cases):
    for name in ANSWERED:
        img, want = cases[name]
        assert want["signal"].shape[1] <= emu.emu_read_bound_samples(len(img)) and len(want["basecallpos"]) <= emu.emu_read_bound_calls(len(img)), name


# ---- tracyhost_read_batch: the readers over images in memory, the fallback of the device call ------------------------------------------


def test_host_batch_equals_the_reader_of_files(cases):
    from tracy_amd import hostlib
    names = list(cases)
    for dt in (np.int32, np.int16):
        for nthreads in (1, 3):
            res = hostlib.read_batch([cases[n][0] for n in names], dt, nthreads)
            for n, r in zip(names, res):
                want = cases[n][1]
                if want is None or (dt == np.int16 and (want["signal"].max(initial=0) > 32767 or want["signal"].min(initial=0) < -32768)):
                    assert r["status"] == 1 and (r["nsamples"], r["ncalls"]) == (0, 0), n
                    continue
                assert r["status"] == 0 and rc.same(r, want) is None, (n, rc.same(r, want))
    flat = hostlib.read_pack([cases[n][0] for n in names])
    nt = flat["nt"]
    small = hostlib.read_batch_raw(flat, hostlib.read_alloc(nt, np.int32, np.ones(nt, np.uint32), np.ones(nt, np.uint32), fill=9))
    assert set(small["status"][:nt].tolist()) == {1, 2} and (small["signal"] == 9).all() and (small["qual"] == 9).all()


# ---- tracyhip_read_validate / tracyhip_read_bound: what tracyhip_read_traces checks before it touches a device ----------------------------


def _job(cases, nt=3, payload=True):
    from tracy_amd import capi
    p = capi.PreparedRead([cases[n][0] for n in ANSWERED[:nt]], np.int16)
    return p.with_capacity(*p.bounds()) if payload else p


def test_read_validate_rejections_and_the_bound(cases):
    from tracy_amd import capi
    lib = capi.lib()
    check = lambda p, mem=0: lib.tracyhip_read_validate(C.byref(p.job), mem, C.byref(p.out))
    assert check(_job(cases)) == 0 and check(_job(cases), 1) == 0 and check(_job(cases, payload=False)) == 0 and check(_job(cases, 0)) == 0
    p = _job(cases)
    assert lib.tracyhip_read_validate(None, 0, C.byref(p.out)) == capi.ERR_ARG and lib.tracyhip_read_validate(C.byref(p.job), 0, None) == capi.ERR_ARG
    assert check(p, 2) == capi.ERR_ARG and b"mem" in lib.tracyhip_last_error()
    for sb in (0, 1, 3, 8):
        p = _job(cases)
        p.job.sample_bytes = sb
        assert check(p) == capi.ERR_ARG and b"sample_bytes" in lib.tracyhip_last_error()
    for field in ("bytes", "file_offset", "file_len"):
        p = _job(cases)
        setattr(p.job, field, None)
        assert check(p) == capi.ERR_ARG, field
    for field in ("status", "format", "nsamples", "ncalls", "sample_offset", "sample_cap", "call_offset", "call_cap"):
        p = _job(cases)
        setattr(p.out, field, None)
        assert check(p) == capi.ERR_ARG, field
    p = _job(cases)
    p.out.basecallpos += 2
    assert check(p) == capi.ERR_ARG and b"aligned" in lib.tracyhip_last_error()
    p = _job(cases)
    p.out.signal += 1
    assert check(p) == capi.ERR_ARG and b"aligned" in lib.tracyhip_last_error()
    p = _job(cases)
    p.job.bytes += 3  # the images lie at any address
    assert check(p) == 0
    # the sizes-only form needs no offset or capacity of the results
    p = _job(cases, payload=False)
    assert check(p) == 0 and not p.out.sample_offset and not p.out.call_cap
    # the call itself answers the same before it looks for a device
    p = _job(cases)
    p.job.sample_bytes = 3
    assert lib.tracyhip_read_traces(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG
    assert lib.tracyhip_read_traces_async(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG
    # four channels take 8 bytes a sample, the positions 2 bytes a call; both stop at what the device answers
    assert capi.read_bound(0) == (0, 0) and capi.read_bound(7) == (0, 3) and capi.read_bound(100001) == (12500, 50000)
    assert capi.read_bound(2 ** 32 - 1) == (2 ** 23, 131071) and capi.read_bound(8 * 2 ** 23 - 1) == (2 ** 23 - 1, 131071)
    ns = C.c_uint32(0)
    assert lib.tracyhip_read_bound(C.c_uint32(100), None, C.byref(ns)) == capi.ERR_ARG


# ---- read_plan.h (chunk cut, descriptors, checks) as a program of its own, plain and under the sanitizers --------------------------------

PLAN_FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(PLAN_FLAGS))
def test_read_plan_program(tmp_path, build):
    exe = tmp_path / ("read_plan_" + build)
    # (-Wno-unknown-pragmas: the header of the wave bodies, which the plan shares its descriptors with, carries `#pragma unroll` for hipcc)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + PLAN_FLAGS[build] + ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "read_plan.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "read_plan: ok" in r.stdout
