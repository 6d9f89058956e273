"""The decompose report printing bodies (tracy_amd/csrc/dcptext_wave.h: count, scan and emit of the .decomp table, the JSON tail and the
VCF record lines) on the 64-fiber host wave, tile after tile: the text against the host writers (hostlib.dcptext_batch) and the
independent restatement of tests/dcptext_cases.py -- equality of bytes, the buffer filled with a sentinel and checked untouched in front
of and behind the text, at every alignment of its first byte.  Plus the argument checks and the bound of
tracyhip_render_decompositions and the stand-alone program over dcptext_plan.h, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dcptext_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENT = 0x7e


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_dcptext.so")
    srcs = [os.path.join(HERE, "emu", "emu_dcptext.cpp"), os.path.join(HERE, "emu", "host_wave.h")]
    srcs += [os.path.join(ROOT, "tracy_amd/csrc", f) for f in ("dcptext_wave.h", "dcptext_plan.h", "render_wave.h", "ragged_plan.h", "dp_lane.h")]
    srcs.append(os.path.join(ROOT, "include", "tracy_hip.h"))
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], stderr=subprocess.DEVNULL)
    lib = C.CDLL(so)
    lib.emu_dcptext_tile.restype = C.c_uint32
    return lib


def pack(c):
    from tracy_amd import hostlib
    return hostlib.dcptext_pack([c], c["maxv"], c["maxt"])


def bound(c, form):
    from tracy_amd import capi
    return capi.dcptext_bound(form, len(c["dcp"]), [len(r[0]) for r in c["rows"]], (len(c["chr1"]), len(c["chr2"])), (len(c["frac1"]), len(c["frac2"])),
                              c["maxv"], c["maxt"])


def run(emu, c, form, shift=0, cap=None, sizes_only=False):
    """one trace through the bodies; the text starts `shift` bytes into a 16-byte aligned buffer of sentinels"""
    from tracy_amd import hostlib
    f = pack(c)
    job = hostlib.dcptext_job(f, form, c["qc"], lambda k: f[k].ctypes.data)
    room = bound(c, form) + 8 if cap is None else cap
    raw = np.full(shift + room + 64 + 16, SENT, np.uint8)
    lead = (-raw.ctypes.data) % 16  # the first byte of `buf` is 16-byte aligned: `shift` is the alignment of the text
    buf = raw[lead:lead + shift + room + 48]
    status, text_len = C.c_int32(-1), C.c_uint32(0)
    off, capv = C.c_uint64(shift), C.c_uint64(room)
    r = emu.emu_dcptext(C.byref(job), None if sizes_only else C.c_void_p(buf.ctypes.data), C.byref(off), C.byref(capv), C.byref(status), C.byref(text_len))
    assert r == 0, {2: "a body wrote past the tile scratch", 3: "the job was refused"}[r]
    wrote = text_len.value if (status.value == dc.OK and not sizes_only) else 0
    return dict(status=status.value, text_len=text_len.value, text=buf[shift:shift + wrote].tobytes(),
                untouched=bool((raw[:lead + shift] == SENT).all() and (raw[lead + shift + wrote:] == SENT).all()))


def host_text(c, form):
    from tracy_amd import hostlib
    return hostlib.dcptext_batch(pack(c), form, c["qc"], 2)[0]


def test_the_tile_is_what_the_cases_assume(emu):
    assert emu.emu_dcptext_tile() == dc.TILE


@pytest.mark.parametrize("form", dc.FORMS)
def test_crafted_cases_against_the_host_writers_and_the_restatement(emu, form):
    items = dc.crafted()
    names = [n for n, _ in items]
    assert len(set(names)) == len(names)
    for i, (name, c) in enumerate(items):
        want = dc.expected(c, form)
        assert not dc.is_deferred(c, form), name
        h = host_text(c, form)
        assert (h["status"], h.get("text")) == (dc.OK, want), (name, "host")
        g = run(emu, c, form, shift=i % 16)
        assert g["status"] == dc.OK and g["text_len"] == len(want), name
        assert g["text"] == want, name
        assert g["untouched"], name
        assert len(want) <= bound(c, form), name


@pytest.mark.parametrize("form", dc.FORMS)
def test_every_alignment_of_the_first_byte(emu, form):
    """the row copies put dwords together from two source dwords: every alignment of the text against every alignment of the rows"""
    cases = dict(dc.crafted())
    for name in ("cols0", "cols1", "cols_around_a_tile", "cols_long", "variants1", "table_empty"):
        c = cases[name]
        want = dc.expected(c, form)
        for shift in range(16):
            g = run(emu, c, form, shift=shift)
            assert (g["status"], g["text"]) == (dc.OK, want), (name, shift)
            assert g["untouched"], (name, shift)
    if form == dc.JSON:  # rows of 5 .. 12 columns behind each other: every source alignment, runs shorter than a dword and its head
        for n in range(5, 13):
            c = dc.base(70 + n, cols=(n, n + 1, n + 2))
            for shift in range(4):
                g = run(emu, c, form, shift=shift)
                assert (g["status"], g["text"], g["untouched"]) == (dc.OK, dc.expected(c, form), True), (n, shift)


def test_the_cases_hit_what_they_are_named_for():
    cases = dict(dc.crafted())
    t = dc.expected(cases["table_maxindel1000"], dc.DECOMP)
    assert t.count(b"\n") == 2003 and t.startswith(b"indel\tdecomp\n-1001\t")
    assert b"-2147483648\t2147483647\n" in dc.expected(cases["table_negative"], dc.DECOMP)
    t = dc.expected(cases["table_empty"], dc.JSON)
    assert b"\"x\": [],\n\"y\": []\n" in t and b"\"rows\": [\n],\n\"xranges\": [\n]\n}\n}\n" in t
    t = dc.expected(cases["types_and_genotypes"], dc.JSON)
    for word in (b"\"SNV\"", b"\"Deletion\"", b"\"Insertion\"", b"\"Complex\"", b"\"het.\"", b"\"hom. ALT\""):
        assert word in t
    t = dc.expected(cases["genotypes_outside"], dc.JSON)
    assert b"\"hom. REF\"" in t and t.count(b"\"missing\"") == 2
    t = dc.expected(cases["genotypes_outside"], dc.VCF)
    assert b"\t0/0:" in t and t.count(b"\t./.:") == 2 and t.startswith(b"chr7\t-5\t.\t")
    t = dc.expected(cases["alt_with_N"], dc.VCF).split(b"\n")
    assert t[0].split(b"\t")[5:7] == [b"0", b"LowQual"] and t[0].endswith(b":60") and t[1].split(b"\t")[5] == b"0" and t[2].split(b"\t")[5:7] == [b"60", b"PASS"]
    t = dc.expected(cases["qual_around_the_cut"], dc.JSON)
    assert b"44, \"LowQual\"" in t and b"45, \"PASS\"" in t and b"46, \"PASS\"" in t
    assert dc.expected(cases["qual_cut_16_bits"], dc.JSON) == t
    assert b"\"range\": [1, 194]" in dc.expected(cases["viewport_clamps_at_1"], dc.JSON)
    assert b"\"range\": [1262, 1435]" in dc.expected(cases["viewport_clamps_at_lastpeak"], dc.JSON)
    assert b"\"ref1pos\": 0,\n" in dc.expected(cases["ref_pos_wraps"], dc.JSON) and b"\"ref2pos\": 2147483648,\n" in dc.expected(cases["ref_pos_wraps"], dc.JSON)
    assert b"\"ref1pos\": 4294967295,\n" in dc.expected(cases["ref_pos_large"], dc.JSON)
    assert b"\"ref1chr\": \"ch\"r\\1\"," in dc.expected(cases["names_quotes"], dc.JSON)
    for fw in ("forward", "reverse"):
        t = dc.expected(cases[fw + "_trims50"], dc.VCF)
        assert b"BASEPOS=51;" in t and b"BASEPOS=81;" in t and b"BASEPOS=110;" in t
    assert len(cases["variants_max_two_tiles"]["variants"]) > dc.TILE


def test_the_deferred_family(emu):
    for name, c in dc.deferred() + [dc.cols_over()]:
        for form in dc.FORMS:
            h = host_text(c, form)
            if dc.unreadable(c, form):
                assert (h["status"], h["text_len"]) == (1, 0), (name, form, "host")
            else:
                assert (h["status"], h.get("text")) == (dc.OK, dc.expected(c, form)), (name, form, "host")  # the host prints what the device leaves to it
            if not dc.is_deferred(c, form):
                g = run(emu, c, form, shift=3)
                assert (g["status"], g["text"]) == (dc.OK, h["text"]) and g["untouched"], (name, form)
                continue
            g = run(emu, c, form, shift=3, cap=64)
            assert (g["status"], g["text_len"]) == (dc.DEFERRED, 0), (name, form)
            assert g["untouched"], (name, form)
            g = run(emu, c, form, sizes_only=True)
            assert (g["status"], g["text_len"]) == (dc.DEFERRED, 0), (name, form)
        assert dc.is_deferred(c, dc.JSON), name


def test_sizes_only_and_too_small(emu):
    cases = dict(dc.crafted())
    for form in dc.FORMS:
        for name in ("plain", "types_and_genotypes", "cols_around_a_tile"):
            c = cases[name]
            want = dc.expected(c, form)
            g = run(emu, c, form, sizes_only=True)
            assert (g["status"], g["text_len"]) == (dc.OK, len(want)) and g["untouched"], name
            g = run(emu, c, form, shift=7, cap=len(want))  # exactly enough
            assert (g["status"], g["text"]) == (dc.OK, want) and g["untouched"], name
            if not want:
                continue
            g = run(emu, c, form, shift=7, cap=len(want) - 1)
            assert (g["status"], g["text_len"]) == (dc.TOO_SMALL, len(want)) and g["untouched"], name


# ---- tracyhip_render_decompositions_validate / _bound: what needs no device ------------------------------------------------------------


def _job(form=dc.JSON, payload=True, n=3):
    from tracy_amd import capi, hostlib
    cs = [c for _, c in dc.crafted()[:n]]
    p = capi.PreparedDcpText(form, hostlib.dcptext_pack(cs, 4, 64))
    return p.with_capacity(p.bounds()) if payload else p


def test_render_decompositions_validate_rejections():
    from tracy_amd import capi
    lib = capi.lib()
    check = lambda p, mem=0: lib.tracyhip_render_decompositions_validate(C.byref(p.job), mem, C.byref(p.out))
    for form in dc.FORMS:
        assert check(_job(form)) == 0 and check(_job(form), 1) == 0 and check(_job(form, payload=False)) == 0 and check(_job(form, n=0)) == 0
    p = _job()
    assert lib.tracyhip_render_decompositions_validate(None, 0, C.byref(p.out)) == capi.ERR_ARG
    assert lib.tracyhip_render_decompositions_validate(C.byref(p.job), 0, None) == capi.ERR_ARG
    assert check(p, 2) == capi.ERR_ARG and b"mem" in lib.tracyhip_last_error()
    p.job.form = 3
    assert check(p) == capi.ERR_ARG and b"form" in lib.tracyhip_last_error()
    for field, values in (("max_variants", ((1, True), (1024, True), (0, False), (1025, False))), ("max_text", ((2, True), (1 << 19, True), (1, False), ((1 << 19) + 1, False)))):
        for v, ok in values:
            p = _job()
            setattr(p.job, field, v)
            assert check(p) == (0 if ok else capi.ERR_RANGE), (field, v)
            p = _job(dc.DECOMP)  # (not read by the table)
            setattr(p.job, field, v)
            assert check(p) == 0
    p = _job()
    p.flat["dcp_rows"][1] = (1 << 22) + 1
    assert check(p) == capi.ERR_RANGE and b"trace 1" in lib.tracyhip_last_error()
    reads = {dc.DECOMP: ("dcp_indel", "dcp_err", "dcp_offset", "dcp_rows"),
             dc.VCF: ("bcpos", "estqual", "bc_offset", "bc_len", "var", "var_text", "var_n", "forward", "trim_left", "trim_right", "names")}
    reads[dc.JSON] = reads[dc.DECOMP] + reads[dc.VCF] + ("breakpoint", "indelshift")
    for form in dc.FORMS:
        for field, _ in capi.DcpTextJob._fields_:
            if field in ("n", "form", "qual_cut", "max_variants", "max_text"):
                continue
            arrays = isinstance(getattr(_job(form).job, field), C.Array)
            for k in (range(len(getattr(_job(form).job, field))) if arrays else (None,)):
                p = _job(form)
                if arrays:
                    getattr(p.job, field)[k] = None
                else:
                    setattr(p.job, field, None)
                needed = field in reads[form] or (arrays and (form == dc.JSON or (form == dc.VCF and field in ("chr_offset", "chr_len") and k == 0)))
                assert check(p) == (capi.ERR_ARG if needed else 0), (form, field, k)
    for field in ("dcp_indel", "bcpos", "var", "var_n"):
        p = _job()
        setattr(p.job, field, getattr(p.job, field) + 2)
        assert check(p) == capi.ERR_ARG and b"misaligned" in lib.tracyhip_last_error(), field
    for field in ("status", "text_len", "text_offset", "text_cap"):
        p = _job()
        setattr(p.out, field, None)
        assert check(p) == capi.ERR_ARG, field
    # the call itself answers the same before it looks for a device
    p = _job()
    p.job.max_variants = 0
    assert lib.tracyhip_render_decompositions(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_RANGE
    assert lib.tracyhip_render_decompositions_async(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG  # (a null context)
    st = capi.DcpTextStats()
    assert lib.tracyhip_last_dcptext_stats(None, C.byref(st)) == capi.ERR_ARG


def test_the_bound_covers_every_case():
    from tracy_amd import capi
    for name, c in dc.crafted():
        for form in dc.FORMS:
            assert bound(c, form) >= len(dc.expected(c, form)), (name, form)
    assert capi.dcptext_bound(3) == 0
    assert all(capi.dcptext_bound(f, 1 << 22, [1 << 22] * 3, [65535] * 2, [65535] * 2, 1024, 1 << 19) < 2 ** 31 for f in dc.FORMS)


# ---- dcptext_plan.h and the sinks of dcptext_wave.h as a program of its own, plain and under the sanitizers -----------------------------

PLAN_FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(PLAN_FLAGS))
def test_dcptext_plan_program(tmp_path, build):
    exe = tmp_path / ("dcptext_plan_" + build)
    # (-Wno-unknown-pragmas: the headers of the wave body, which the plan shares its descriptors with, may carry `#pragma unroll` for hipcc)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + PLAN_FLAGS[build] + ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "dcptext_plan.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "dcptext_plan: ok" in r.stdout
