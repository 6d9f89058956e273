"""The alignment printing bodies (tracy_amd/csrc/alntext_wave.h: letters, count, scan and emit of the plot, the FASTA and the JSON tail) on
the 64-fiber host wave, tile after tile: the text against the host writers (hostlib.alntext_batch) and the independent restatement of
tests/alntext_cases.py -- equality of bytes, the buffer filled with a sentinel and checked untouched in front of and behind the text, at
every alignment of its first byte.  Plus the reference slice body, the argument checks and the bound of tracyhip_render_alignments, the
range check of tracyhip_reference_slices and the stand-alone program over alntext_plan.h, which need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alntext_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENT = 0x7e


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_alntext.so")
    srcs = [os.path.join(HERE, "emu", "emu_alntext.cpp"), os.path.join(HERE, "emu", "host_wave.h")]
    srcs += [os.path.join(ROOT, "tracy_amd/csrc", f) for f in ("alntext_wave.h", "alntext_plan.h", "render_wave.h", "ragged_plan.h", "dp_lane.h")]
    srcs.append(os.path.join(ROOT, "include", "tracy_hip.h"))
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], stderr=subprocess.DEVNULL)
    lib = C.CDLL(so)
    lib.emu_alntext_tile.restype = lib.emu_alntext_max_item.restype = lib.emu_slice_tile.restype = C.c_uint32
    return lib


def run(emu, c, form, key=0, L=60, shift=0, cap=None, sizes_only=False):
    """one alignment through the bodies; the text starts `shift` bytes into a 16-byte aligned buffer of sentinels"""
    from tracy_amd import capi
    arr = lambda b: np.frombuffer(bytes(b) + b"\0", np.uint8).copy()
    r0, r1, names = arr(c["row0"]), arr(c["row1"]), arr(c["name0"] + c["name1"])
    cols = len(c["row0"])
    room = capi.alntext_bound(form, L, cols, len(c["name0"]), len(c["name1"])) + 8 if cap is None else cap
    raw = np.full(shift + room + 64 + 16, SENT, np.uint8)
    lead = (-raw.ctypes.data) % 16  # the first byte of `buf` is 16-byte aligned: `shift` is the alignment of the text
    buf = raw[lead:lead + shift + room + 48]
    out = (C.c_int32 * 2)()
    r = emu.emu_alntext(C.c_uint32(form), C.c_uint32(key), C.c_uint32(L), C.c_void_p(r0.ctypes.data), C.c_void_p(r1.ctypes.data), C.c_uint32(cols),
                        C.c_void_p(names.ctypes.data), C.c_uint32(len(c["name0"])), C.c_uint32(len(c["name1"])), C.c_int32(c["pos"]),
                        C.c_uint32(c["reflen"]), C.c_uint8(c["forward"]), C.c_int32(c["score"]), None if sizes_only else C.c_void_p(buf.ctypes.data),
                        C.c_uint64(shift), C.c_uint64(room), out)
    assert r == 0, {1: "an item longer than the LDS image allows", 2: "a body wrote past the tile scratch", 3: "the job was refused"}[r]
    status, ln = out[0], out[1]
    wrote = ln if (status == ac.OK and not sizes_only) else 0
    return dict(status=status, text_len=ln, text=buf[shift:shift + wrote].tobytes(),
                untouched=bool((raw[:lead + shift] == SENT).all() and (raw[lead + shift + wrote:] == SENT).all()))


def host_texts(items, form):
    """hostlib.alntext_batch over a list of (name, key, linelimit, alignment): one call per (key, linelimit); the texts in the list's order"""
    from tracy_amd import hostlib
    texts = {}
    for (key, L), group in ac.jobs(items).items():
        res = hostlib.alntext_batch(hostlib.alntext_pack(**ac.pack([c for _, c in group])), form, key, L, 2)
        for (name, _), h in zip(group, res):
            assert h["status"] == ac.OK, (name, "host")
            texts[name] = h["text"]
    return [texts[name] for name, _, _, _ in items]


def test_the_tile_is_what_the_cases_assume(emu):
    assert emu.emu_alntext_tile() == ac.TILE and emu.emu_alntext_max_item() >= 38


@pytest.mark.parametrize("form", ac.FORMS)
def test_crafted_cases_against_the_host_writers_and_the_restatement(emu, form):
    from tracy_amd import capi
    items = ac.crafted()
    names = [n for n, _, _, _ in items]
    assert len(set(names)) == len(names)
    for i, ((name, key, L, c), h) in enumerate(zip(items, host_texts(items, form))):
        want = ac.expected(c, form, key, L)
        assert not ac.is_deferred(c, form, key), name
        assert h == want, (name, "host")
        g = run(emu, c, form, key, L, shift=i % 16)
        assert g["status"] == ac.OK and g["text_len"] == len(want), name
        assert g["text"] == want, name
        assert g["untouched"], name
        assert len(want) <= capi.alntext_bound(form, L, len(c["row0"]), len(c["name0"]), len(c["name1"])), name


@pytest.mark.parametrize("form", ac.FORMS)
def test_every_alignment_of_the_first_byte_and_short_texts(emu, form):
    """texts shorter than one 16-byte word, texts that end on a word boundary, every head and tail"""
    cases = {n: (k, L, c) for n, k, L, c in ac.crafted()}
    for name in ("cols0", "cols1", "cols65", "line7_cols+1", "pos_crosses_setw9"):
        key, L, c = cases[name]
        want = ac.expected(c, form, key, L)
        for shift in range(16):
            g = run(emu, c, form, key, L, shift=shift)
            assert (g["status"], g["text"]) == (ac.OK, want), (name, shift)
            assert g["untouched"], (name, shift)


def test_the_cases_hit_what_they_are_named_for(emu):
    cases = {n: (k, L, c) for n, k, L, c in ac.crafted()}
    text = lambda name: ac.expected(cases[name][2], ac.PLOT, cases[name][0], cases[name][1])
    t = text("counters_1_to_1100")
    for a, b in ((9, 10), (99, 100), (999, 1000)):
        assert b"Alt%10d " % a in t and b"Alt%10d " % b in t and b"Ref%10d " % b in t
    # linelimit 1: nine items per block, so block 256 opens tile 9 of the blocks
    assert 9 * 256 % ac.TILE == 0
    assert re.findall(rb"^Ref +(\d+) ", text("counter_1000_at_a_tile_start"), re.M)[256] == b"1000"
    assert re.findall(rb"^Alt1 +(\d+) ", text("counter_10_at_a_tile_start"), re.M)[256] == b"10"
    assert text("counter_1000_at_a_block_start").count(b"Ref      1000 ") == 1 and text("counter_100_at_a_block_start").count(b"Ref       100 ") == 1
    t = text("mirrored_120_to_1")
    assert b"Ref       100 " in t and b"Ref        99 " in t and b"Ref        10 " in t and b"Ref         9 " in t and t.index(b"Ref       100 ") < t.index(b"Ref        99 ")
    assert b"Ref1000000001 " in text("pos_fills_setw10") and b"Alt21000000001 " in text("pos_overflows_setw9")
    t = text("pos_crosses_setw9")
    assert b"Alt2999999981 " in t and b"Alt21000000002 " in t
    assert b"score: -2147483648\n" in text("score-2147483648") and b"score: 0\n" in text("score0")
    for blocks, spacer in ((5, 4), (6, 0), (7, 0)):
        t = text("blocks%d" % blocks)
        assert len(re.findall(rb"^Ref ", t, re.M)) == blocks and t.endswith(b"\n\n" + b"\n" * spacer + (b"#" + b"-" * 23 + b"\n") * 2 + b"\n\n")
    fald = 21
    for k in (0, fald - 1, fald, fald + 1, 2 * fald):
        c = cases["letters%d" % k][2]
        t = text("letters%d" % k)
        body = t[len(c["name0"]) + 1:t.index(c["name1"])]
        assert body.count(b"\n") == (k + fald - 1) // fald and len(body) == k + body.count(b"\n")
    assert set(cases["row0_gaps_only"][2]["row0"]) == {0x2d} and text("row0_gaps_only").startswith(b">Alt\n>Ref")
    for byte in (b"\"", b"\\", b"\x80", b"\x00"):
        assert byte in cases["row_bytes"][2]["row0"]
    assert max(len(c["row0"]) for _, _, _, c in ac.crafted()) > 64 * ac.TILE  # more column tiles in front of an anchor than a wave sums in one step


def test_the_deferred_family(emu):
    items = ac.deferred()
    for form in ac.FORMS:
        for (name, key, L, c), h in zip(items, host_texts(items, form)):
            assert h == ac.expected(c, form, key, L), (name, "host")  # the host writers print what the device leaves to them
            if not ac.is_deferred(c, form, key):  # (the mirrored check is the plot's, name0 is not the JSON tail's)
                assert (name.startswith("mirrored") and form != ac.PLOT) or (name == "name0_over" and form == ac.JSON)
                g = run(emu, c, form, key, L, shift=3)
                assert (g["status"], g["text"]) == (ac.OK, h) and g["untouched"], name
                continue
            if name == "cols_over" and form != ac.PLOT:
                continue  # (one form is enough for four million columns)
            g = run(emu, c, form, key, L, shift=3, cap=64)
            assert (g["status"], g["text_len"]) == (ac.DEFERRED, 0), name
            assert g["untouched"], name
            g = run(emu, c, form, key, L, sizes_only=True)
            assert (g["status"], g["text_len"]) == (ac.DEFERRED, 0), name
    assert all(ac.is_deferred(c, ac.PLOT, key) for _, key, _, c in items)


def test_sizes_only_and_too_small(emu):
    cases = {n: (k, L, c) for n, k, L, c in ac.crafted()}
    for form in ac.FORMS:
        for name in ("cols65", "line7", "key3_forward0"):
            key, L, c = cases[name]
            want = ac.expected(c, form, key, L)
            g = run(emu, c, form, key, L, sizes_only=True)
            assert (g["status"], g["text_len"]) == (ac.OK, len(want)) and g["untouched"], name
            g = run(emu, c, form, key, L, shift=7, cap=len(want))  # exactly enough
            assert (g["status"], g["text"]) == (ac.OK, want) and g["untouched"], name
            g = run(emu, c, form, key, L, shift=7, cap=len(want) - 1)
            assert (g["status"], g["text_len"]) == (ac.TOO_SMALL, len(want)) and g["untouched"], name


@pytest.mark.parametrize("form", ac.FORMS)
def test_200_random_alignments(emu, form):
    items = ac.random_cases()
    assert len(items) == 200 and max(len(c["row0"]) for _, _, _, c in items) <= 600
    if True:
        for i, ((name, key, L, c), h) in enumerate(zip(items, host_texts(items, form))):
            want = ac.expected(c, form, key, L)
            assert h == want, (name, form, "host")
            g = run(emu, c, form, key, L, shift=i % 16)
            if ac.is_deferred(c, form, key):
                assert (g["status"], g["text_len"]) == (ac.DEFERRED, 0) and g["untouched"], (name, form)
            else:
                assert (g["status"], g["text"]) == (ac.OK, want) and g["untouched"], (name, form)


# ---- the reference slice body -------------------------------------------------------------------------------------------------------


def test_slices_on_the_host_wave(emu):
    rng = np.random.default_rng(3)
    T = emu.emu_slice_tile()
    alphabet = np.frombuffer(b"ACGTNacgtnRYKMxz-*\x00\x80\xff", np.uint8)
    for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17):
        ref = alphabet[rng.integers(0, len(alphabet), n)].tobytes()
        rc = ac.revcomp_rule(ref)
        for begin, ln in ((0, n), (0, 0), (n, 0), (n // 2, n - n // 2), (1, n - 1), (n // 3, n // 3)):
            for fw, oriented in ((1, ref), (0, rc)):
                src = np.frombuffer(ref + b"\0", np.uint8).copy()
                out = np.full(ln + 32, SENT, np.uint8)
                emu.emu_slice(C.c_void_p(src.ctypes.data), C.c_uint32(n), C.c_uint8(fw), C.c_uint32(begin), C.c_uint32(ln), C.c_void_p(out.ctypes.data + 16))
                assert out[16:16 + ln].tobytes() == oriented[begin:begin + ln], (n, begin, ln, fw)
                assert (out[:16] == SENT).all() and (out[16 + ln:] == SENT).all()


# ---- tracyhip_render_alignments_validate / _bound, tracyhip_reference_slices_validate: what needs no device --------------------------


def _job(n=3, payload=True, form=ac.PLOT, key=0, L=60):
    from tracy_amd import capi
    cs = [c for _, _, _, c in ac.crafted()[:n]]
    p = capi.PreparedAlnText(form, key=key, linelimit=L, **ac.pack(cs))
    return p.with_capacity(p.bounds()) if payload else p


def test_render_alignments_validate_rejections():
    from tracy_amd import capi
    lib = capi.lib()
    check = lambda p, mem=0: lib.tracyhip_render_alignments_validate(C.byref(p.job), mem, C.byref(p.out))
    assert check(_job()) == 0 and check(_job(), 1) == 0 and check(_job(payload=False)) == 0 and check(_job(0)) == 0
    for form in ac.FORMS:
        assert check(_job(form=form)) == 0
    p = _job()
    assert lib.tracyhip_render_alignments_validate(None, 0, C.byref(p.out)) == capi.ERR_ARG
    assert lib.tracyhip_render_alignments_validate(C.byref(p.job), 0, None) == capi.ERR_ARG
    assert check(p, 2) == capi.ERR_ARG and b"mem" in lib.tracyhip_last_error()
    p.job.form = 3
    assert check(p) == capi.ERR_ARG and b"form" in lib.tracyhip_last_error()
    for key, ok in ((3, True), (4, False)):
        p = _job()
        p.job.key = key
        assert (check(p) == 0) == ok
    assert b"key" in lib.tracyhip_last_error()
    for L, ok in ((0, False), (1, True), (65535, True), (65536, False)):
        p = _job()
        p.job.linelimit = L
        assert (check(p) == 0) == ok, L
    assert b"linelimit" in lib.tracyhip_last_error()
    p = _job(form=ac.FASTA)  # key and linelimit are the plot's
    p.job.key, p.job.linelimit = 9, 0
    assert check(p) == 0
    for field in ("rows0", "rows1", "rows_offset", "cols", "names", "name0_offset", "name0_len", "name1_offset", "name1_len", "ref_pos", "ref_len",
                  "forward", "score"):
        for payload in (True, False):  # the sizes-only form reads the same arrays
            p = _job(payload=payload)
            setattr(p.job, field, None)
            assert check(p) == capi.ERR_ARG, field
    for field in ("name0_offset", "name0_len", "score"):  # not read by the JSON tail
        p = _job(form=ac.JSON)
        setattr(p.job, field, None)
        assert check(p) == 0, field
    p = _job(form=ac.FASTA)
    p.job.score = None
    assert check(p) == 0
    for field in ("status", "text_len", "text_offset", "text_cap"):
        p = _job()
        setattr(p.out, field, None)
        assert check(p) == capi.ERR_ARG, field
    # the call itself answers the same before it looks for a device
    p = _job()
    p.job.key = 4
    assert lib.tracyhip_render_alignments(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG
    assert lib.tracyhip_render_alignments_async(None, C.byref(p.job), 0, C.byref(p.out)) == capi.ERR_ARG


def test_the_bound_covers_every_case():
    from tracy_amd import capi
    for name, key, L, c in ac.crafted() + ac.random_cases(60, seed=11):
        for form in ac.FORMS:
            b = capi.alntext_bound(form, L, len(c["row0"]), len(c["name0"]), len(c["name1"]))
            assert b >= len(ac.expected(c, form, key, L)), (name, form)
    assert capi.alntext_bound(3, 60, 10, 1, 1) == 0 and capi.alntext_bound(ac.PLOT, 0, 10, 1, 1) == 0
    assert all(capi.alntext_bound(f, L, 1 << 22, 65535, 65535) < 2 ** 31 for f in ac.FORMS for L in (1, 60, 65535))


def test_reference_slices_refusals():
    from tracy_amd import capi
    lib = capi.lib()
    refs = [b"ACGTACGTAC", b"TTTT"]
    ok = capi.PreparedSlices(refs, [1, 0], [2, 0], [8, 4])
    assert ok.validate() == 0
    p = capi.PreparedSlices(refs, [1, 0], [3, 0], [8, 4])  # 3 + 8 > 10
    assert p.validate() == capi.ERR_RANGE and b"beyond the reference" in lib.tracyhip_last_error() and b"slice 0" in lib.tracyhip_last_error()
    p = capi.PreparedSlices(refs, [1, 0], [2, 1], [8, 4])
    assert p.validate() == capi.ERR_RANGE and b"slice 1" in lib.tracyhip_last_error()
    p = capi.PreparedSlices(refs, [1, 0, 1], [0, 0, 0], [1, 1, 1])  # identity: no third reference
    assert p.validate() == capi.ERR_ARG
    p = capi.PreparedSlices(refs, [1, 0, 1], [0, 0, 9], [1, 1, 1], ref_index=[1, 1, 0])
    assert p.validate() == 0
    p = capi.PreparedSlices(refs, [1, 0, 1], [0, 0, 9], [1, 1, 2], ref_index=[1, 1, 0])
    assert p.validate() == capi.ERR_RANGE
    p = capi.PreparedSlices(refs, [1], [0], [1], ref_index=[2])
    assert p.validate() == capi.ERR_ARG and b"index" in lib.tracyhip_last_error()
    p = capi.PreparedSlices(refs, [1, 0], [2, 0], [8, 4])
    p.job.refs.kind = capi.SEQ_PROFILE
    assert p.validate() == capi.ERR_ARG and b"CHAR" in lib.tracyhip_last_error()
    for field in ("forward", "slice_begin", "slice_len"):
        p = capi.PreparedSlices(refs, [1, 0], [2, 0], [8, 4])
        setattr(p.job, field, None)
        assert p.validate() == capi.ERR_ARG, field
    p = capi.PreparedSlices(refs, [1, 0], [2, 0], [8, 4])
    assert lib.tracyhip_reference_slices_validate(C.byref(p.job), 0, None, capi._u64p(p.out_offset)) == capi.ERR_ARG
    assert lib.tracyhip_reference_slices_validate(C.byref(p.job), 2, C.c_void_p(p.out_ptr()), capi._u64p(p.out_offset)) == capi.ERR_ARG
    # the call itself answers the same before it looks for a device
    bad = capi.PreparedSlices(refs, [1, 0], [3, 0], [8, 4])
    assert lib.tracyhip_reference_slices(None, C.byref(bad.job), 0, C.c_void_p(bad.out_ptr()), capi._u64p(bad.out_offset)) == capi.ERR_RANGE


# ---- alntext_plan.h and the sinks of alntext_wave.h as a program of its own, plain and under the sanitizers ----------------------------

PLAN_FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(PLAN_FLAGS))
def test_alntext_plan_program(tmp_path, build):
    exe = tmp_path / ("alntext_plan_" + build)
    # (-Wno-unknown-pragmas: the headers of the wave body, which the plan shares its descriptors with, may carry `#pragma unroll` for hipcc)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + PLAN_FLAGS[build] + ["-o", str(exe), os.path.join(ROOT, "tests", "cpp", "alntext_plan.cpp")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "alntext_plan: ok" in r.stdout
