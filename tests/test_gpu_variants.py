"""tracyhip_call_variants and tracyhip_decompose_variants (the variant calling of `tracy decompose -v` on the device) against
tests/indigo_oracle.py: the stage on the named cases of tests/variants_cases.py and random alignment pairs, the pipeline on a batch of
small traces carried through the oracle chain tests/test_gpu_cli.py spells out for the command line."""
import ctypes as C

import numpy as np
import pytest

import indigo_oracle as io
import pyoracle as orc
import variants_cases as vc
from decomp_cases import SC, make_case
from sage_oracle import revcomp

pytestmark = pytest.mark.gpu
TRIMS = (20, 20)
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


# ---- the stage ---------------------------------------------------------------------------------------------------------------------
def stage_cases():
    named = vc.named_cases()
    return [named[k] for k in sorted(named)] + vc.random_cases(64)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_stage_against_the_oracle(ctx, device):
    """every named case and 64 random pairs in one call.  What the header promises about the arrays: only the first var_n[t] records of
    a trace and the text they point to are written, in both kinds of memory -- the rest keeps the caller's bytes."""
    from tracy_amd import capi
    cases = stage_cases()
    nt = len(cases)
    rows, pos = [], []
    for c in cases:
        for a in (c["a"], c["b"]):
            rows.append((a[0], a[1])); pos.append(a[2])
    b = capi.VariantBuffers(nt, 128, 4096, device, fill=GUARD)
    got, flags = ctx.call_variants(rows, pos, [c["forward"] for c in cases], [c["bc_len"] for c in cases], *vc.TRIMS, device=device, buffers=b)
    rec, text, n, _ = b.arrays()
    for t, c in enumerate(cases):
        want = vc.expected(c)[0]
        assert flags[t] == 0 and got[t] == want, (t, got[t], want)
        used = sum(len(v["ref"]) + len(v["alt"]) for v in want)
        assert (rec[t, len(want):].view(np.uint8) == GUARD).all() and (text[t, used:] == GUARD).all(), t
    assert sum(len(g) for g in got) > 400


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_stage_capacities(ctx, device):
    from tracy_amd import capi
    for name, c, max_variants, max_text, fits in vc.capacity_cases():
        b = capi.VariantBuffers(1, max_variants, max_text, device, fill=GUARD)
        got, flags = ctx.call_variants([c["a"][:2], c["b"][:2]], [c["a"][2], c["b"][2]], [c["forward"]], [c["bc_len"]], *vc.TRIMS, device=device, buffers=b)
        rec, text, n, _ = b.arrays()
        if fits:
            assert flags[0] == 0 and got[0] == vc.expected(c)[0], name
        else:  # flagged, empty, and nothing of the trace's regions written
            assert flags[0] == 1 and got[0] == [] and n[0] == 0, name
            assert (rec.view(np.uint8) == GUARD).all() and (text == GUARD).all(), name


def test_stage_argument_checks(ctx):
    from tracy_amd import capi
    lib = capi.lib()
    z = np.zeros(8, np.uint8)
    u64, u32, i32 = np.zeros(2, np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.int32)
    b = capi.VariantBuffers(1, 4, 16)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(max_variants=4, max_text=16, mem=0, var=b.struct.var, rows0=z):
        return lib.tracyhip_call_variants(ctx._h, C.c_uint32(1), p(rows0) if rows0 is not None else None, p(z), p(u64), p(u32), p(i32), p(z), p(u32),
                                          C.c_uint32(20), C.c_uint32(20), C.c_uint32(max_variants), C.c_uint32(max_text), mem, C.c_void_p(var),
                                          C.c_void_p(b.struct.text), C.c_void_p(b.struct.var_n), C.c_void_p(b.struct.var_flags))
    assert call() == 0
    assert call(max_variants=0) == capi.ERR_RANGE and call(max_variants=1025) == capi.ERR_RANGE and call(max_variants=1024, var=0) == capi.ERR_ARG
    assert "max_variants" in lib.tracyhip_last_error().decode() or "null" in lib.tracyhip_last_error().decode()
    assert call(max_text=1) == capi.ERR_RANGE and "max_text" in lib.tracyhip_last_error().decode()
    assert call(mem=2) == capi.ERR_ARG and call(rows0=None) == capi.ERR_ARG and call(var=0) == capi.ERR_ARG


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
def oracle_variants(w, ref, trims, slice_pos):
    """tests/test_gpu_cli.py:223-233 on arrays: (the sorted list, events of allele 1, events of allele 2 on its own), None for a failed trace"""
    if w["status"] != 0:
        return None
    forward = bool(w["forward"])
    refslice = ref if forward else revcomp(ref)
    var, per = [], []
    for k, seq in enumerate((io.trimmed_seq(w["primary"], *trims), io.trimmed_seq(w["secdecomp"], *trims))):
        sl = refslice[w["slice_begin%d" % k]:w["slice_begin%d" % k] + w["slice_len%d" % k]]
        if forward:
            r0, r1 = orc.create_alignment_str(w["btr%d" % k], seq, sl)
        else:
            rseq, rsl = revcomp(seq), revcomp(sl)
            _, btr = orc.gotoh_str(rseq, rsl, 1, 0, SC)
            r0, r1 = orc.create_alignment_str(btr, rseq, rsl)
        own = []
        io.call_variants(r0, r1, "chr", slice_pos + w["ref_pos%d" % k], own)
        per.append(len(own))
        io.call_variants(r0, r1, "chr", slice_pos + w["ref_pos%d" % k], var)
    io.sort_variants(var)
    nb = len(w["primary"])
    out = [dict(pos=v["pos"], basenum=v["basenum"], gt=v["gt"], ref=v["ref"].encode(), alt=v["alt"].encode(),
                call_index=(trims[0] + v["basenum"] - 1) if forward else nb - (trims[1] + v["basenum"])) for v in var]
    return out, per[0], per[1]


@pytest.fixture(scope="module")
def batch():
    """24 traces of about 250 basecalls against 500-base references: every second one reads the reverse strand, most carry a heterozygous
    indel and SNVs, one has a reference of 30 unrelated bases (status != 0).  The oracle chain runs once."""
    from tracy_amd import hostlib
    rng = np.random.default_rng(77)
    tr = []
    for i in range(24):
        c = make_case(300 + i, n=500, mf=250, kind=(1 if i % 6 == 5 else 0), frac1=(0.6, 0.55, 0.7)[i % 3], maxlen=12)
        ref = c["ref"]
        if i == 9:
            ref = bytes(rng.choice(list(b"ACGT"), size=30).tolist())  # far shorter than the trace: it cannot reach the score gate of indigo.h:303-309
        if i % 2:
            ref = revcomp(ref)
        slice_pos = 1000 * i + 7
        w = io.decompose_trace(c["sig"], c["bcpos"], c["pri"], c["sec"], ref, SC, *TRIMS)
        tr.append(dict(sig=c["sig"], pos=c["pos"], bcpos=c["bcpos"], pri=c["pri"], sec=c["sec"], ref=ref, slice_pos=slice_pos, w=w,
                       want=oracle_variants(w, ref, TRIMS, slice_pos),
                       prof=hostlib.create_profile(c["sig"], c["bcpos"], c["pri"], c["sec"], 0, 0)))
    status = [t["w"]["status"] for t in tr]
    assert status[9] != 0 and sum(s == 0 for s in status) >= 20
    good = [t for t in tr if t["want"] is not None]
    assert sum(1 for t in good if not t["w"]["forward"]) >= 8 and sum(1 for t in good if t["w"]["forward"]) >= 8
    assert sum(1 for t in good if any(len(v["ref"]) != len(v["alt"]) for v in t["want"][0])) >= 6  # indels
    assert sum(1 for t in good if any(len(v["ref"]) == len(v["alt"]) for v in t["want"][0])) >= 6  # SNVs
    return tr


def decompose(ctx, tr, device=False):
    from tracy_amd import capi
    refs = [t["ref"] for t in tr]
    if device:
        pb = capi.PreparedBasecall([t["sig"] for t in tr], [t["pos"] for t in tr], 0.33, 0, device=True).run(ctx)
        assert not pb.meta["status"].any()
        return ctx.decompose_traces(None, None, refs, SC, *TRIMS, device_bc=pb)
    hbc = capi.HostBaseCalls([t["sig"] for t in tr], [t["bcpos"] for t in tr], [t["pri"] for t in tr], [t["sec"] for t in tr])
    return ctx.decompose_traces([t["prof"] for t in tr], hbc, refs, SC, *TRIMS)


def check_lists(tr, got, flags):
    for i, t in enumerate(tr):
        assert flags[i] == 0, i
        assert got[i] == ([] if t["want"] is None else t["want"][0]), (i, got[i], t["want"])


def usable_reverse(tr):
    return sum(1 for t in tr if t["want"] is not None and not t["w"]["forward"])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pipeline_against_the_oracle_chain(ctx, batch, device):
    outcome = decompose(ctx, batch, device)
    assert [int(s) for s in outcome["status"][:24]] == [t["w"]["status"] for t in batch]
    sp = [t["slice_pos"] for t in batch]
    got, flags = ctx.decompose_variants(outcome, sp)
    check_lists(batch, got, flags)
    st = ctx.last_call_stats()
    nvar = sum(len(g) for g in got)
    assert st["traces"] == 24 and st["var_traces"] == sum(t["want"] is not None for t in batch) and st["var_truncated"] == 0 and st["var_chunks"] == 1
    assert st["var_realigned"] == usable_reverse(batch) > 0
    # the formula of the header, one chunk: the plan read and the end / the counts and the packed copy -- the issue's two per chunk
    want_syncs = (1 + 1) if device else (1 + (1 if nvar else 0))
    assert want_syncs == 2
    assert st["host_syncs"] == want_syncs
    # ... and it does not depend on the number of traces
    got8, flags8 = ctx.decompose_variants(decompose(ctx, batch[:8], device), sp[:8])
    check_lists(batch[:8], got8, flags8)
    assert ctx.last_call_stats()["host_syncs"] == want_syncs


def test_pipeline_in_several_chunks(ctx, batch):
    """a workspace limit that holds the rows of a few dozen traces (and the traceback planes of one re-alignment batch)"""
    tr = batch * 6
    outcome = decompose(ctx, tr)
    sp = [t["slice_pos"] for t in tr]
    ctx.set_workspace_limit(200 << 10)
    try:
        got, flags = ctx.decompose_variants(outcome, sp)
        st = ctx.last_call_stats()
    finally:
        ctx.set_workspace_limit(0)
    check_lists(tr, got, flags)
    nrev = usable_reverse(tr)
    assert st["var_chunks"] >= 3 and st["var_realigned"] == nrev
    assert st["host_syncs"] == (st["var_chunks"] - 1) + 2  # (every chunk of this batch holds reverse traces: one wait each before the last)
    assert st["host_syncs"] <= 2 * st["var_chunks"]
    one, flags1 = ctx.decompose_variants(outcome, sp)
    assert ctx.last_call_stats()["var_chunks"] == 1 and one == got


def test_pipeline_on_the_benchmark_shape(ctx):
    """1 kb traces against 3 kb windows at trims 50 / 50, as bench.py's decompose leg makes them: heterozygous indel + SNVs, a homozygous
    indel only, no variant at all; both strands"""
    from tracy_amd import capi, hostlib
    d = hostlib.synth_decompose_batch(5000, 30, 3000, 1000, 4, mix=1)
    pick = [18, 19, 21, 28, 29]
    tr = []
    for i in pick:
        sig, bcpos, pri, sec, ref = d["signal"][i], d["bcpos"][i], d["primary"][i].tobytes(), d["secondary"][i].tobytes(), d["refs"][i].tobytes()
        w = io.decompose_trace(sig, bcpos, pri, sec, ref, SC, 50, 50)
        tr.append(dict(sig=sig, bcpos=bcpos, pri=pri, sec=sec, ref=ref, w=w, want=oracle_variants(w, ref, (50, 50), 11 * i), slice_pos=11 * i,
                       prof=d["profiles"][i]))
    assert all(t["w"]["status"] == 0 for t in tr) and {bool(t["w"]["forward"]) for t in tr} == {True, False}
    assert {bool(t["w"]["bp"].indelshift) for t in tr} == {True, False}  # with and without a heterozygous indel
    hbc = capi.HostBaseCalls([t["sig"] for t in tr], [t["bcpos"] for t in tr], [t["pri"] for t in tr], [t["sec"] for t in tr])
    outcome = ctx.decompose_traces([t["prof"] for t in tr], hbc, [t["ref"] for t in tr], SC)
    got, flags = ctx.decompose_variants(outcome, [t["slice_pos"] for t in tr])
    check_lists(tr, got, flags)
    assert sum(len(g) for g in got) >= 4 and ctx.last_call_stats()["host_syncs"] == 2


def test_pipeline_all_failed_and_all_reverse(ctx, batch):
    """a batch in which no trace is called (no forward op string is staged, nothing is re-aligned), and one of reverse traces only"""
    bad = [dict(batch[9], slice_pos=5)] * 3
    got, flags = ctx.decompose_variants(decompose(ctx, bad), [5, 5, 5])
    st = ctx.last_call_stats()
    assert got == [[], [], []] and not flags.any() and st["var_traces"] == 0 and st["var_realigned"] == 0 and st["host_syncs"] == 1
    rev = [t for t in batch if t["want"] is not None and not t["w"]["forward"]]
    assert len(rev) >= 8
    got, flags = ctx.decompose_variants(decompose(ctx, rev), [t["slice_pos"] for t in rev])
    check_lists(rev, got, flags)
    st = ctx.last_call_stats()
    assert st["var_realigned"] == st["var_traces"] == len(rev) and st["host_syncs"] == 2


def test_pipeline_async(ctx, batch):
    from tracy_amd import capi
    outcome = decompose(ctx, batch)
    c = outcome.call
    sp = np.array([t["slice_pos"] for t in batch], np.uint32)
    b = capi.VariantBuffers(24, 256, 4096)
    ctx.decompose_variants_async(c["job"], c["out"], sp, c["prm"], b.struct, capi.MEM_HOST)
    sp[:] = 0  # (copied by the call)
    ctx.synchronize()
    check_lists(batch, *b.lists())


def test_truncation(ctx, batch):
    """max_variants = 2: flagged are exactly the traces with more than two events on either allele or after the merge; the others unchanged"""
    outcome = decompose(ctx, batch)
    got, flags = ctx.decompose_variants(outcome, [t["slice_pos"] for t in batch], max_variants=2, max_text=4096)
    over = []
    for i, t in enumerate(batch):
        if t["want"] is None:
            assert flags[i] == 0 and got[i] == []
            continue
        lst, n1, n2 = t["want"]
        big = n1 > 2 or n2 > 2 or len(lst) > 2
        over.append(big)
        assert flags[i] == (1 if big else 0), (i, n1, n2, len(lst))
        assert got[i] == ([] if big else lst), i
    assert any(over) and not all(over)
    assert ctx.last_call_stats()["var_truncated"] == sum(over)


def test_pipeline_refuses_memory_of_the_other_kind(ctx, batch):
    import torch
    from tracy_amd import capi
    outcome = decompose(ctx, batch[:4])
    c = outcome.call
    b = capi.VariantBuffers(4, 8, 64, device=True)  # device arrays, the call says host
    sp = np.zeros(4, np.uint32)
    rc = capi.lib().tracyhip_decompose_variants(ctx._h, C.byref(c["job"]), C.byref(c["out"]), capi._u32p(sp), C.byref(c["prm"]), capi.MEM_HOST,
                                                C.byref(b.struct))
    assert rc == capi.ERR_ARG and "device memory" in capi.lib().tracyhip_last_error().decode()
    del torch


# ---- the command line --------------------------------------------------------------------------------------------------------------
def _timers(stderr):
    line = [ln for ln in stderr.splitlines() if ln.startswith("timers:")]
    assert len(line) == 1, stderr[-800:]
    tok = line[0].split()
    return {tok[i]: tok[i + 1] for i in range(1, len(tok) - 1, 2)}


def test_command_line_batch_equals_per_file_and_oracle(tmp_path):
    """`decompose -v --batch` on six small traces, both strands: .vcf / .bcf / .json byte for byte what the per-file command writes, the
    variant list the oracle's; the run reports that the device path called the variants.  Then with capacities that send traces to the
    host code: the same bytes."""
    import os
    import subprocess
    from bcf_reader import read_bcf
    from test_gpu_cli import CLI, decompose_case, expected_decompose
    rows = []
    for i in range(6):
        t, r, _ = decompose_case(str(tmp_path), "v%d" % i, 6100 + i, n=900 + 60 * i, mf=300 + 20 * i, kind=(1 if i == 4 else 0), reverse=bool(i % 2))
        rows.append((t, r))
    exts = (".vcf", ".bcf", ".json")

    def batch(tag, caps=None):
        man = str(tmp_path / ("manifest_%s.tsv" % tag))
        pre = [str(tmp_path / ("%s%d" % (tag, i))) for i in range(6)]
        open(man, "w").write("".join("%s\t%s\t%s\n" % (t, r, p) for (t, r), p in zip(rows, pre)))
        env = dict(os.environ, TRACY_AMD_CLI_TIMERS="1")
        if caps:
            env["TRACY_AMD_CLI_VARIANT_CAPS"] = caps
        p = subprocess.run([CLI, "decompose", "-v", "--batch", man], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr[-800:]
        return pre, _timers(p.stderr)
    pre, tm = batch("dev")
    assert float(tm["var_traces"]) == 6 and float(tm["var_fallback"]) == 0
    nvar = 0
    for i, (t, r) in enumerate(rows):
        single = str(tmp_path / ("single%d" % i))
        p = subprocess.run([CLI, "decompose", "-v", "-r", r, "-o", single, t], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-800:]
        for ext in exts:
            assert open(pre[i] + ext, "rb").read() == open(single + ext, "rb").read(), (i, ext)
        files, rep, w = expected_decompose(t, r)
        assert open(pre[i] + ".json").read() == files[".json"], i
        recs = [ln.split("\t") for ln in open(pre[i] + ".vcf").read().split("\n") if ln and not ln.startswith("#")]
        assert [(x[0], int(x[1]), x[3], x[4], x[9].split(":")[0]) for x in recs] == \
               [(v["chr"], v["pos"], v["ref"], v["alt"], {1: "0/1", 2: "1/1"}[v["gt"]]) for v in rep["var"]], i
        _, brecs, _ = read_bcf(pre[i] + ".bcf")
        assert [(b["CHROM"], b["POS"], b["REF"], b["ALT"]) for b in brecs] == [(x[0], int(x[1]), x[3], x[4]) for x in recs], i
        nvar += len(recs)
        assert bool(w["forward"]) == (i % 2 == 0)
    assert nvar >= 6
    pre2, tm2 = batch("host", caps="1,2")  # one record, two bytes: every trace with two events goes to the host code
    assert float(tm2["var_fallback"]) >= 3 and float(tm2["var_traces"]) + float(tm2["var_fallback"]) == 6
    for i in range(6):
        for ext in exts:
            assert open(pre[i] + ext, "rb").read() == open(pre2[i] + ext, "rb").read(), (i, ext)
