"""Device trace padding (tracyhip_pad_traces) against the restatements of assemble_oracle.py / sage_oracle.py and the host chain
(hostlib.pad_batch): every field of every trace, exact; host and device buffers, int16 and int32 samples, partial workgroups, deferred
traces between answered ones, staging in several chunks, the queued call, and the two chains -- signals -> basecalls -> alignment rows ->
gapped chromatograms without a payload on the host, and the rows of an assembled group taken by offset."""
import ctypes as C

import numpy as np
import pytest

import pad_cases as pc

pytestmark = pytest.mark.gpu

SCORE = (3, -5, -10, -4)
SENT = 0x7e


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def answered():
    """the crafted set and 300 random traces with what the oracle gives for them, computed once"""
    cases = pc.crafted() + [("random%d" % s, pc.random_small(s)) for s in range(300)]
    return [(name, c, pc.expected(c)) for name, c in cases]


def prepared(cases, device, int16=False):
    from tracy_amd import capi
    sigs = [c["sig"].astype(np.int16) if int16 else c["sig"] for c in cases]
    bc = [dict(bcpos=c["bcpos"], primary=c["pri"], secondary=c["sec"], consensus=c["con"], estqual=c["q"]) for c in cases]
    return capi.PreparedPad(sigs, bc, [c["row"] for c in cases], [c["l"] for c in cases], [c["r"] for c in cases], [c["reverse"] for c in cases],
                            device=device)


def run_checked(ctx, cases, device, int16=False, asynchronous=False, slack=3):
    """sizes-only call, buffers of those sizes plus `slack` elements per trace filled with a sentinel, the call; asserts that nothing past
    the reported sizes was written.  Returns (PreparedPad, per-trace results without host fill-in)"""
    p = prepared(cases, device, int16)
    nso, nco = p.sizes(ctx)
    p.with_capacity(nso + slack, nco + slack, fill=SENT).run(ctx, asynchronous)
    if asynchronous:
        ctx.synchronize()
    o = p.host_arrays()
    sent_sig = np.array([SENT], np.uint8).astype(o["signal"].dtype)[0]
    for t in range(p.nt):
        ok = int(o["status"][t]) == pc.OK
        ks, kc = (4 * int(o["nsamples_out"][t]), int(o["ncalls_out"][t])) if ok else (0, 0)
        so, co = int(o["sample_offset"][t]), int(o["call_offset"][t])
        assert (o["signal"][so + ks:int(o["sample_offset"][t + 1])] == sent_sig).all(), t
        for k in ("primary", "secondary", "consensus", "estqual"):
            assert (o[k][co + kc:int(o["call_offset"][t + 1])] == SENT).all(), (t, k)
        assert (o["bcpos"][co + kc:int(o["call_offset"][t + 1])] == SENT).all(), t
    return p, p.results(fill_deferred=False)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("int16", [False, True])
def test_every_field_equals_the_oracle_and_the_host_chain(ctx, answered, device, int16):
    from tracy_amd import hostlib
    cases = [c for _, c, _ in answered]
    p, rows = run_checked(ctx, cases, device, int16)
    st = ctx.last_call_stats()
    assert (st["pad_deferred"], st["pad_too_small"], st["pad_chunks"]) == (0, 0, 1)
    if device:
        assert st["host_syncs"] == 1  # one synchronisation per call with device payloads
    host = hostlib.pad_batch(p.host_flat(), 4)
    for (name, c, want), got, h in zip(answered, rows, host):
        pc.compare(got, want, name)  # status OK: none of these is deferred
        pc.compare(h, want, (name, "host"))


@pytest.mark.parametrize("nt", [1, 3, 4, 5])
def test_partial_workgroups(ctx, answered, nt):
    pick = answered[20:20 + nt]
    for device in (False, True):
        _, rows = run_checked(ctx, [c for _, c, _ in pick], device)
        for (name, _, want), got in zip(pick, rows):
            pc.compare(got, want, (name, nt, device))


def test_deferred_between_answered_and_the_host_fill_in(ctx):
    items = pc.mixed_batch()
    cases = [c for _, c, _ in items]
    for device in (False, True):
        p, rows = run_checked(ctx, cases, device)
        st = ctx.last_call_stats()
        assert st["pad_deferred"] == sum(1 for _, _, ok in items if not ok) > 5 and st["pad_too_small"] == 0
        for (name, c, ok), got in zip(items, rows):
            if ok:
                pc.compare(got, pc.expected(c), (name, device))
            else:
                assert (got["status"], got["nsamples_out"], got["ncalls_out"]) == (pc.DEFERRED, 0, 0), name
        # the reference's loops cannot run these either: the fill-in leaves them deferred
        filled = p.results(fill_deferred=True)
        for (name, c, ok), got in zip(items, filled):
            if ok:
                pc.compare(got, pc.expected(c), (name, device, "filled"))
            else:
                assert got["status"] == pc.DEFERRED and got.get("unreadable"), name


def test_fill_deferred_runs_the_host_chain_where_it_can(ctx):
    """more calls than the device answers, nothing wrong otherwise: deferred, then answered by hostlib.pad_batch"""
    big = dict(pc.deferred())["too_many_calls"]
    small = dict(pc.crafted())["apart"]
    from tracy_amd import capi
    p = prepared([small, big, small], device=True)
    p.with_capacity(*p.sizes(ctx)).run(ctx)
    assert p.meta["status"][:3].tolist() == [pc.OK, pc.DEFERRED, pc.OK]
    rows = p.results(fill_deferred=True)
    for got, c in zip(rows, (small, big, small)):
        pc.compare(got, pc.expected(c), "fill")
    assert capi.PAD_DEFERRED == pc.DEFERRED


def test_too_small_reports_the_sizes_and_writes_nothing(ctx, answered):
    pick = answered[:12]
    cases = [c for _, c, _ in pick]
    for device in (False, True):
        p = prepared(cases, device)
        nso, nco = p.sizes(ctx)
        scap, ccap = nso.copy(), nco.copy()
        scap[2] -= 1
        ccap[5] -= 1
        p.with_capacity(scap, ccap, fill=SENT).run(ctx)
        assert ctx.last_call_stats()["pad_too_small"] == 2
        o = p.host_arrays()
        for t, (name, _, want) in enumerate(pick):
            assert (int(o["nsamples_out"][t]), int(o["ncalls_out"][t])) == (want["signal"].shape[1], len(want["bcPos"])), name
            if t in (2, 5):
                assert int(o["status"][t]) == pc.TOO_SMALL
                assert (o["signal"][int(o["sample_offset"][t]):int(o["sample_offset"][t + 1])] == SENT).all()
                assert (o["primary"][int(o["call_offset"][t]):int(o["call_offset"][t + 1])] == SENT).all()
            else:
                pc.compare(p.results(False)[t], want, name)


def test_host_staging_in_several_chunks(ctx, answered):
    pick = answered[:120]
    cases = [c for _, c, _ in pick]
    ctx.set_workspace_limit(64 << 10)
    try:
        p, rows = run_checked(ctx, cases, device=False)
        st = ctx.last_call_stats()
    finally:
        ctx.set_workspace_limit(0)
    assert st["pad_chunks"] > 1
    for (name, _, want), got in zip(pick, rows):
        pc.compare(got, want, name)
    _, one = run_checked(ctx, cases, device=False)
    assert ctx.last_call_stats()["pad_chunks"] == 1
    for a, b in zip(rows, one):
        assert np.array_equal(a["signal"], b["signal"]) and np.array_equal(a["bcPos"], b["bcPos"]) and a["primary"] == b["primary"]


def test_device_payloads_in_several_chunks(ctx, answered):
    """A device call stages nothing: the insert scratch of its rows alone cuts it, and only in the call with payloads.  The launches of
    all chunks follow each other over their slices of one descriptor buffer, and the results of all of them come back behind the last
    launch, in the one wait of the call."""
    from tracy_amd import hostlib
    pick = answered[20:28]  # (the crafted rows with inserts: 1 KB of scratch holds some of them in pairs, none of them all)
    cases = [c for _, c, _ in pick]
    ctx.set_workspace_limit(1 << 10)
    try:
        p, rows = run_checked(ctx, cases, device=True)
        st = ctx.last_call_stats()
    finally:
        ctx.set_workspace_limit(0)
    assert 3 <= st["pad_chunks"] < len(cases)
    assert (st["pad_deferred"], st["pad_too_small"]) == (0, 0)  # a deferral cannot hide a failure
    assert st["host_syncs"] == 1  # as measured on the commit before the drivers shared one chunk loop: one wait, however many chunks
    _, whole = run_checked(ctx, cases, device=True)
    assert ctx.last_call_stats()["pad_chunks"] == 1
    host = hostlib.pad_batch(p.host_flat(), 4)
    for (name, _, want), got, one, h in zip(pick, rows, whole, host):
        pc.compare(got, want, (name, "chunks"))
        pc.compare(one, want, (name, "whole"))
        pc.compare(h, want, (name, "host"))


def _synth(seed, mf):
    from tracy_amd import hostlib
    ref, sig, pos, _ = hostlib.synth_decompose(seed, mf + 400, mf, 30, seed % 4, 0.6)
    return ref, sig, pos


def test_queued_behind_basecalling_on_one_context(ctx, answered):
    from tracy_amd import capi
    data = [_synth(900 + i, 150) for i in range(4)]
    pb = capi.PreparedBasecall([s for _, s, _ in data], [p for _, _, p in data], 0.33, 0, device=True)
    pick = answered[:40]
    pp = prepared([c for _, c, _ in pick], device=True)
    pp.with_capacity(*pp.sizes(ctx))
    pb.run(ctx, asynchronous=True)
    pp.run(ctx, asynchronous=True)
    ctx.synchronize()
    assert not pb.meta["status"][:4].any() and pb.meta["bc_len"][:4].min() > 100
    for (name, _, want), got in zip(pick, pp.results(False)):
        pc.compare(got, want, name)


def test_chain_signals_to_gapped_chromatograms_on_the_device(ctx):
    """basecall_traces(device=True) -> the rows of an alignment of the profiles -> pad_traces(device_bc=...): the chromatograms and
    basecalls never leave the device between the calls"""
    import torch
    from tracy_amd import hostlib
    import sage_oracle as so
    data = [_synth(700 + i, 200) for i in range(8)]
    pb = ctx.basecall_traces([s for _, s, _ in data], [p for _, _, p in data], 0.33, 0, device=True)
    assert not pb.meta["status"][:8].any()
    profs, calls = [], []
    for _, sig, pos in data:  # (the host chain's profiles: the rows below are the alignment's, whoever computed its inputs)
        pri, sec, con, bcpos, q = hostlib.basecall_qual(sig, pos, 0.33)
        profs.append(hostlib.create_profile(sig, bcpos, pri, sec))
        calls.append((pri, sec, con, bcpos, q))
    _, _, rws = ctx.align(profs, [r for r, _, _ in data], SCORE + (1, 0), rows=True)
    rows0 = [r0 for r0, _ in rws]
    row_len = np.array([len(r) for r in rows0], np.uint32)
    row_off = np.zeros(8, np.uint64)
    row_off[1:] = np.cumsum(row_len.astype(np.uint64) + 5)[:-1]  # (rows of a result array: not back to back)
    blob = np.full(int(row_off[-1]) + int(row_len[-1]) + 5, ord("#"), np.uint8)
    for o, r in zip(row_off, rows0):
        blob[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    d_rows = torch.from_numpy(blob).cuda()
    pp = ctx.pad_traces(None, None, (d_rows, row_off, row_len), device_bc=pb)
    st = ctx.last_call_stats()
    assert st["host_syncs"] == 1 and st["pad_deferred"] == 0
    got = pp.results(fill_deferred=False)
    host = hostlib.pad_batch(pp.host_flat(), 2)
    for t, (_, sig, _) in enumerate(data):
        pri, sec, con, bcpos, q = calls[t]
        p = so.alignment_trace_padding(rows0[t], sig, bcpos.tolist(), pri, sec, con, q.tolist())
        want = dict(signal=np.asarray(p["signal"], np.int64), bcPos=np.asarray(p["bcPos"], np.int64), primary=bytes(p["primary"]),
                    secondary=bytes(p["secondary"]), consensus=bytes(p["consensus"]), estQual=np.asarray(p["estQual"], np.int64),
                    leadingGaps=p["leadingGaps"], trailingGaps=p["trailingGaps"], step=got[t]["step"])
        pc.compare(got[t], want, t)
        pc.compare(host[t], want, (t, "host"))
        assert got[t]["step"] == host[t]["step"]


def test_chain_rows_of_assembled_groups_by_offset(ctx):
    """2 groups x 3 traces, one of each reversed, with -t trims, through assemble_traces: every trace padded along its row of the group's
    `rows`, addressed by rows_offset[g] + r * ncol, against assemble_oracle's chain"""
    import torch
    from tracy_amd import capi, hostlib
    import pyoracle as orc
    import sage_oracle as so
    groups, refs, traces = [], [], []
    for g in range(2):
        ref, sig, pos = _synth(500 + g, 150)
        ns = sig.shape[1]
        variants = [(sig, pos), (sig, pos[12:]), (np.ascontiguousarray(sig[::-1, ::-1]), (ns - 1 - pos[::-1]).astype(np.int32))]
        grp = []
        for s, p in variants:
            pri, sec, con, bcpos, q = hostlib.basecall_qual(s, p, 0.33)
            tl, tr = so.trim_trace(2, sec, bcpos.tolist())
            assert tl + tr < len(pri)
            t = dict(sig=s, bcpos=bcpos.tolist(), pri=pri, sec=sec, con=con, q=q.tolist(), l=tl, r=tr)
            traces.append(t)
            grp.append(orc.create_profile_trace(s, bcpos, pri, sec, tl, tr))
        groups.append(grp)
        refs.append(orc.create_profile_str(ref))
    pa = capi.PreparedAssemble(groups, refs, SCORE)
    capi._check(capi.lib().tracyhip_assemble_traces(ctx._h, C.byref(pa.job), C.byref(pa.prm), capi.MEM_HOST, C.byref(pa.out)))
    res = pa.res
    sel, row_off, row_len, rev = [], [], [], []
    for g in range(2):
        nrows, ncol = int(res["nrows"][g]), int(res["ncol"][g])
        assert nrows == 4  # all three traces match
        for i in range(3):
            t = 3 * g + i
            r = nrows - 2 - int(res["rank"][t])
            sel.append(t); row_off.append(int(pa.roff[g]) + r * ncol); row_len.append(ncol); rev.append(not res["forward"][t])
    assert sum(rev) == 2  # the mirrored trace of each group
    pick = [traces[t] for t in sel]
    bc = [dict(bcpos=t["bcpos"], primary=t["pri"], secondary=t["sec"], consensus=t["con"], estqual=t["q"]) for t in pick]
    for device in (False, True):
        rows = (torch.from_numpy(res["rows"]).cuda(), row_off, row_len) if device else (res["rows"], row_off, row_len)
        got = ctx.pad_traces([t["sig"] for t in pick], bc, rows, [t["l"] for t in pick], [t["r"] for t in pick], rev, device=device)
        got = got.results(False) if device else got
        for k, t in enumerate(pick):
            c = dict(t, row=res["rows"][row_off[k]:row_off[k] + row_len[k]].tobytes(), reverse=rev[k])
            pc.compare(got[k], pc.expected(c), (k, device))
