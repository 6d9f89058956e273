"""Device trace printing (tracyhip_render_traces) against the host writers (hostlib.render_batch) and the restatements of
tests/render_cases.py: the text of every trace, byte for byte; the three forms, int16 and int32 samples, host and device buffers; text
regions at odd offsets in a buffer of sentinels that must stay untouched around every text; partial workgroups, deferred traces between
answered ones, TOO_SMALL, staging in several chunks, the queued call, the two chains that keep every payload on the device, and the
table form pinned to the stored answers of the reference itself."""
import hashlib
import json

import numpy as np
import pytest

import render_cases as rc

pytestmark = pytest.mark.gpu

SCORE = (3, -5, -10, -4)
SENT = 0x7e
_EXPECTED = {}


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def main_set(wide):
    """the crafted cases and the long trace with what the restatements print for them in each form, computed once per sample width"""
    if wide not in _EXPECTED:
        cases = rc.crafted(256, wide) + [("long", rc.long_trace(wide))]
        _EXPECTED[wide] = [(name, c, {form: rc.expected(c, form) for form in rc.FORMS}) for name, c in cases]
    return _EXPECTED[wide]


def prepared(cases, form, device, int16=False):
    from tracy_amd import capi
    sigs = [c["sig"].astype(np.int16) if int16 else c["sig"] for c in cases]
    return capi.PreparedRender(form, sigs, [rc.bc_of(c) for c in cases], [c["l"] for c in cases], [c["r"] for c in cases], device=device,
                               sample_dtype=np.int16 if int16 else np.int32)


def odd_offsets(caps):
    """text_offset per trace and the buffer size behind them: every region starts at an odd byte, a few bytes behind the one before"""
    off = np.zeros(len(caps) + 1, np.uint64)
    at = 1
    for t, c in enumerate(caps):
        off[t] = at
        at = (at + int(c) + 2) | 1
    off[len(caps)] = at
    return off


def run_checked(ctx, p, asynchronous=False, slack=3, caps=None):
    """the sizes-only call, regions of those sizes plus `slack` bytes at odd offsets in a buffer of sentinels, the call; asserts that no
    byte outside [text_offset, text_offset + text_len) of an answered trace was written.  Returns the per-trace results, no host fill-in"""
    sizes = p.sizes(ctx)
    caps = (sizes.astype(np.uint64) + slack) if caps is None else caps
    p.with_capacity(caps, fill=SENT, offsets=odd_offsets(caps)).run(ctx, asynchronous)
    if asynchronous:
        ctx.synchronize()
    o = p.host_arrays()
    outside = np.ones(len(o["text"]), bool)
    for t in range(p.nt):
        if int(o["status"][t]) == rc.OK:
            a = int(o["text_offset"][t])
            assert int(o["text_len"][t]) <= int(o["text_cap"][t])
            outside[a:a + int(o["text_len"][t])] = False
    assert (o["text"][outside] == SENT).all()
    return p.results(fill_deferred=False)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("form", rc.FORMS)
def test_text_equals_the_host_writers_and_the_restatements(ctx, form, int16, device):
    from tracy_amd import hostlib
    items = main_set(not int16)
    p = prepared([c for _, c, _ in items], form, device, int16)
    rows = run_checked(ctx, p)
    st = ctx.last_call_stats()
    assert (st["render_deferred"], st["render_too_small"], st["render_chunks"]) == (0, 0, 1)  # a deferral cannot hide a failure
    if device:
        assert st["host_syncs"] == 1  # one synchronisation per call with device payloads
    host = hostlib.render_batch(p.host_flat(), form, 4)
    for (name, _, want), got, h in zip(items, rows, host):
        assert h["status"] == rc.OK and h["text"] == want[form], (name, "host")  # none of these is refused on the CPU either
        assert got["status"] == rc.OK and got["text_len"] == len(want[form]), name
        assert got["text"] == want[form], name
    # capacities from tracyhip_render_bound serve a single call without the sizes-only round trip
    rows = run_checked(ctx, p, caps=p.bounds())
    assert ctx.last_call_stats()["render_too_small"] == 0
    for (name, _, want), got in zip(items, rows):
        assert got["text"] == want[form], (name, "bound")


@pytest.mark.parametrize("nt", [1, 3, 4, 5])
def test_partial_workgroups(ctx, nt):
    pick = main_set(False)[3:3 + nt]
    for form in rc.FORMS:
        for device in (False, True):
            rows = run_checked(ctx, prepared([c for _, c, _ in pick], form, device))
            for (name, _, want), got in zip(pick, rows):
                assert (got["status"], got["text"]) == (rc.OK, want[form]), (name, nt, form, device)


def test_deferred_between_answered_and_the_host_fill_in(ctx):
    items = rc.mixed_batch()
    cases = [c for _, c, _ in items]
    for form in rc.FORMS:
        for device in (False, True):
            p = prepared(cases, form, device)
            rows = run_checked(ctx, p)
            st = ctx.last_call_stats()
            assert st["render_deferred"] == sum(1 for _, _, ok in items if not ok) == 6 and st["render_too_small"] == 0
            for (name, c, ok), got in zip(items, rows):
                if ok:
                    assert (got["status"], got["text"]) == (rc.OK, rc.expected(c, form)), (name, form, device)
                else:
                    assert (got["status"], got["text_len"]) == (rc.DEFERRED, 0), name
            # the reference's loops cannot run these either: the fill-in leaves them deferred
            for (name, c, ok), got in zip(items, p.results(fill_deferred=True)):
                if ok:
                    assert got["text"] == rc.expected(c, form), (name, "filled")
                else:
                    assert got["status"] == rc.DEFERRED and got.get("unreadable"), name


def test_too_small_reports_the_size_and_writes_nothing(ctx):
    pick = main_set(False)[:12]
    for form in rc.FORMS:
        for device in (False, True):
            p = prepared([c for _, c, _ in pick], form, device)
            caps = p.sizes(ctx).astype(np.uint64)
            caps[2] -= 1
            caps[5] -= 1
            rows = run_checked(ctx, p, caps=caps)  # (asserts the sentinels: a TOO_SMALL region is untouched)
            assert ctx.last_call_stats()["render_too_small"] == 2
            for t, ((name, _, want), got) in enumerate(zip(pick, rows)):
                assert got["text_len"] == len(want[form]), name
                if t in (2, 5):
                    assert got["status"] == rc.TOO_SMALL
                else:
                    assert (got["status"], got["text"]) == (rc.OK, want[form]), name


def test_host_staging_in_at_least_three_chunks(ctx):
    pick = main_set(False)[:24]
    cases = [c for _, c, _ in pick]
    for form in rc.FORMS:
        ctx.set_workspace_limit(48 << 10)
        try:
            rows = run_checked(ctx, prepared(cases, form, device=False))
            st = ctx.last_call_stats()
        finally:
            ctx.set_workspace_limit(0)
        assert st["render_chunks"] >= 3 and st["render_deferred"] == 0
        for (name, _, want), got in zip(pick, rows):
            assert (got["status"], got["text"]) == (rc.OK, want[form]), (name, form)
        run_checked(ctx, prepared(cases, form, device=False))
        assert ctx.last_call_stats()["render_chunks"] == 1


DEVICE_CHUNK_LIMIT = {rc.TSV: 64, rc.JSON: 256, rc.GAPPED: 128}  # bytes: five chunks of these eight traces in every form


def test_device_payloads_in_at_least_three_chunks(ctx):
    """A device call stages nothing: its tile scratch alone (8 bytes a tile) cuts it.  The launches of all chunks follow each other over
    their slices of one descriptor buffer, and the results of all of them come back behind the last launch, in the one wait of the call."""
    from tracy_amd import hostlib
    pick = main_set(False)[:8]
    cases = [c for _, c, _ in pick]
    for form in rc.FORMS:
        p = prepared(cases, form, device=True)
        ctx.set_workspace_limit(DEVICE_CHUNK_LIMIT[form])
        try:
            rows = run_checked(ctx, p)
            st = ctx.last_call_stats()
        finally:
            ctx.set_workspace_limit(0)
        assert 3 <= st["render_chunks"] < len(cases)  # (some chunks hold several traces)
        assert (st["render_deferred"], st["render_too_small"]) == (0, 0)  # a deferral cannot hide a failure
        assert st["host_syncs"] == 1  # as measured on the commit before the drivers shared one chunk loop: one wait, however many chunks
        whole = run_checked(ctx, prepared(cases, form, device=True))
        assert ctx.last_call_stats()["render_chunks"] == 1
        host = hostlib.render_batch(p.host_flat(), form, 4)
        for (name, _, want), got, one, h in zip(pick, rows, whole, host):
            assert got["status"] == rc.OK and got["text"] == one["text"] == h["text"] == want[form], (name, form)


def _synth(seed, mf):
    from tracy_amd import hostlib
    ref, sig, pos, _ = hostlib.synth_decompose(seed, mf + 400, mf, 30, seed % 4, 0.6)
    return ref, sig, pos


def test_queued_behind_basecalling_on_one_context(ctx):
    from tracy_amd import capi
    data = [_synth(900 + i, 150) for i in range(4)]
    pb = capi.PreparedBasecall([s for _, s, _ in data], [p for _, _, p in data], 0.33, 0, device=True)
    pick = main_set(False)[:20]
    pb.run(ctx, asynchronous=True)
    for form in rc.FORMS:
        rows = run_checked(ctx, prepared([c for _, c, _ in pick], form, device=True), asynchronous=True)
        for (name, _, want), got in zip(pick, rows):
            assert (got["status"], got["text"]) == (rc.OK, want[form]), (name, form)
    assert not pb.meta["status"][:4].any() and pb.meta["bc_len"][:4].min() > 100


def test_chain_signals_to_the_table_on_the_device(ctx):
    """basecall_traces(device=True) -> render_traces(TSV, device_bc=...): the chromatograms and basecalls never leave the device"""
    from tracy_amd import hostlib
    data = [_synth(700 + i, 200) for i in range(8)]
    pb = ctx.basecall_traces([s for _, s, _ in data], [p for _, _, p in data], 0.33, 2, device=True)
    assert not pb.meta["status"][:8].any()
    tl, tr = pb.trims()
    pr = ctx.render_traces(rc.TSV, trim_left=tl, trim_right=tr, device_bc=pb)
    st = ctx.last_call_stats()
    assert st["host_syncs"] == 1 and st["render_deferred"] == 0 and st["render_too_small"] == 0
    for t, (got, (_, sig, pos)) in enumerate(zip(pr.results(fill_deferred=False), data)):
        pri, sec, con, bcpos, q = hostlib.basecall_qual(sig, pos, 0.33)
        want = rc.trace_txt(dict(sig=sig, bcpos=bcpos.tolist(), pri=pri, sec=sec, con=con, q=q, l=int(tl[t]), r=int(tr[t])))
        assert got["status"] == rc.OK and got["text"] == want, t
        assert b"\tY\n" in want and b"\tN\n" in want


def test_chain_signals_to_the_gapped_trace_on_the_device(ctx):
    """signals -> basecalls -> the rows of an alignment -> pad_traces(device) -> render_traces(GAPPED, device_pad=...): equal to the inner
    text of sage_oracle.trace_align_json for the same traces"""
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
    row_off[1:] = np.cumsum(row_len.astype(np.uint64))[:-1]
    d_rows = torch.from_numpy(np.frombuffer(b"".join(rows0), np.uint8).copy()).cuda()
    pp = ctx.pad_traces(None, None, (d_rows, row_off, row_len), device_bc=pb)
    assert ctx.last_call_stats()["pad_deferred"] == 0
    pr = ctx.render_traces(rc.GAPPED, device_pad=pp)
    st = ctx.last_call_stats()
    assert st["host_syncs"] == 1 and st["render_deferred"] == 0 and st["render_too_small"] == 0
    inserted = 0
    for t, (got, (_, sig, _)) in enumerate(zip(pr.results(fill_deferred=False), data)):
        pri, sec, con, bcpos, q = calls[t]
        p = so.alignment_trace_padding(rows0[t], sig, bcpos.tolist(), pri, sec, con, q.tolist())
        inserted += bytes(p["primary"]).count(b"-")
        whole = so.trace_align_json(p, "chr", 7, True, rows0[t], rws[t][1]).encode()
        head = ("{\n\"gappedTrace\":\n{\n\"traceFileName\": \"trace\",\n\"leadingGaps\": %d,\n\"trailingGaps\": %d,\n" % (p["leadingGaps"], p["trailingGaps"])).encode()
        assert got["status"] == rc.OK
        assert whole.startswith(head + got["text"] + b"}\n,\n\"refchr\""), t
    assert inserted > 0  # (pseudo calls were printed)


def test_the_table_is_pinned_to_the_reference(ctx):
    """the cases of tests/test_trace_io.py, basecalled on the host and printed on the device: the sha256 of the text equals the stored
    answer of the reference's traceTxtOut (tests/golden/trace_io_reference.json) wherever the reference wrote a file"""
    import test_trace_io as tio
    from tracy_amd import capi, hostlib
    gold = json.load(open(tio.GOLD_REF))["estqual"]
    cases = list(tio.estqual_cases(np.random.default_rng(77)))
    assert len(cases) == len(gold)
    sigs, bcs = [], []
    for tr, pos in cases:
        pri, sec, con, bcpos, q = hostlib.basecall_qual(tr, pos, 0.33)
        sigs.append(tr)
        bcs.append(dict(bcpos=bcpos, primary=pri, secondary=sec, consensus=con, estqual=q))
    compared = 0
    for k, (lt, rt) in enumerate(tio.TRACE_TXT_TRIMS):
        for device in (False, True):
            p = capi.PreparedRender(rc.TSV, sigs, bcs, [lt] * len(sigs), [rt] * len(sigs), device=device)
            rows = run_checked(ctx, p)
            for got, want in zip(rows, gold):
                w = want["trace_txt"][k]
                if w["rc"] == 0:
                    assert got["status"] == rc.OK and hashlib.sha256(got["text"]).hexdigest() == w["sha256"], (lt, rt, device)
                    compared += 1
    assert compared >= 2 * len(tio.TRACE_TXT_TRIMS) * 5
