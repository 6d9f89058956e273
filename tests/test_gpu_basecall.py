"""Device basecalling (tracyhip_basecall_traces) against the reference's abif.h, the host chain and the restatements of sage_oracle.py:
every output field of every trace, exact (profile floats bit for bit), host and device buffers, int16 and int32 samples, the synchronous
and the queued call; the crafted traces the device must defer -- and no others; and the chain: the device call's output fed as it stands
(TRACYHIP_MEM_DEVICE) into align_traces and decompose_traces against the same calls fed from the host chain."""
import numpy as np
import pytest

import basecall_cases as bcs

pytestmark = pytest.mark.gpu

SCORE = (3, -5, -10, -4)


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    """the synthetic traces, the crafted ones and the deferral cases in one batch, interleaved"""
    syn, cr, de = bcs.synthetic(), bcs.crafted(), bcs.deferred()
    items = [(n, s, p, False) for n, s, p in syn + cr]
    for k, (n, s, p) in enumerate(de):
        items.insert(7 + 31 * k, (n, s, p, True))
    return items


def run(ctx, items, ratio, stringency, device, int16, asynchronous=False):
    from tracy_amd import capi
    sigs = [s.astype(np.int16) if int16 else s for _, s, _, _ in items]
    p = capi.PreparedBasecall(sigs, [q for _, _, q, _ in items], ratio, stringency, device=device)
    assert p.job.sample_bytes == (2 if int16 else 4)
    p.run(ctx, asynchronous)
    if asynchronous:
        ctx.synchronize()
    return p


def check(p, items, ratio, stringency, want_cache):
    rows = p.results(fill_deferred=False)
    deferred = [items[t][0] for t, r in enumerate(rows) if r["status"] != 0]
    assert deferred == [n for n, _, _, d in items if d]  # exactly the crafted deferral cases, none of the synthetic traces
    for t, (name, sig, pos, is_def) in enumerate(items):
        if is_def:
            assert rows[t]["bc_len"] == 0
            continue
        key = (name, ratio)
        if key not in want_cache:
            want_cache[key] = bcs.expected(sig, pos, ratio, range(1, 10))
        bcs.compare(rows[t], want_cache[key], stringency, (name, ratio, stringency))


@pytest.fixture(scope="module")
def want_cache():
    return {}


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("int16", [False, True])
def test_every_field_equals_the_host_chain(ctx, batch, want_cache, device, int16):
    for ratio, stringency in ((0.33, 0), (0.33, 4), (0.1, 1), (0.5, 9), (0.9, 2)):
        check(run(ctx, batch, ratio, stringency, device, int16), batch, ratio, stringency, want_cache)


def test_all_stringencies_and_the_queued_call(ctx, batch, want_cache):
    for s in range(1, 10):
        check(run(ctx, batch, 0.33, s, device=bool(s & 1), int16=bool(s & 2), asynchronous=True), batch, 0.33, s, want_cache)
    p = run(ctx, batch, 0.33, 12.5, True, True)  # clamped to 9 as the commands do
    check(p, batch, 0.33, 9, want_cache)


def test_untouched_outside_the_results_and_optional_payloads(ctx, batch):
    """host buffers: only the first bc_len entries of a trace's region are written, nothing for a deferred trace; NULL payloads are skipped"""
    from tracy_amd import capi
    p = capi.PreparedBasecall([s for _, s, _, _ in batch], [q for _, _, q, _ in batch], 0.33, 4)
    for v in p.payload.values():
        v.view(np.uint8)[:] = 0x7e
    p.run(ctx)
    for t in range(p.nt):
        o, n, cap = int(p.pos_off[t]), int(p.meta["bc_len"][t]), int(p.npos[t])
        for k, _, w in capi._BC_PAYLOADS:
            assert (p.payload[k][w * (o + n):w * (o + cap)].view(np.uint8) == 0x7e).all(), (batch[t][0], k)
    q = capi.PreparedBasecall([s for _, s, _, _ in batch], [q for _, _, q, _ in batch], 0.33, 4)
    for k in ("consensus", "estqual", "bcpos", "secondary"):
        setattr(q.out, k, None)
    q.run(ctx)
    for k in ("status", "bc_len", "trim_left", "trim_right", "best_section"):
        assert np.array_equal(q.meta[k], p.meta[k]), k
    for k, _, w in capi._BC_PAYLOADS:
        if k not in ("primary", "peaks", "profiles"):
            continue
        for t in range(p.nt):
            a, b = w * int(p.pos_off[t]), w * (int(p.pos_off[t]) + int(p.meta["bc_len"][t]))
            assert np.array_equal(q.payload[k][a:b].view(np.uint8), p.payload[k][a:b].view(np.uint8)), (batch[t][0], k)  # (bits: a profile may hold NaN)


def _prefilled(items, int16):
    from tracy_amd import capi
    p = capi.PreparedBasecall([s.astype(np.int16) if int16 else s for _, s, _, _ in items], [q for _, _, q, _ in items], 0.33, 4)
    for v in p.payload.values():
        v.view(np.uint8)[:] = 0x7e
    return p


@pytest.mark.parametrize("int16", [False, True])
def test_chunked_run_equals_the_unlimited_run(ctx, batch, want_cache, int16):
    """host payloads under a workspace limit of a quarter of the staged chromatogram: four chunks or more, every byte as without a limit"""
    from tracy_amd import capi
    items = batch[:40]
    assert any(d for _, _, _, d in items[1:-1])  # deferred traces between answered ones
    syncs = lambda: ctx.last_call_stats()["host_syncs"]
    whole = _prefilled(items, int16)
    s0 = syncs()
    whole.run(ctx)
    assert syncs() - s0 == 2  # one chunk: the results, the copy back
    check(whole, items, 0.33, 4, want_cache)
    cut = _prefilled(items, int16)
    staged = int((4 * cut.nsamples[:cut.nt].astype(np.uint64)).sum()) * cut.job.sample_bytes
    try:
        ctx.set_workspace_limit(staged // 4)
        s0 = syncs()
        cut.run(ctx)
        nsync = syncs() - s0
    finally:
        ctx.set_workspace_limit(0)
    assert nsync >= 8 and nsync % 2 == 0, nsync  # two per chunk
    check(cut, items, 0.33, 4, want_cache)
    for k in ("status", "bc_len", "trim_left", "trim_right", "best_section"):
        assert np.array_equal(cut.meta[k], whole.meta[k]), k
    for k, _, w in capi._BC_PAYLOADS:
        assert np.array_equal(cut.payload[k].view(np.uint8), whole.payload[k].view(np.uint8)), k
        for t in range(cut.nt):
            o, n, cap = int(cut.pos_off[t]), int(cut.meta["bc_len"][t]), int(cut.npos[t])
            assert (cut.payload[k][w * (o + n):w * (o + cap)].view(np.uint8) == 0x7e).all(), (items[t][0], k)


def test_an_offset_that_leaves_64_bits_is_refused(ctx, batch):
    from tracy_amd import capi
    import ctypes as C
    p = _prefilled(batch[:40], False)
    for v in p.meta.values():
        v[:] = 77
    p.pos_off[6] = 2**64 - 8
    rc = capi.lib().tracyhip_basecall_traces(ctx._h, C.byref(p.job), p.mem, C.byref(p.out))
    assert rc == capi.ERR_RANGE
    for k, v in p.meta.items():
        assert (v == 77).all(), k
    for k, v in p.payload.items():
        assert (v.view(np.uint8) == 0x7e).all(), k


def test_context_method_fills_deferred_traces_from_the_host(ctx, batch):
    from tracy_amd import hostlib
    items = batch[:40]
    rows = ctx.basecall_traces([s for _, s, _, _ in items], [p for _, _, p, _ in items], 0.33, 4)
    assert any(d for _, _, _, d in items)
    for r, (name, sig, pos, is_def) in zip(rows, items):
        assert r["status"] == (1 if is_def else 0)
        if r.get("unreadable"):  # a position outside the chromatogram: the host chain would read out of bounds as the reference does
            assert name in ("beyond_samples", "negative") and r["bc_len"] == 0
            continue
        pri, sec, con, bcpos, q = hostlib.basecall_qual(sig, pos, 0.33)
        assert (r["primary"], r["secondary"], r["consensus"]) == (pri, sec, con), name
        assert np.array_equal(r["bcpos"], bcpos) and np.array_equal(r["estqual"], q), name


def _chain_inputs():
    """traces of a kind `tracy align` / `tracy decompose` take: long enough for the 50 / 50 trims, with their reference windows"""
    from tracy_amd import hostlib
    out = []
    for i in range(24):
        mf = 500 + 37 * i
        ref, sig, pos, _ = hostlib.synth_decompose(4000 + i, mf + 400, mf, 30, i % 4, 0.6)
        out.append((ref, sig, pos))
    return out


def test_chain_into_align_traces_on_the_device(ctx):
    import ctypes as C
    import torch
    from tracy_amd import capi, hostlib
    data = _chain_inputs()
    refs = [r for r, _, _ in data]
    host_profiles = []
    for _, sig, pos in data:
        pri, sec, _, bcpos, _ = hostlib.basecall_qual(sig, pos, 0.33)
        host_profiles.append(hostlib.create_profile(sig, bcpos, pri, sec))
    want = ctx.align_traces(host_profiles, refs, SCORE, 50, 50)
    pb = capi.PreparedBasecall([s.astype(np.int16) for _, s, _ in data], [p for _, _, p in data], 0.33, 0, device=True).run(ctx)
    assert not pb.meta["status"].any()
    pa = capi.PreparedAlign(host_profiles, refs, SCORE, 50, 50)  # (the result layout; its profile payload is replaced below)
    assert np.array_equal(pa.keep[0].length[:pb.nt], pb.meta["bc_len"][:pb.nt])
    d_refs = torch.from_numpy(pa.keep[1].data).cuda()
    pa.job.profiles = pb.profiles_seqset()  # the device call's profiles as they stand
    pa.job.refs = pa.keep[1].seqset(d_refs.data_ptr())
    dres = {k: torch.zeros(v.nbytes, dtype=torch.uint8, device="cuda") for k, v in pa.res.items()}
    for k, v in dres.items():
        setattr(pa.out, k, v.data_ptr())
    torch.cuda.synchronize()
    capi._check(capi.lib().tracyhip_align_traces(ctx._h, C.byref(pa.job), C.byref(pa.prm), capi.MEM_DEVICE, C.byref(pa.out)))
    torch.cuda.synchronize()
    for k, v in dres.items():
        pa.res[k] = v.cpu().numpy().view(pa.res[k].dtype)
    got = pa.results()
    for k in ("score_fwd", "score_rev", "forward", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final", "ops_len"):
        assert np.array_equal(got[k], want[k]), k
    assert got["btr"] == want["btr"]


def test_chain_into_decompose_traces_on_the_device(ctx):
    from tracy_amd import capi, hostlib
    data = _chain_inputs()
    refs = [r for r, _, _ in data]
    profs, bcp, pris, secs = [], [], [], []
    for _, sig, pos in data:
        pri, sec, _, bcpos, _ = hostlib.basecall_qual(sig, pos, 0.33)
        profs.append(hostlib.create_profile(sig, bcpos, pri, sec))
        bcp.append(bcpos); pris.append(pri); secs.append(sec)
    hbc = capi.HostBaseCalls([s for _, s, _ in data], bcp, pris, secs)
    want = ctx.decompose_traces(profs, hbc, refs, SCORE)
    pb = capi.PreparedBasecall([s for _, s, _ in data], [p for _, _, p in data], 0.33, 0, device=True).run(ctx)
    assert not pb.meta["status"].any()
    got = ctx.decompose_traces(None, None, refs, SCORE, device_bc=pb)
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), k
        elif isinstance(want[k], list):
            assert got[k] == want[k], k
    for i in range(len(data)):
        for f in ("indelshift", "traceleft", "breakpoint", "best_diff"):
            assert getattr(got["bp"][i], f) == getattr(want["bp"][i], f), (i, f)
        for f in ("kind", "best_ins", "best_del", "best_fr", "dcp_n"):
            assert getattr(got["dstatus"][i], f) == getattr(want["dstatus"][i], f), (i, f)
    assert (want["status"] == 0).any()
