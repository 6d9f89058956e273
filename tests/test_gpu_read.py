"""Device file reading (tracyhip_read_traces) against the host readers (hostlib.read_trace, and the reference's stored answers for the golden
files): every field of every trace, exact; the whole case list of tests/read_cases.py as ONE batch with host and device buffers, int16 and
int32 samples, staging in several chunks, the queued call, the sizes-only form, capacities that are too small, and the chain file bytes ->
chromatograms -> basecalls -> the .abif table without a payload on the host."""
import numpy as np
import pytest

import read_cases as rc

pytestmark = pytest.mark.gpu

SENT = 0x7e


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    """(names, images, what the host reader gives or None) of every case, computed once; the golden files carry the reference's answers"""
    named = rc.answered() + rc.abif_cases_images() + rc.deferred() + [rc.scf_wide()]
    want = rc.expected([img for _, img in named])
    gold = rc.golden_images()
    names = [n for n, _ in named] + [n for n, _, _ in gold]
    assert len(set(names)) == len(names)
    return names, [img for _, img in named] + [img for _, img, _ in gold], want + [w for _, _, w in gold]


def packed(images):
    """the images one after another with 0 .. 3 bytes between them: every image address mod 4 occurs"""
    from tracy_amd import hostlib
    flat = hostlib.read_pack(images)
    nt = flat["nt"]
    off = np.zeros(nt + 1, np.uint64)
    for t in range(nt):
        off[t + 1] = off[t] + np.uint64(len(images[t]) + (t * 7 + 1) % 4)
    buf = np.full(int(off[nt]) + 8, 0xEE, np.uint8)
    for t in range(nt):
        buf[int(off[t]):int(off[t]) + len(images[t])] = np.frombuffer(images[t], np.uint8)
    assert {int(o) % 4 for o in off[:nt]} == {0, 1, 2, 3}
    return dict(flat, bytes=buf, file_off=off)


def run_checked(ctx, images, dtype, device, asynchronous=False, slack=3, limit=None):
    """capacities from the bound plus `slack` elements per trace, every payload filled with a sentinel, one call; asserts that nothing past
    the reported sizes was written.  Returns (PreparedRead, per-trace results without host fill-in)"""
    from tracy_amd import capi
    p = capi.PreparedRead(packed(images), dtype, device)
    scap, ccap = p.bounds()
    ctx.set_workspace_limit(limit or 0)
    try:
        p.with_capacity(scap + slack, ccap + slack, fill=SENT).run(ctx, asynchronous)
        if asynchronous:
            ctx.synchronize()
    finally:
        ctx.set_workspace_limit(0)
    o = p.host_arrays()
    sent_sig = np.array([SENT], np.uint8).astype(o["signal"].dtype)[0]
    for t in range(p.nt):
        ok = int(o["status"][t]) == rc.OK
        ks, kc = (4 * int(o["nsamples"][t]), int(o["ncalls"][t])) if ok else (0, 0)
        so, co = int(o["sample_offset"][t]), int(o["call_offset"][t])
        assert (o["signal"][so + ks:int(o["sample_offset"][t + 1])] == sent_sig).all(), t
        for k in ("basecallpos", "basecalls1", "basecalls2", "qual"):
            assert (o[k][co + kc:int(o["call_offset"][t + 1])] == SENT).all(), (t, k)
    return p, p.results(fill_deferred=False)


def fits16(w):
    return w["signal"].max(initial=0) <= 32767 and w["signal"].min(initial=0) >= -32768


def check(batch, res, int16):
    names, _, want = batch
    deferred = {n for n, _ in rc.deferred()} | ({"scf_leaves_int16"} if int16 else set())
    for n, r, w in zip(names, res, want):
        if n in deferred:
            assert (r["status"], r["nsamples"], r["ncalls"]) == (rc.DEFERRED, 0, 0), n
            continue
        assert r["status"] == rc.OK, n
        assert rc.same(r, w) is None, (n, rc.same(r, w))
    return len(deferred)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_every_case_in_one_batch(ctx, batch, device, dtype):
    p, res = run_checked(ctx, batch[1], dtype, device)
    ndef = check(batch, res, dtype == np.int16)
    st = ctx.last_call_stats()
    assert st["read_chunks"] == 1 and st["read_deferred"] == ndef and st["read_too_small"] == 0
    assert st["host_syncs"] == (1 if device else 2)
    fmt = dict(zip(batch[0], p.meta["format"]))
    assert fmt["junk_bytes"] == -1 and fmt["scf_version_2"] == 1 and fmt["repeated_data9"] == 0 and fmt["scf_ns3"] == 1


def test_deferred_traces_are_filled_in_by_the_host_readers(ctx, batch):
    from tracy_amd import hostlib
    names, images, want = batch
    res = ctx.read_traces(images, np.int32)
    for n, r, w in zip(names, res, want):
        if w is None:
            assert r["status"] == rc.DEFERRED and r.get("unreadable"), n
        else:
            assert r["status"] == rc.OK and rc.same(r, w) is None, (n, rc.same(r, w))


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_a_workspace_limit_that_cuts_the_batch(ctx, batch, dtype):
    whole, res0 = run_checked(ctx, batch[1], dtype, False)
    p, res = run_checked(ctx, batch[1], dtype, False, limit=48 << 10)
    ndef = check(batch, res, dtype == np.int16)
    st = ctx.last_call_stats()
    assert st["read_chunks"] >= 3 and st["read_deferred"] == ndef and st["host_syncs"] == 2 * st["read_chunks"]
    a, b = whole.host_arrays(), p.host_arrays()
    for k in ("status", "format", "nsamples", "ncalls", "signal", "basecallpos", "basecalls1", "basecalls2", "qual"):
        assert np.array_equal(a[k], b[k]), k
    # a limit below any file: every file alone
    p, res = run_checked(ctx, batch[1], dtype, False, limit=1)
    check(batch, res, dtype == np.int16)
    assert ctx.last_call_stats()["read_chunks"] == len(batch[1])


@pytest.mark.parametrize("device", [False, True])
def test_queued_call_then_synchronise(ctx, batch, device):
    p, res = run_checked(ctx, batch[1], np.int16, device, asynchronous=True)
    check(batch, res, True)


@pytest.mark.parametrize("device", [False, True])
def test_sizes_only_and_too_small(ctx, batch, device):
    from tracy_amd import capi
    names, images, want = batch
    p = capi.PreparedRead(packed(images), np.int32, device)
    ns, nc = p.sizes(ctx)
    status = p.meta["status"][:p.nt].copy()
    for t, (n, w) in enumerate(zip(names, want)):
        if status[t] == rc.OK:
            assert (ns[t], nc[t]) == (w["signal"].shape[1], len(w["basecallpos"])), n
        else:
            assert (status[t], ns[t], nc[t]) == (rc.DEFERRED, 0, 0), n
    # exactly the reported sizes: everything fits; one sample or one call less for every third trace: TOO_SMALL, the sizes, no payload
    short = np.array([t % 3 == 0 and status[t] == rc.OK for t in range(p.nt)])
    less_samples = short & (np.arange(p.nt) % 2 == 0)
    p.with_capacity(ns - less_samples, nc - (short & ~less_samples), fill=SENT).run(ctx)
    o = p.host_arrays()
    res = p.results(fill_deferred=False)
    sent_sig = np.array([SENT], np.uint8).astype(np.int32)[0]
    for t, (n, w) in enumerate(zip(names, want)):
        if short[t]:
            assert (res[t]["status"], res[t]["nsamples"], res[t]["ncalls"]) == (rc.TOO_SMALL, ns[t], nc[t]), n
            assert (o["signal"][int(o["sample_offset"][t]):int(o["sample_offset"][t + 1])] == sent_sig).all(), n
            assert (o["qual"][int(o["call_offset"][t]):int(o["call_offset"][t + 1])] == SENT).all(), n
        elif status[t] == rc.OK:
            assert res[t]["status"] == rc.OK and rc.same(res[t], w) is None, n
    assert ctx.last_call_stats()["read_too_small"] == int(short.sum())


def test_file_bytes_to_the_abif_table_without_a_host_copy(ctx, batch, tmp_path):
    """read_traces(device=True) -> basecall_traces -> render_traces(TSV) equals hostlib.trace_txt of the same files, byte for byte"""
    from tracy_amd import capi, hostlib
    names, images, want = batch
    keep = [t for t, (n, w) in enumerate(zip(names, want))
            if w is not None and w["signal"].shape[1] >= 64 and fits16(w) and n not in {d for d, _ in rc.deferred()}]
    assert len(keep) >= 20 and {want[t]["format"] for t in keep} == {0, 1}
    for dtype in (np.int16, np.int32):
        rd = ctx.read_traces([images[t] for t in keep], dtype, device=True)
        assert (rd.meta["status"][:rd.nt] == rc.OK).all()
        bc = ctx.basecall_traces(rd)
        assert bc.device and bc.signal is None  # (nothing of the chromatograms came to the host)
        texts = ctx.render_traces(capi.RENDER_TSV, device_bc=bc).results()
        done = 0
        for t, b, r in zip(keep, bc.meta["status"][:bc.nt], texts):
            if b != capi.BASECALL_OK:  # (random positions: a case the basecaller defers is not what this test is about)
                continue
            out = str(tmp_path / "t.abif")
            assert hostlib.trace_txt(out, want[t]["signal"], want[t]["basecallpos"]) == 0
            assert r["text"] == open(out, "rb").read(), names[t]
            done += 1
        assert done >= 15
