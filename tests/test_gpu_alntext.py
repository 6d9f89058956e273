"""Device alignment printing (tracyhip_render_alignments) against the host writers (hostlib.alntext_batch) and the restatement of
tests/alntext_cases.py: the text of every alignment, byte for byte; the three forms and the four keys, host and device buffers; text
regions at odd offsets in a buffer of sentinels that must stay untouched around every text; partial workgroups, deferred alignments
between answered ones, TOO_SMALL, staging in several chunks, the queued call; tracyhip_reference_slices against the host's reverse
complement and substr, and the chain align_traces -> reference_slices -> alignment_rows -> render_alignments with every payload on the
device against the host steps of the command line plus the host writers."""
import ctypes as C

import numpy as np
import pytest

import alntext_cases as ac

pytestmark = pytest.mark.gpu

SCORE = (3, -5, -10, -4)
SENT = 0x7e
_SETS = {}


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def main_set():
    """the crafted and the random alignments with what the restatement prints for them in each form, computed once"""
    if "main" not in _SETS:
        items = ac.crafted() + ac.random_cases()
        _SETS["main"] = [(name, key, L, c, {form: ac.expected(c, form, key, L) for form in ac.FORMS}) for name, key, L, c in items]
    return _SETS["main"]


def groups(items, form):
    """the jobs of a list of (name, key, linelimit, alignment, ...): one per (key, linelimit) for the plot, one for the other forms"""
    g = {}
    for it in items:
        g.setdefault((it[1], it[2]) if form == ac.PLOT else (0, 60), []).append(it)
    return g


def prepared(cs, form, key, L, device):
    from tracy_amd import capi
    return capi.PreparedAlnText(form, key=key, linelimit=L, device=device, **ac.pack(cs))


def odd_offsets(caps):
    """text_offset per alignment and the buffer size behind them: every region starts at an odd byte, a few bytes behind the one before"""
    off = np.zeros(len(caps) + 1, np.uint64)
    at = 1
    for t, c in enumerate(caps):
        off[t] = at
        at = (at + int(c) + 2) | 1
    off[len(caps)] = at
    return off


def run_checked(ctx, p, asynchronous=False, slack=3, caps=None):
    """the sizes-only call, regions of those sizes plus `slack` bytes at odd offsets in a buffer of sentinels, the call; asserts that no
    byte outside [text_offset, text_offset + text_len) of an answered alignment was written.  Returns the results, no host fill-in"""
    sizes = p.sizes(ctx)
    caps = (sizes.astype(np.uint64) + slack) if caps is None else caps
    p.with_capacity(caps, fill=SENT, offsets=odd_offsets(caps)).run(ctx, asynchronous)
    if asynchronous:
        ctx.synchronize()
    o = p.host_arrays()
    outside = np.ones(len(o["text"]), bool)
    for t in range(p.nt):
        if int(o["status"][t]) == ac.OK:
            a = int(o["text_offset"][t])
            assert int(o["text_len"][t]) <= int(o["text_cap"][t])
            outside[a:a + int(o["text_len"][t])] = False
    assert (o["text"][outside] == SENT).all()
    return p.results(fill_deferred=False)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("form", ac.FORMS)
def test_text_equals_the_host_writers_and_the_restatement(ctx, form, device):
    from tracy_amd import hostlib
    compared = 0
    for (key, L), items in groups(main_set(), form).items():
        p = prepared([it[3] for it in items], form, key, L, device)
        rows = run_checked(ctx, p)
        st = ctx.last_call_stats()
        want_deferred = sum(1 for it in items if ac.is_deferred(it[3], form, key))  # (random mirrored plots whose row 1 is longer than ref_len: none today)
        assert (st["alntext_deferred"], st["alntext_too_small"], st["alntext_chunks"]) == (want_deferred, 0, 1)  # a deferral cannot hide a failure
        if device:
            assert st["host_syncs"] == 1  # one synchronisation per call with device payloads
        host = hostlib.alntext_batch(p.host_flat(), form, key, L, 4)
        for it, got, h in zip(items, rows, host):
            want = it[4][form]  # (key and linelimit are read by the plot alone)
            assert h["status"] == ac.OK and h["text"] == want, (it[0], "host")
            if ac.is_deferred(it[3], form, key):
                assert (got["status"], got["text_len"]) == (ac.DEFERRED, 0), it[0]
                continue
            assert got["status"] == ac.OK and got["text_len"] == len(want), it[0]
            assert got["text"] == want, it[0]
            compared += 1
        # capacities from tracyhip_render_alignments_bound serve a single call without the sizes-only round trip
        rows = run_checked(ctx, p, caps=p.bounds())
        assert ctx.last_call_stats()["alntext_too_small"] == 0
        for it, got in zip(items, rows):
            if got["status"] == ac.OK:
                assert got["text"] == it[4][form], (it[0], "bound")
    assert compared >= len(main_set()) - 5


def test_the_most_columns_the_device_answers(ctx):
    """2^22 columns, mirrored: 16 384 column tiles in front of the last anchors"""
    from tracy_amd import hostlib
    name, key, L, c = ac.largest()
    want = ac.expected(c, ac.PLOT, key, L)
    for device in (False, True):
        p = prepared([c], ac.PLOT, key, L, device)
        got = run_checked(ctx, p)[0]
        assert got["status"] == ac.OK and got["text"] == want, device
    assert hostlib.alntext_batch(p.host_flat(), ac.PLOT, key, L, 1)[0]["text"] == want


@pytest.mark.parametrize("nt", [1, 3, 4, 5])
def test_partial_workgroups(ctx, nt):
    pick = [it for it in main_set() if it[1] == 0 and it[2] == 60][2:2 + nt]
    assert len(pick) == nt
    for form in ac.FORMS:
        for device in (False, True):
            rows = run_checked(ctx, prepared([it[3] for it in pick], form, 0, 60, device))
            for it, got in zip(pick, rows):
                assert (got["status"], got["text"]) == (ac.OK, it[4][form]), (it[0], nt, form, device)


def test_deferred_between_answered_and_the_host_fill_in(ctx):
    ok = [it for it in main_set() if it[1] == 0 and it[2] == 60][:9]
    bad = [it for it in ac.deferred() if it[0] != "cols_over"]
    cases, flags = [], []
    for k, it in enumerate(ok):  # an answered alignment on both sides of every deferred one
        cases.append(it[3]); flags.append(False)
        if k < len(bad):
            cases.append(bad[k][3]); flags.append(True)
    assert sum(flags) == len(bad) == 7 and not flags[0] and not flags[-1]
    for form in ac.FORMS:
        for device in (False, True):
            p = prepared(cases, form, 0, 60, device)
            rows = run_checked(ctx, p)
            want_def = [f and ac.is_deferred(c, form, 0) for c, f in zip(cases, flags)]
            st = ctx.last_call_stats()
            assert st["alntext_deferred"] == sum(want_def) >= 4 and st["alntext_too_small"] == 0
            for t, (c, d, got) in enumerate(zip(cases, want_def, rows)):
                if d:
                    assert (got["status"], got["text_len"]) == (ac.DEFERRED, 0), (t, form, device)
                else:
                    assert (got["status"], got["text"]) == (ac.OK, ac.expected(c, form, 0, 60)), (t, form, device)
            # the host batch prints what the device leaves to it
            for t, (c, d, got) in enumerate(zip(cases, want_def, p.results(fill_deferred=True))):
                assert got["status"] == ac.OK and got["text"] == ac.expected(c, form, 0, 60), (t, "filled")
                assert bool(got.get("deferred")) == d
    # a mirrored alignment whose row 1 is too long, found by the data, late in a long alignment and under another key and line length
    name, key, L, c = [it for it in ac.deferred() if it[0] == "mirrored_row1_longer_late"][0]
    p = prepared([ok[0][3], c, ok[1][3]], ac.PLOT, key, L, True)
    rows = run_checked(ctx, p)
    assert [r["status"] for r in rows] == [ac.OK, ac.DEFERRED, ac.OK]
    assert rows[0]["text"] == ac.expected(ok[0][3], ac.PLOT, key, L) and rows[2]["text"] == ac.expected(ok[1][3], ac.PLOT, key, L)


def test_too_small_reports_the_size_and_writes_nothing(ctx):
    pick = [it for it in main_set() if it[1] == 0 and it[2] == 60][:12]
    for form in ac.FORMS:
        for device in (False, True):
            p = prepared([it[3] for it in pick], form, 0, 60, device)
            caps = p.sizes(ctx).astype(np.uint64)
            caps[2] -= 1
            caps[5] -= 1
            rows = run_checked(ctx, p, caps=caps)  # (asserts the sentinels: a TOO_SMALL region is untouched)
            assert ctx.last_call_stats()["alntext_too_small"] == 2
            for t, (it, got) in enumerate(zip(pick, rows)):
                assert got["text_len"] == len(it[4][form]), it[0]
                if t in (2, 5):
                    assert got["status"] == ac.TOO_SMALL
                else:
                    assert (got["status"], got["text"]) == (ac.OK, it[4][form]), it[0]


def test_host_staging_in_at_least_three_chunks(ctx):
    pick = [it for it in main_set() if it[1] == 0 and it[2] == 60 and len(it[3]["row0"]) <= 1100][:24]
    cases = [it[3] for it in pick]
    for form in ac.FORMS:
        ctx.set_workspace_limit(4 << 10)
        try:
            rows = run_checked(ctx, prepared(cases, form, 0, 60, device=False))
            st = ctx.last_call_stats()
        finally:
            ctx.set_workspace_limit(0)
        assert st["alntext_chunks"] >= 3 and st["alntext_deferred"] == 0
        for it, got in zip(pick, rows):
            assert (got["status"], got["text"]) == (ac.OK, it[4][form]), (it[0], form)
        run_checked(ctx, prepared(cases, form, 0, 60, device=False))
        assert ctx.last_call_stats()["alntext_chunks"] == 1


DEVICE_CHUNK_LIMIT = {ac.PLOT: 256, ac.FASTA: 128, ac.JSON: 128}  # bytes: five chunks of these eight alignments in every form


def test_device_payloads_in_at_least_three_chunks(ctx):
    """A device call stages nothing: its tile scratch alone (12 bytes a tile, 8 a column tile) cuts it.  The launches of all chunks follow
    each other over their slices of one descriptor buffer, and the results of all of them come back behind the last launch, in the one
    wait of the call."""
    from tracy_amd import hostlib
    pick = [it for it in main_set() if it[1] == 0 and it[2] == 60 and len(it[3]["row0"]) <= 1100][:8]
    cases = [it[3] for it in pick]
    for form in ac.FORMS:
        p = prepared(cases, form, 0, 60, device=True)
        ctx.set_workspace_limit(DEVICE_CHUNK_LIMIT[form])
        try:
            rows = run_checked(ctx, p)
            st = ctx.last_call_stats()
        finally:
            ctx.set_workspace_limit(0)
        assert 3 <= st["alntext_chunks"] < len(cases)  # (some chunks hold several alignments)
        assert (st["alntext_deferred"], st["alntext_too_small"]) == (0, 0)  # a deferral cannot hide a failure
        assert st["host_syncs"] == 1  # as measured on the commit before the drivers shared one chunk loop: one wait, however many chunks
        whole = run_checked(ctx, prepared(cases, form, 0, 60, device=True))
        assert ctx.last_call_stats()["alntext_chunks"] == 1
        host = hostlib.alntext_batch(p.host_flat(), form, 0, 60, 4)
        for it, got, one, h in zip(pick, rows, whole, host):
            assert got["status"] == ac.OK and got["text"] == one["text"] == h["text"] == it[4][form], (it[0], form)


def test_the_queued_call(ctx):
    pick = [it for it in main_set() if it[1] == 3 and it[2] == 7][:20]
    assert len(pick) >= 5
    for form in ac.FORMS:
        for device in (False, True):
            rows = run_checked(ctx, prepared([it[3] for it in pick], form, 3, 7, device), asynchronous=True)
            for it, got in zip(pick, rows):
                assert (got["status"], got["text"]) == (ac.OK, it[4][form]), (it[0], form)


# ---- tracyhip_reference_slices and the resident chain -------------------------------------------------------------------------------


def test_reference_slices_against_the_host_rule(ctx):
    rng = np.random.default_rng(9)
    alphabet = np.frombuffer(b"ACGTNacgtnRYKMxz-*\x00\x80\xff", np.uint8)
    refs = [alphabet[rng.integers(0, len(alphabet), n)].tobytes() for n in (1, 63, 64, 65, 1023, 1024, 1025, 3000, 17)]
    idx, fwd, begin, ln = [], [], [], []
    for k in range(70):  # (not a multiple of the four waves of a workgroup)
        r = int(rng.integers(0, len(refs)))
        b = int(rng.integers(0, len(refs[r]) + 1))
        idx.append(r); fwd.append(k % 3 != 0); begin.append(b)
        ln.append(len(refs[r]) - b if k % 5 == 0 else int(rng.integers(0, len(refs[r]) - b + 1)))
    want = []
    for r, f, b, n in zip(idx, fwd, begin, ln):
        want.append((refs[r] if f else ac.revcomp_rule(refs[r]))[b:b + n])
    assert any(len(w) == 0 for w in want) and any(len(w) > 1024 for w in want)
    assert ctx.reference_slices(refs, fwd, begin, ln, ref_index=idx) == want
    p = ctx.reference_slices(refs, fwd, begin, ln, ref_index=idx, device=True)
    assert p.slices() == want
    p = ctx.reference_slices(refs, fwd, begin, ln, ref_index=idx, device=True, asynchronous=True)
    ctx.synchronize()
    assert p.slices() == want
    from tracy_amd import capi
    with pytest.raises(capi.TracyHipError) as e:
        ctx.reference_slices(refs, [1], [2], [len(refs[0])], ref_index=[0])
    assert e.value.code == capi.ERR_RANGE


def test_the_resident_chain_against_the_host_steps(ctx):
    """64 traces of 300 bases against 1 kb windows, odd traces on the reverse strand: align_traces(MEM_DEVICE) -> reference_slices ->
    alignment_rows(MEM_DEVICE) -> render_alignments, rows and slices never on the host, against align_traces with host buffers, the
    reverse complement and substr of the command line (align_fasta_group), alignment_rows from host buffers and the host writers"""
    import torch
    from tracy_amd import capi, hostlib
    nt = 64
    batch = hostlib.synth_decompose_batch(4100, nt, 1000, 300, 0, 1)
    profs = [batch["profiles"][t] for t in range(nt)]
    refs = [batch["refs"][t].tobytes() for t in range(nt)]
    lib = capi.lib()
    u8p, u32p = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))), capi._u32p

    def names(fwd, pos, ln, t):
        a, b = pos + 1, pos + ln
        ref = b">Ref chr%d:%d-%d forward" % (t, a, b) if fwd else b">Ref chr%d:%d-%d reversecomplement" % (t, pos + ln - (b - pos) + 1, pos + ln - (a - pos) + 1)
        return {ac.PLOT: (b">Alt", ref), ac.FASTA: (b"trace%d" % t, b"chr%d" % t), ac.JSON: (b"", b"chr%d" % t)}

    # ---- the host steps
    hres = ctx.align_traces(profs, refs, SCORE, 50, 50)
    assert 8 <= int(hres["forward"].sum()) <= nt - 8
    hslices = [(refs[t] if hres["forward"][t] else ac.revcomp_rule(refs[t]))[int(hres["slice_begin"][t]):int(hres["slice_begin"][t]) + int(hres["slice_len"][t])]
               for t in range(nt)]
    pp, ps = capi.PackedSeqs(profs, capi.SEQ_PROFILE), capi.PackedSeqs(hslices, capi.SEQ_CHAR)
    pr = capi.Pairs()
    pr.npairs, pr.a1, pr.a2 = nt, pp.seqset(), ps.seqset()
    hp = capi.PreparedAlign(profs, refs, SCORE, 50, 50)
    off = hp.off
    ops = np.zeros(len(hp.res["ops"]), np.uint8)
    olen = np.ascontiguousarray(hres["ops_len"], dtype=np.uint32)
    for t in range(nt):
        ops[int(off[t]):int(off[t]) + int(olen[t])] = np.frombuffer(hres["btr"][t], np.uint8)
    r0, r1 = np.zeros_like(ops), np.zeros_like(ops)
    capi._check(lib.tracyhip_alignment_rows(ctx._h, C.byref(pr), capi.MEM_HOST, u8p(ops), capi._u64p(off), u32p(olen), u8p(r0), u8p(r1)))
    hrows = [(r0[int(off[t]):int(off[t]) + int(olen[t])].tobytes(), r1[int(off[t]):int(off[t]) + int(olen[t])].tobytes()) for t in range(nt)]

    # ---- the resident chain
    dp_ = capi.PreparedAlign(profs, refs, SCORE, 50, 50)
    dpp, dpr = dp_.keep[0], dp_.keep[1]
    d_prof, d_refs = torch.from_numpy(dpp.data).cuda(), torch.from_numpy(dpr.data).cuda()
    dp_.job.profiles, dp_.job.refs = dpp.seqset(d_prof.data_ptr()), dpr.seqset(d_refs.data_ptr())
    dres = {k: torch.zeros(v.shape, dtype=getattr(torch, str(v.dtype)) if str(v.dtype) != "uint32" else torch.int32, device="cuda") for k, v in dp_.res.items()}
    for k, v in dres.items():
        setattr(dp_.out, k, v.data_ptr())
    torch.cuda.synchronize()
    capi._check(lib.tracyhip_align_traces(ctx._h, C.byref(dp_.job), C.byref(dp_.prm), capi.MEM_DEVICE, C.byref(dp_.out)))
    small = {k: dres[k].cpu().numpy().view(dp_.res[k].dtype) for k in ("forward", "slice_begin", "slice_len", "ref_pos", "score_final", "ops_len")}  # (per-trace numbers, no payload)
    sl = ctx.reference_slices(dpr, small["forward"][:nt], small["slice_begin"][:nt], small["slice_len"][:nt], device_refs=d_refs)
    assert sl.slices() == hslices
    dpairs = capi.Pairs()
    dpairs.npairs, dpairs.a1, dpairs.a2 = nt, dpp.seqset(d_prof.data_ptr()), sl.seqset()
    d_r0, d_r1 = torch.zeros_like(dres["ops"]), torch.zeros_like(dres["ops"])
    capi._check(lib.tracyhip_alignment_rows(ctx._h, C.byref(dpairs), capi.MEM_DEVICE, C.c_void_p(dres["ops"].data_ptr()), capi._u64p(dp_.off),
                                            C.c_void_p(dres["ops_len"].data_ptr()), C.c_void_p(d_r0.data_ptr()), C.c_void_p(d_r1.data_ptr())))
    for form in ac.FORMS:
        nm = [names(bool(small["forward"][t]), int(small["ref_pos"][t]), int(small["slice_len"][t]), t)[form] for t in range(nt)]
        p = ctx.render_alignments(form, name0=[a for a, _ in nm], name1=[b for _, b in nm], ref_pos=small["ref_pos"][:nt], ref_len=small["slice_len"][:nt],
                                  forward=small["forward"][:nt], score=small["score_final"][:nt], key=0, linelimit=60,
                                  device_rows=(d_r0, d_r1, dp_.off, small["ops_len"][:nt]))
        st = ctx.last_call_stats()
        assert (st["alntext_deferred"], st["alntext_too_small"], st["host_syncs"]) == (0, 0, 1)
        hn = [names(bool(hres["forward"][t]), int(hres["ref_pos"][t]), int(hres["slice_len"][t]), t)[form] for t in range(nt)]
        flat = hostlib.alntext_pack([a for a, _ in hrows], [b for _, b in hrows], [a for a, _ in hn], [b for _, b in hn], hres["ref_pos"][:nt],
                                    hres["slice_len"][:nt], hres["forward"][:nt], hres["score_final"][:nt])
        host = hostlib.alntext_batch(flat, form, 0, 60, 4)
        for t, (got, h) in enumerate(zip(p.results(fill_deferred=False), host)):
            assert got["status"] == ac.OK and h["status"] == ac.OK and got["text"] == h["text"], (t, form)
            c = dict(row0=hrows[t][0], row1=hrows[t][1], name0=hn[t][0], name1=hn[t][1], pos=int(hres["ref_pos"][t]), reflen=int(hres["slice_len"][t]),
                     forward=int(hres["forward"][t]), score=int(hres["score_final"][t]))
            assert got["text"] == ac.expected(c, form, 0, 60), (t, form, "restatement")
        if form == ac.PLOT:
            assert any(b"reversecomplement" in r["text"] for r in p.results(fill_deferred=False))
