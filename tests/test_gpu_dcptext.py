"""tracyhip_render_decompositions on the device against the host writers (hostlib.dcptext_batch) and the restatement of
tests/dcptext_cases.py: the hand-made cases and 64 traces carried through decompose_traces -> alignment_rows -> decompose_variants, from
host buffers and with every payload on the device, all three forms; capacities, chunks, the deferred family, the asynchronous form and
the counters.  (What tracyhip_render_decompositions_validate refuses needs no device: tests/test_emu_dcptext.py.)"""
import ctypes as C

import numpy as np
import pytest

import dcptext_cases as dc
import dcptext_chain as ch
from decomp_cases import SC
from sage_oracle import revcomp

pytestmark = pytest.mark.gpu
TRIMS = (20, 20)
SENT = 0x7e
MAXV, MAXT = 64, 1024


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def groups(items):
    """cases that may share a job: one max_variants, max_text and qual_cut"""
    out = {}
    for name, c in items:
        out.setdefault((c["maxv"], c["maxt"], c["qc"]), []).append((name, c))
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("form", dc.FORMS)
def test_crafted_cases(ctx, form, device):
    from tracy_amd import capi, hostlib
    seen = 0
    for (maxv, maxt, qc), group in groups(dc.crafted()).items():
        flat = hostlib.dcptext_pack([c for _, c in group], maxv, maxt)
        host = hostlib.dcptext_batch(flat, form, qc, 4)
        p = capi.PreparedDcpText(form, flat, qc, device=device)
        p.with_capacity(p.sizes(ctx)).run(ctx)
        st = p.stats(ctx)
        assert (st["dcptext_chunks"], st["dcptext_deferred"], st["dcptext_too_small"]) == (1, 0, 0)
        assert ctx.last_call_stats()["host_syncs"] == (1 if device else 2)
        for (name, c), got, h in zip(group, p.results(fill_deferred=False), host):
            want = dc.expected(c, form)
            assert h["status"] == dc.OK and h["text"] == want, (name, "host")
            assert got["status"] == dc.OK and got["text_len"] == len(want) and got["text"] == want, name
            seen += 1
    assert seen == len(dc.crafted())


# ---- the real chain ----------------------------------------------------------------------------------------------------------------


def library_rows(ctx, first, second, btrs):
    """tracyhip_alignment_rows over char x char pairs and their op strings: per pair (row0, row1)"""
    from tracy_amd import capi
    n = len(first)
    pa, pb = capi.PackedSeqs(first, capi.SEQ_CHAR), capi.PackedSeqs(second, capi.SEQ_CHAR)
    pr = capi.Pairs()
    pr.npairs, pr.a1, pr.a2 = n, pa.seqset(), pb.seqset()
    olen = np.array([len(b) for b in btrs], np.uint32)
    off = np.concatenate([[0], np.cumsum(olen.astype(np.uint64))[:-1]]).astype(np.uint64)
    ops = np.frombuffer(b"".join(btrs) + b"\0", np.uint8).copy()
    r0, r1 = np.zeros_like(ops), np.zeros_like(ops)
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    capi._check(capi.lib().tracyhip_alignment_rows(ctx._h, C.byref(pr), capi.MEM_HOST, u8p(ops), capi._u64p(off), capi._u32p(olen), u8p(r0), u8p(r1)))
    return [(r0[int(o):int(o) + int(l)].tobytes(), r1[int(o):int(o) + int(l)].tobytes()) for o, l in zip(off, olen)]


@pytest.fixture(scope="module")
def chain(ctx):
    """64 traces of 300 bases against 600-base windows, odd ones on the reverse strand, through decompose_traces (device payloads) ->
    alignment_rows -> decompose_variants (device payloads); the usable traces as cases, and the device arrays as the calls left them"""
    import torch
    from tracy_amd import capi, hostlib
    nt = 64
    tr = []
    for i in range(nt):
        ref, sig, pos, _ = hostlib.synth_decompose(900 + i, 600, 300, 12, 1 if i % 8 == 7 else 0, (0.6, 0.55, 0.7)[i % 3])
        tr.append(dict(ref=revcomp(ref) if i % 2 else ref, sig=sig, pos=pos))
    pb = capi.PreparedBasecall([t["sig"] for t in tr], [t["pos"] for t in tr], ch.PRATIO, 0, device=True).run(ctx)
    assert not pb.meta["status"].any()
    calls = pb.results(fill_deferred=False)  # (bcpos and estqual; the letters are read behind the decompose call)
    outcome = ctx.decompose_traces(None, None, [t["ref"] for t in tr], SC, *TRIMS, device_bc=pb)
    sp = np.array([1000 * i + 7 for i in range(nt)], np.uint32)
    bufs = capi.VariantBuffers(nt, MAXV, MAXT, device=True)
    var, flags = ctx.decompose_variants(outcome, sp, buffers=bufs)
    good = [t for t in range(nt) if int(outcome["status"][t]) == 0 and int(flags[t]) == 0]
    assert len(good) >= 48 and sum(1 for t in good if outcome["forward"][t]) >= 16 and sum(1 for t in good if not outcome["forward"][t]) >= 16
    ws = []
    for t in good:
        w = dict(status=0, forward=int(outcome["forward"][t]), bp=outcome["bp"][t], af=tuple(float(x) for x in outcome["fractions"][2 * t:2 * t + 2]),
                 dcp=outcome["dcp"][t], primary=outcome["primary"][t], secondary=outcome["secondary"][t], secdecomp=outcome["secdecomp_list"][t])
        for k in range(3):
            w["score%d" % k], w["btr%d" % k] = int(outcome["score%d" % k][t]), outcome["btr%d" % k][t]
        for k in range(2):
            for nm in ("slice_begin", "slice_len", "ref_pos"):
                w["%s%d" % (nm, k)] = int(outcome["%s%d" % (nm, k)][t])
        ws.append(w)
    al = [ch.alleles(w, TRIMS) for w in ws]
    sl = [ch.slices(w, tr[t]["ref"]) for w, t in zip(ws, good)]
    rows = [library_rows(ctx, [a[k] for a in al], [s[k] for s in sl], [w["btr%d" % k] for w in ws]) for k in range(2)]
    rows.append(library_rows(ctx, [a[0] for a in al], [a[1] for a in al], [w["btr2"] for w in ws]))
    cases = [ch.trace_case(w, [rows[k][i] for k in range(3)], calls[t]["bcpos"], calls[t]["estqual"], var[t], int(sp[t]), TRIMS, b"chr%d" % t)
             for i, (w, t) in enumerate(zip(ws, good))]
    assert sum(len(c["variants"]) for c in cases) >= 100 and sum(1 for c in cases if c["indelshift"]) >= 24
    flat = hostlib.dcptext_pack(cases, MAXV, MAXT)
    # the same job over the arrays the three calls left on the device: tables, basecalls and variants where they lie, the rows uploaded
    cap = 2 * 1000 + 2
    dflat = dict(flat, dcp_off=np.append(np.array(good, np.uint64) * np.uint64(cap), np.uint64(0)), bc_off=np.append(pb.pos_off[good], np.uint64(0)),
                 var_index=np.append(np.array(good, np.uint32), np.uint32(0)))
    darr = dict(dcp_indel=outcome.device_tensor("dcp_indel"), dcp_err=outcome.device_tensor("dcp_err"), bcpos=pb.payload["bcpos"],
                estqual=pb.payload["estqual"], var=bufs.t["var"], var_text=bufs.t["text"], var_n=bufs.t["var_n"])
    for k in range(3):
        for r in range(2):
            darr["rows%d_%d" % (r, k)] = torch.from_numpy(flat["rows%d_%d" % (r, k)]).cuda()
    torch.cuda.synchronize()
    return dict(tr=tr, good=good, ws=ws, cases=cases, flat=flat, dflat=dflat, darr=darr, sp=sp, keep=(pb, outcome, bufs))


@pytest.fixture(scope="module")
def chain_host_texts(chain):
    from tracy_amd import hostlib
    return {form: hostlib.dcptext_batch(chain["flat"], form, ch.QUAL_CUT, 4) for form in dc.FORMS}


@pytest.mark.parametrize("form", dc.FORMS)
def test_chain_from_host_buffers_and_on_the_device(ctx, chain, chain_host_texts, form):
    from tracy_amd import capi
    host = chain_host_texts[form]
    got_h = ctx.render_decompositions(form, chain["flat"], ch.QUAL_CUT)
    p = ctx.render_decompositions(form, chain["dflat"], ch.QUAL_CUT, device_arrays=chain["darr"])
    st = p.stats(ctx)
    assert (st["dcptext_chunks"], st["dcptext_deferred"], st["dcptext_too_small"]) == (1, 0, 0) and ctx.last_call_stats()["host_syncs"] == 1
    got_d = p.results(fill_deferred=False)
    for i, c in enumerate(chain["cases"]):
        want = dc.expected(dict(c, maxv=MAXV, maxt=MAXT, qc=ch.QUAL_CUT), form)
        assert host[i]["status"] == dc.OK and host[i]["text"] == want, (i, "host writers")
        assert got_h[i]["status"] == dc.OK and got_h[i]["text"] == want, (i, "host buffers")
        assert got_d[i]["status"] == dc.OK and got_d[i]["text"] == want, (i, "device payloads")


def test_chain_against_the_files_of_the_whole_file_writers(ctx, chain, tmp_path):
    """the first 8 usable traces with an indel shift (the report of the others centres its viewport on a breakpoint the file writer
    looks up itself): .decomp, the tail of the .json, the record lines of the .vcf"""
    pick = [i for i, c in enumerate(chain["cases"]) if c["indelshift"]][:8]
    assert len(pick) == 8
    got = {form: ctx.render_decompositions(form, chain["dflat"], ch.QUAL_CUT, device_arrays=chain["darr"]).results(fill_deferred=False) for form in dc.FORMS}
    for i in pick:
        t, w, c = chain["good"][i], chain["ws"][i], chain["cases"][i]
        d = tmp_path / ("t%d" % i)
        d.mkdir()
        vrows = ch.variant_rows(w, chain["tr"][t]["ref"], TRIMS, c["rows"])
        files = ch.whole_file_texts(d, w, chain["tr"][t]["sig"], chain["tr"][t]["pos"], chain["tr"][t]["ref"], c["rows"], vrows, int(chain["sp"][t]), TRIMS,
                                    c["chr1"].decode())
        for form in dc.FORMS:
            assert got[form][i]["text"] == files[form], (i, form)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sizes_then_exact_capacity_and_one_byte_short(ctx, chain, chain_host_texts, device):
    from tracy_amd import capi
    for form in dc.FORMS:
        host = chain_host_texts[form]
        mk = lambda: capi.PreparedDcpText(form, chain["dflat"], ch.QUAL_CUT, device_arrays=chain["darr"]) if device else capi.PreparedDcpText(form, chain["flat"], ch.QUAL_CUT)
        p = mk()
        sizes = p.sizes(ctx)
        assert [int(s) for s in sizes] == [len(h["text"]) for h in host]
        assert (p.meta["status"][:p.nt] == dc.OK).all()
        p.with_capacity(sizes, fill=SENT).run(ctx)
        o = p.host_arrays()
        assert o["text"][:int(o["text_offset"][p.nt])].tobytes() == b"".join(h["text"] for h in host)
        short = sizes.astype(np.uint64).copy()
        cut = [i for i in range(p.nt) if i % 3 == 1 and sizes[i] > 0]
        short[cut] -= 1
        p = mk().with_capacity(short, fill=SENT).run(ctx)
        o = p.host_arrays()
        for i in range(p.nt):
            a, n = int(o["text_offset"][i]), int(short[i])
            if i in cut:
                assert (o["status"][i], o["text_len"][i]) == (dc.TOO_SMALL, sizes[i]) and (o["text"][a:a + n] == SENT).all(), i
            else:
                assert o["status"][i] == dc.OK and o["text"][a:a + n].tobytes() == host[i]["text"], i
        assert p.stats(ctx)["dcptext_too_small"] == len(cut) > 0


@pytest.mark.parametrize("form", dc.FORMS)
def test_a_workspace_limit_does_not_change_the_bytes(ctx, chain, chain_host_texts, form):
    from tracy_amd import capi
    host = chain_host_texts[form]
    # a trace stages about 0.6 KB for the table and its text, 5 KB of calls and variants for the record lines, 10 KB with the rows and the tail
    ctx.set_workspace_limit({dc.DECOMP: 8 << 10, dc.JSON: 64 << 10, dc.VCF: 32 << 10}[form])
    try:
        p = capi.PreparedDcpText(form, chain["flat"], ch.QUAL_CUT)
        p.with_capacity(p.sizes(ctx), fill=SENT).run(ctx)
        st = p.stats(ctx)
        syncs = ctx.last_call_stats()["host_syncs"]
    finally:
        ctx.set_workspace_limit(0)
    assert st["dcptext_chunks"] >= 3 and syncs == 2 * st["dcptext_chunks"]
    assert [r.get("text") for r in p.results(fill_deferred=False)] == [h["text"] for h in host]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_deferred_traces_write_status_and_length_alone(ctx, device):
    from tracy_amd import capi, hostlib
    for (maxv, maxt, qc), group in list(groups(dc.deferred()).items()) + [((4, 64, dc.QC), [dc.cols_over()])]:
        cs = [dc.base(99, nvar=1, maxv=maxv, maxt=maxt)] + [c for _, c in group] + [dc.base(98, nvar=2, maxv=maxv, maxt=maxt)]
        names = ["good"] + [n for n, _ in group] + ["good"]
        flat = hostlib.dcptext_pack(cs, maxv, maxt)
        for form in dc.FORMS:
            if form != dc.JSON and any(n == "cols_over" for n in names):
                continue  # (one form is enough for four million columns)
            p = capi.PreparedDcpText(form, flat, qc, device=device)
            sizes = p.sizes(ctx)
            p.with_capacity(np.maximum(sizes, 64), fill=SENT).run(ctx)
            o = p.host_arrays()
            deferred = 0
            for i, (name, c) in enumerate(zip(names, cs)):
                a, n = int(o["text_offset"][i]), int(o["text_cap"][i])
                if dc.is_deferred(c, form):
                    deferred += 1
                    assert (o["status"][i], o["text_len"][i], sizes[i]) == (dc.DEFERRED, 0, 0), (name, form)
                    assert (o["text"][a:a + n] == SENT).all(), (name, form)
                else:
                    want = dc.expected(c, form)
                    assert o["status"][i] == dc.OK and o["text"][a:a + len(want)].tobytes() == want and (o["text"][a + len(want):a + n] == SENT).all(), (name, form)
            assert p.stats(ctx)["dcptext_deferred"] == deferred
            # the host answers what it can index, the rest stays deferred
            for name, c, r in zip(names, cs, p.results()):
                if dc.unreadable(c, form):
                    assert r["status"] == dc.DEFERRED and r.get("unreadable"), (name, form)
                else:
                    assert r["status"] == dc.OK and r["text"] == dc.expected(c, form) and bool(r.get("deferred")) == dc.is_deferred(c, form), (name, form)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_async_form_gives_the_same_bytes(ctx, chain, chain_host_texts, device):
    for form in dc.FORMS:
        if device:
            p = ctx.render_decompositions(form, chain["dflat"], ch.QUAL_CUT, device_arrays=chain["darr"], asynchronous=True)
        else:
            p = ctx.render_decompositions(form, chain["flat"], ch.QUAL_CUT, asynchronous=True)
        ctx.synchronize()
        assert [r.get("text") for r in p.results(fill_deferred=False)] == [h["text"] for h in chain_host_texts[form]], form


def test_an_empty_batch_and_an_offset_beyond_64_bits(ctx):
    from tracy_amd import capi, hostlib
    assert ctx.render_decompositions(dc.JSON, hostlib.dcptext_pack([], 4, 64)) == []
    p = capi.PreparedDcpText(dc.DECOMP, hostlib.dcptext_pack([dc.base(1), dc.base(2)], 4, 64))
    p.flat["dcp_off"][1] = 2 ** 64 - 2
    rc = capi.lib().tracyhip_render_decompositions(ctx._h, C.byref(p.job), p.mem, C.byref(p.out))
    assert rc == capi.ERR_RANGE and b"trace 1" in capi.lib().tracyhip_last_error()
