"""Per-trace trims (trim_left_each / trim_right_each) through tracyhip_align_traces, tracyhip_decompose_traces,
tracyhip_decompose_variants and tracyhip_seed_traces: one call with arrays against the same traces through the scalar interface, one
call per distinct pair, and against the oracle with each trace's own pair -- on the stream-ordered and the host-planned pipeline, where
traces fall back to the host-planned tiers, over lanes and a device group, and down the chain signals -> basecalls -> alignments."""
import numpy as np
import pytest

import indigo_oracle as io
import sage_oracle as so
from test_gpu_stream import ALIGN_KEYS, SC, both_ways, same_align, same_decompose

pytestmark = pytest.mark.gpu
LEFT, RIGHT = (0, 10, 50, 77, 120), (0, 20, 50, 90)
STATS = ("stream_ordered", "host_syncs", "fallback_traces")


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def draw_trims(seed, n):
    rng = np.random.default_rng(seed)
    return rng.choice(LEFT, n).astype(np.uint32), rng.choice(RIGHT, n).astype(np.uint32)


def by_pair(tl, tr):
    """{(l, r): indices}"""
    groups = {}
    for i, p in enumerate(zip(tl.tolist(), tr.tolist())):
        groups.setdefault(p, []).append(i)
    return groups


def align_grouped(ctx, profs, refl, tl, tr, **kw):
    """the scalar interface, one call per distinct pair, put back in trace order"""
    out = {k: [None] * len(profs) for k in ALIGN_KEYS + ("btr",)}
    for (l, r), idx in by_pair(tl, tr).items():
        g = ctx.align_traces([profs[i] for i in idx], [refl[i] for i in idx], SC, l, r, **kw)
        for k in out:
            for j, i in enumerate(idx):
                out[k][i] = g[k][j]
    return {k: (v if k == "btr" else np.asarray(v)) for k, v in out.items()}


def against_align_oracle(got, profs, refl, tl, tr, which, what=""):
    for i in which:
        w = so.align_trace(profs[i], refl[i], SC, int(tl[i]), int(tr[i]))
        for k in ("forward", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final"):
            assert int(got[k][i]) == int(w[k]), (what, i, k, int(tl[i]), int(tr[i]))
        assert got["btr"][i] == w["btr"], (what, i)


@pytest.fixture(scope="module")
def uniform():
    from tracy_amd import hostlib
    refs, profs, rev = hostlib.synth_align(31, 96, 4000, 1000, 2)
    return list(profs), [r.tobytes() for r in refs]


# ---- 1. arrays equal to the scalar ---------------------------------------------------------------------------------------------------
def test_align_arrays_of_one_value_are_the_scalar_call(ctx, uniform):
    profs, refl = uniform
    fifty = np.full(len(profs), 50, np.uint32)
    for device in (False, True):
        a = ctx.align_traces(profs, refl, SC, 50, 50, device=device)
        sa = ctx.last_call_stats()
        b = ctx.align_traces(profs, refl, SC, fifty, fifty, device=device)
        sb = ctx.last_call_stats()
        same_align(a, b, True, "device %s" % device)
        assert np.array_equal(a["ops_len"], b["ops_len"])
        assert {k: sa[k] for k in STATS} == {k: sb[k] for k in STATS} and sa["stream_ordered"] == 1, (sa, sb)


def decompose_run(ctx, d, refs, idx, tl, tr, peaks_only=True):
    from tracy_amd import capi
    hbc = capi.HostBaseCalls([d["signal"][i] for i in idx], [d["bcpos"][i] for i in idx],
                             [d["primary"][i].tobytes() for i in idx], [d["secondary"][i].tobytes() for i in idx])
    return ctx.decompose_traces([d["profiles"][i] for i in idx], hbc, [refs[i] for i in idx], SC, tl, tr, peaks_only=peaks_only)


@pytest.fixture(scope="module")
def dbatch():
    from tracy_amd import hostlib
    nd = 64
    d = hostlib.synth_decompose_batch(2024, nd, 1600, 520, 0, mix=1)
    return d, [d["refs"][i].tobytes() for i in range(nd)], nd


def test_decompose_arrays_of_one_value_are_the_scalar_call(ctx, dbatch):
    d, refs, nd = dbatch
    fifty = np.full(nd, 50, np.uint32)
    a = decompose_run(ctx, d, refs, range(nd), 50, 50)
    sa = ctx.last_call_stats()
    b = decompose_run(ctx, d, refs, range(nd), fifty, fifty)
    sb = ctx.last_call_stats()
    same_decompose(a, b)
    assert {k: sa[k] for k in STATS} == {k: sb[k] for k in STATS} and sa["stream_ordered"] == 1, (sa, sb)


# ---- 2. mixed trims, align -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def uniform_mixed(ctx, uniform):
    """the scalar interface pair by pair (exact scores, default pipeline) and the oracle on every third trace: computed once"""
    profs, refl = uniform
    tl, tr = draw_trims(7, len(profs))
    assert len(by_pair(tl, tr)) >= 12
    return tl, tr, align_grouped(ctx, profs, refl, tl, tr)


@pytest.mark.parametrize("exact", [True, False])
def test_align_mixed_trims(ctx, uniform, uniform_mixed, exact):
    """(the stated trim range keeps the batch stream-ordered: nothing had to be narrowed)"""
    profs, refl = uniform
    tl, tr, grouped = uniform_mixed
    a, sa, b, sb = both_ways(ctx, lambda: ctx.align_traces(profs, refl, SC, tl, tr, exact_scores=exact))
    assert sa["stream_ordered"] == 1 and sb["stream_ordered"] == 0, (sa, sb)
    assert sa["host_syncs"] <= 2, sa
    same_align(a, grouped, exact, "stream-ordered vs one scalar call per pair")
    same_align(b, grouped, exact, "host-planned vs one scalar call per pair")
    against_align_oracle(a, profs, refl, tl, tr, range(0, len(profs), 3))


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------------
def test_align_edge_trims_against_the_oracle(ctx):
    """l + r = mf - 1, mf, mf + 1 (createProfile keeps one column / trims nothing, while trimReferenceSlice still widens by the requested
    values); a window that begins inside the trace (ri < trim_left: no left widening) and one that ends inside it, or an r beyond the
    window (no right widening), on both strands.  The reverse offset n - ri - risize of fmindex.h:455 cannot go negative through the
    pipeline -- the widening keeps ri + risize <= n for every pair of values -- so the reverse traces here are those nearest to it: slices
    that reach the window's last column."""
    from test_gpu_front import COMP, noisy, profile_of, rand_seq
    rng = np.random.default_rng(11)
    profs, wins, tl, tr = [], [], [], []

    def add(seq, win, l, r, reverse=False):
        profs.append(profile_of(rng, seq)); wins.append(win.translate(COMP)[::-1] if reverse else win); tl.append(l); tr.append(r)
    mf = 300
    for total in (mf - 1, mf, mf + 1):
        for l in (0, 120, total):
            seq = rand_seq(rng, mf)
            add(seq, rand_seq(rng, 200) + noisy(rng, seq, 0.02) + rand_seq(rng, 300), l, total - l, reverse=(l == 120))
    for reverse in (False, True):
        seq = rand_seq(rng, 400)
        add(seq, seq[30:] + rand_seq(rng, 500), 50, 20, reverse)            # the window begins inside the trace: ri < trim_left
        add(seq, rand_seq(rng, 500) + seq[:370], 10, 50, reverse)           # ... ends inside it: no room for trim_right
        add(seq, rand_seq(rng, 100) + seq + rand_seq(rng, 40), 50, 90, reverse)     # 40 columns behind the slice, trim_right 90
        add(seq, rand_seq(rng, 100) + seq + rand_seq(rng, 40), 77, 60000, reverse)  # l + r >= mf and r beyond the window
        add(seq, rand_seq(rng, 20) + seq + rand_seq(rng, 400), 120, 0, reverse)     # 20 columns before the slice, trim_left 120
    tl, tr = np.array(tl, np.uint32), np.array(tr, np.uint32)
    a, sa, b, sb = both_ways(ctx, lambda: ctx.align_traces(profs, wins, SC, tl, tr))
    same_align(a, b, True, "stream-ordered (or what took its place) vs host-planned")
    against_align_oracle(a, profs, wins, tl, tr, range(len(profs)), "edges")
    assert len({int(x) for x in a["forward"]}) == 2


# ---- 4. the fallback tiers carry the right pair ------------------------------------------------------------------------------------------
def test_align_fallback_traces_keep_their_own_pair(ctx):
    """test_gpu_front's cases at (50, 50), of which at least four fall back (test_gpu_stream), between uniform traces at other pairs: the
    sub-job of the dead traces must gather each one's own pair -- an index off by one hands a case its neighbour's"""
    from tracy_amd import hostlib
    from test_gpu_front import cases
    cs = cases(np.random.default_rng(77))
    refs, uprofs, _ = hostlib.synth_align(501, len(cs), 2500, 700, 2)
    utl, utr = draw_trims(9, len(cs))
    profs, wins, tl, tr = [], [], [], []
    for i, c in enumerate(cs):
        if (int(utl[i]), int(utr[i])) == (50, 50):
            utl[i] = 77
        profs += [uprofs[i], c[0]]; wins += [refs[i].tobytes(), c[1]]; tl += [int(utl[i]), 50]; tr += [int(utr[i]), 50]
    tl, tr = np.array(tl, np.uint32), np.array(tr, np.uint32)
    a, sa, b, sb = both_ways(ctx, lambda: ctx.align_traces(profs, wins, SC, tl, tr))
    assert sa["stream_ordered"] == 1 and sa["fallback_traces"] >= 4, sa
    same_align(a, b, True, "stream-ordered with fallbacks vs host-planned")
    against_align_oracle(a, profs, wins, tl, tr, [i for i in range(len(profs)) if i % 2 == 1 or i % 8 == 0], "fallback")


# ---- 5. lanes and group ----------------------------------------------------------------------------------------------------------------
def test_align_mixed_trims_over_lanes_and_a_group(ctx):
    import tracy_amd
    from tracy_amd import hostlib
    nt = 256  # two lanes of 128, three group members of 85 / 86: all above the smallest chunk that is split (64)
    refs, profs, _ = hostlib.synth_align(5, nt, 3000, 900, 2)
    profs, refl = list(profs), [r.tobytes() for r in refs]
    tl, tr = draw_trims(13, nt)
    want = ctx.align_traces(profs, refl, SC, tl, tr)
    against_align_oracle(want, profs, refl, tl, tr, (0, 127, 128, 129, 255))
    ctx.set_lanes(2)
    try:
        got = ctx.align_traces(profs, refl, SC, tl, tr, device=True)
        st = ctx.last_call_stats()
        assert st["stream_ordered"] == 1, st
        same_align(got, want, True, "two lanes, device buffers")
        same_align(ctx.align_traces(profs, refl, SC, tl, tr), want, True, "two lanes, host buffers")
    finally:
        ctx.set_lanes(1)
    g = tracy_amd.Group([0, 0, 0])
    try:
        same_align(g.align_traces(profs, refl, SC, tl, tr), want, True, "group of three")
    finally:
        g.close()


def test_decompose_mixed_trims_over_lanes_and_a_group(ctx):
    import tracy_amd
    from tracy_amd import hostlib
    nd = 200
    d = hostlib.synth_decompose_batch(99, nd, 1500, 520, 0, mix=1)
    refs = [d["refs"][i].tobytes() for i in range(nd)]
    tl, tr = draw_trims(17, nd)
    want = decompose_run(ctx, d, refs, range(nd), tl, tr)
    ctx.set_lanes(2)
    try:
        same_decompose(decompose_run(ctx, d, refs, range(nd), tl, tr), want, "two lanes")
    finally:
        ctx.set_lanes(1)
    g = tracy_amd.Group([0, 0, 0])
    try:
        same_decompose(decompose_run(g, d, refs, range(nd), tl, tr), want, "group of three")
    finally:
        g.close()


# ---- 6. mixed trims, decompose and variants ----------------------------------------------------------------------------------------------
RAW = ("dcp_indel", "dcp_err", "ops", "secdecomp")  # (laid out by offsets: compared through dcp, btr* and secdecomp_list)


def trace_view(o, j):
    """everything a decompose outcome holds of trace j, comparable"""
    out = {}
    for k, v in o.items():
        if k in RAW:
            continue
        if k == "fractions":
            out[k] = tuple(float(x) for x in v[2 * j:2 * j + 2])
        elif k == "bp":
            out[k] = (v[j].indelshift, v[j].traceleft, v[j].breakpoint, v[j].best_diff)
        elif k == "dstatus":
            out[k] = (v[j].kind, v[j].best_ins, v[j].best_del, v[j].best_fr, v[j].dcp_n)
        else:
            out[k] = v[j].item() if hasattr(v[j], "item") else v[j]
    return out


@pytest.fixture(scope="module")
def dmixed(ctx, dbatch):
    """the scalar interface pair by pair, with the variant lists of every group: computed once"""
    d, refs, nd = dbatch
    tl, tr = draw_trims(21, nd)
    groups = by_pair(tl, tr)
    assert len(groups) >= 12
    want, lists = [None] * nd, [None] * nd
    for (l, r), idx in groups.items():
        g = decompose_run(ctx, d, refs, idx, l, r)
        got, flags = ctx.decompose_variants(g)
        assert not any(flags)
        for j, i in enumerate(idx):
            lists[i] = got[j]
            want[i] = trace_view(g, j)
    return tl, tr, want, lists


def same_per_trace(got, want, nd, what):
    """(of a trace whose status is not 0 the later outputs are unspecified: its status alone is compared)"""
    for i in range(nd):
        v = trace_view(got, i)
        assert v["status"] == want[i]["status"], (what, i)
        if v["status"] == 0:
            assert v == want[i], (what, i, [k for k in v if v[k] != want[i][k]])


@pytest.mark.parametrize("peaks_only", [True, False], ids=["peak_table", "signal"])
def test_decompose_mixed_trims(ctx, dbatch, dmixed, peaks_only):
    d, refs, nd = dbatch
    tl, tr, want, lists = dmixed
    a, sa, b, sb = both_ways(ctx, lambda: decompose_run(ctx, d, refs, range(nd), tl, tr, peaks_only))
    assert sa["stream_ordered"] == 1 and sb["stream_ordered"] == 0, (sa, sb)
    same_decompose(a, b, "stream-ordered vs host-planned")
    same_per_trace(a, want, nd, "vs one scalar call per pair")
    checked = 0
    for i in range(0, nd, 3):
        w = io.decompose_trace(d["signal"][i], d["bcpos"][i], d["primary"][i].tobytes(), d["secondary"][i].tobytes(), refs[i], SC, int(tl[i]), int(tr[i]))
        assert int(a["status"][i]) == w["status"], i
        if w["status"] != 0:
            continue
        checked += 1
        assert (a["btr0"][i], a["btr1"][i], a["btr2"][i]) == (w["btr0"], w["btr1"], w["btr2"]), (i, int(tl[i]), int(tr[i]))
        assert a["primary"][i] == w["primary"] and a["secondary"][i] == w["secondary"] and a["dcp"][i] == w["dcp"], i
        assert a["secdecomp_list"][i] == w["secdecomp"], i
        for k in range(2):
            assert (int(a["slice_begin%d" % k][i]), int(a["slice_len%d" % k][i]), int(a["ref_pos%d" % k][i])) == \
                (w["slice_begin%d" % k], w["slice_len%d" % k], w["ref_pos%d" % k]), (i, k)
        assert tuple(a["fractions"][2 * i:2 * i + 2]) == tuple(w["af"]), i
    assert checked >= nd // 6, checked


def test_decompose_variants_with_mixed_trims(ctx, dbatch, dmixed):
    from test_gpu_variants import oracle_variants
    d, refs, nd = dbatch
    tl, tr, want, lists = dmixed
    outcome = decompose_run(ctx, d, refs, range(nd), tl, tr)
    got, flags = ctx.decompose_variants(outcome)
    assert not any(flags)
    assert got == lists  # records and text of one scalar call per pair
    checked = 0
    for i in range(16):
        w = io.decompose_trace(d["signal"][i], d["bcpos"][i], d["primary"][i].tobytes(), d["secondary"][i].tobytes(), refs[i], SC, int(tl[i]), int(tr[i]))
        ov = oracle_variants(w, refs[i], (int(tl[i]), int(tr[i])), 0)
        assert got[i] == ([] if ov is None else ov[0]), i
        checked += ov is not None and len(ov[0]) > 0
    assert checked >= 4, checked


# ---- 7. seed ---------------------------------------------------------------------------------------------------------------------------
class IndexedBrute(so.BruteGenome):
    """sage_oracle's genome with the positions of every k-mer of the text looked up in a dictionary built once: the same answers as its
    scan of the text per k-mer, which takes a second per trace on 200 kb"""

    def __init__(self, contigs, k):
        super().__init__(contigs)
        self.k, self.index = k, {}
        for p in range(len(self.text) - k + 1):
            self.index.setdefault(self.text[p:p + k], []).append(p)

    def locate(self, pat):
        return self.index.get(pat, []) if len(pat) == self.k else super().locate(pat)


def test_seed_with_mixed_trims(ctx, tmp_path):
    from tracy_amd import capi, hostlib
    from test_gpu_seed_device import FIELDS, mutate, rand_dna
    rng = np.random.default_rng(31)
    contigs = [rand_dna(rng, 120000), rand_dna(rng, 80000)]
    path = str(tmp_path / "g.fa")
    with open(path, "w") as f:
        for n, c in enumerate(contigs):
            f.write(">chr%d\n%s\n" % (n, "\n".join(c[i:i + 60] for i in range(0, len(c), 60))))
    g = hostlib.Genome(path, 15, 4)
    dg = g.to_device(ctx)
    try:
        reads = []
        for i in range(64):
            c = contigs[i % 2]
            start = int(rng.integers(0, len(c) - 900))
            r = mutate(rng, c[start:start + int(rng.integers(400, 900))], 0.01)
            reads.append((so._revcomp_str(r) if i % 3 == 0 else r).encode())
        tl, tr = draw_trims(41, 64)
        tl[tl < 14], tr[tr < 14] = 14, 20  # every pair inside what the device answers (a trim of at least k - 1) ...
        tl[37], tr[37] = 10, 50             # ... but one
        got = dg.seed(reads, tl, tr, 3, 1000, 4)
        assert got["n_deferred"] == 1  # the device's own verdicts: one trace deferred to the host ...
        ok_l = tl.copy()
        ok_l[37] = 14
        assert dg.seed(reads, ok_l, tr, 3, 1000, 4)["n_deferred"] == 0  # ... the one whose trim is shorter than k - 1
        for (l, r), idx in by_pair(tl, tr).items():
            want = g.seed([reads[i] for i in idx], l, r, 3, 1000, 4)
            for j, i in enumerate(idx):
                assert int(got["status"][i]) == int(want["status"][j]) and int(got["slice_len"][i]) == int(want["slice_len"][j]), (i, l, r)
                if int(want["status"][j]) == 1:
                    for k in FIELDS:
                        assert int(got[k][i]) == int(want[k][j]), (i, k, l, r)
                    assert got["slices"][i] == want["slices"][j], i
        brute = IndexedBrute([("chr%d" % n, c) for n, c in enumerate(contigs)], 15)
        for i, r in enumerate(reads):
            w = so.get_reference_slice(brute, r.decode(), int(tl[i]), int(tr[i]), 15, 3, 1000)
            assert int(got["status"][i]) == (0 if w is None else 1), i
            if w is not None:
                assert (int(got["forward"][i]), int(got["kmersupport"][i]), int(got["pos"][i]), int(got["contig"][i])) == \
                    (int(w["forward"]), w["kmersupport"], w["pos"], w["contig"]), i
                assert got["slices"][i] == w["refslice"].encode(), i
        assert int((np.asarray(got["status"]) == 1).sum()) >= 56
    finally:
        dg.close()
        g.close()


# ---- 8. the chain ----------------------------------------------------------------------------------------------------------------------
def test_basecall_trims_feed_align_traces_on_the_device(ctx):
    """signals -> tracyhip_basecall_traces with a trim stringency (profiles stay on the device, trims come back per trace) ->
    tracyhip_align_traces with those arrays: every trace as the oracle aligns it with the host chain's trims.  The signals are
    basecall_cases' synthetic ones with their ends roughened, so that trimTrace has something to cut."""
    import ctypes as C
    import torch
    from basecall_cases import synthetic
    from tracy_amd import capi, hostlib
    from test_gpu_cli_trims import rough_ends
    rng = np.random.default_rng(3)
    # (as they are, the synthetic signals all trim to (14, 0) at stringency 2: a second peak under some of their first and last calls)
    data = [(n, rough_ends(s, p, (0, 25, 45, 70)[i % 4], (0, 20, 40, 60, 80, 100)[i % 6], rng), p)
            for i, (n, s, p) in enumerate([c for c in synthetic(40, 1000) if len(c[2]) >= 400][:24])]
    host_profiles, refs, host_trims = [], [], []
    for _, sig, pos in data:
        pri, sec, con, bcpos, _ = hostlib.basecall_qual(sig, pos, 0.33)
        host_profiles.append(hostlib.create_profile(sig, bcpos, pri, sec))
        l, r = hostlib.trim_trace(sig, pos, 0.33, 2)
        host_trims.append((l & 0xFFFF, r & 0xFFFF))
        flank = lambda k: bytes(rng.choice(list(b"ACGT"), size=k).tolist())  # noqa: E731
        refs.append(flank(300) + bytes(c if c in b"ACGT" else ord("A") for c in pri) + flank(300))
    assert len(set(host_trims)) >= 4, host_trims
    pb = capi.PreparedBasecall([s for _, s, _ in data], [p for _, _, p in data], 0.33, 2, device=True).run(ctx)
    assert not pb.meta["status"].any()
    tl, tr = pb.trims()
    assert list(zip(tl.tolist(), tr.tolist())) == host_trims
    pa = capi.PreparedAlign(host_profiles, refs, SC, tl, tr)  # (the result layout; its profile payload is replaced below)
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
    against_align_oracle(got, host_profiles, refs, np.array([t[0] for t in host_trims]), np.array([t[1] for t in host_trims]), range(len(data)), "chain")
