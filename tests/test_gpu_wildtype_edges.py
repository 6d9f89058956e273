"""The edges of the two wildtype-trace paths on the device (tests/wildtype_cases.py; tests/test_wildtype_cases.py asserts without a GPU
that every case is really there): tracyhip_align_traces with refs of kind PROFILE -- rows 4 and 5 of a wildtype read on its reverse
copy, wildtypes of 1 column to 1500, trimmed heights at every strip edge, more than 256 traces in one chunk, a wildtype set laid
out by hand, no score_prelim in device memory -- and tracyhip_decompose_traces with ref_profiles and no `oriented`: every strip
height of the trimmed view, device memory, a strand tie, an N row, a stranger, chunks, lanes and a group.  Every field exact, against
the oracle chain of tests/wildtype_oracle.py."""
import ctypes as C

import numpy as np
import pytest

import wildtype_cases as wc
import wildtype_oracle as wo
from test_gpu_wildtype_decompose import FIELDS

pytestmark = pytest.mark.gpu

SCORE = wc.SCORE


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


# ---- align -----------------------------------------------------------------------------------------------------------------------
def align(c, b, wild=None, **kw):
    return c.align_traces(b["traces"], None, SCORE, b["tl"], b["tr"], ref_index=b["ridx"], ref_profiles=b["wild"] if wild is None else wild,
                          rows=True, **kw)


def check(got, want):
    assert len(got["btr"]) == len(want)
    for i, w in enumerate(want):
        wo.check_trace(got, i, w)


def same(a, b):
    for k in wo.FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert a["btr"] == b["btr"] and a["rows0"] == b["rows0"] and a["rows1"] == b["rows1"]


@pytest.mark.parametrize("option", [None, "no_screen", "no_fused_walk", "no_narrow"])
def test_a1_rows_4_and_5_of_the_reverse_copy(ctx, option):
    b = wc.a1()
    if option:
        ctx.set_option(option, 1)
    try:
        got = align(ctx, b)
    finally:
        if option:
            ctx.set_option(option, 0)
    check(got, b["want"])
    st = ctx.last_call_stats()
    assert st["host_syncs"] == 2 and st["wt_chunks"] == 1


def test_a2_wildtypes_of_one_column_to_1500(ctx):
    b = wc.a2()
    check(align(ctx, b), b["want"])
    check(align(ctx, b, device=True), b["want"])


def test_a3_trimmed_heights_at_the_strip_edges(ctx):
    b = wc.a3()
    check(align(ctx, b), b["want"])
    assert ctx.last_call_stats()["host_syncs"] == 2


def test_a4_more_than_256_traces_in_one_chunk(ctx):
    b = wc.a4()
    whole = align(ctx, b)
    st = ctx.last_call_stats()
    assert st["wt_chunks"] == 1 and st["host_syncs"] == 2 and st["traces"] == 300
    check(whole, b["want"])
    # wildtype_plan.h: the planes of a pair of 120 rows (one pass) and n columns take (n + 63) x 64 words of 8 bytes, 44 544 bytes
    # (n = 24) to 52 736 (n = 40), and one pass needs no boundary rows; seven consecutive traces take 342 528 bytes, all 300 take
    # 14 675 968.  4 MB holds 79 to 94 traces: four chunks.  13.5 MB = 14 155 776 bytes holds 41 runs of seven and a few traces more:
    # a first chunk of more than 256 traces (two blocks of the decision kernel) and a second one that starts behind it
    for limit, chunks in ((4 << 20, 4), (27 << 19, 2)):
        ctx.set_workspace_limit(limit)
        try:
            cut = align(ctx, b)
            st = ctx.last_call_stats()
        finally:
            ctx.set_workspace_limit(0)
        assert st["wt_chunks"] == chunks >= 2 and st["host_syncs"] == 2
        same(whole, cut)


@pytest.mark.parametrize("device", [False, True])
def test_a5_wildtype_set_laid_out_by_hand(ctx, device):
    from tracy_amd import capi
    b = wc.a5()
    laid = capi.PackedSeqs(b["wild"], capi.SEQ_PROFILE)
    laid.data, laid.offset = wc.a5_layout(b["wild"])  # reverse index order, sentinel padding between the profiles
    assert laid.offset.dtype == np.uint64 and laid.data.dtype == np.float32
    got = align(ctx, b, wild=laid, device=device)
    check(got, b["want"])
    same(got, align(ctx, b, device=device))


def test_a6_no_score_prelim_in_device_memory(ctx):
    """the A1 batch with every result array in device memory and score_prelim NULL; ops / rows0 / rows1 with 16 bytes of slack behind
    every trace's mf + n, which stay as they were"""
    import torch
    from tracy_amd import capi
    b = wc.a1()
    nt = len(b["traces"])
    pa = capi.PreparedAlign(b["traces"], None, SCORE, b["tl"], b["tr"], ref_index=b["ridx"], ref_profiles=b["wild"], rows=True)
    pp, pr = pa.keep[0], pa.keep[1]
    cap = pp.length[:nt].astype(np.uint64) + pr.length[b["ridx"]].astype(np.uint64)
    pa.off[1:nt] = np.cumsum(cap + np.uint64(16))[:-1]  # (out.ops_offset points at this array)
    total = int((cap + np.uint64(16)).sum())
    d_prof, d_wild = torch.from_numpy(pp.data).cuda(), torch.from_numpy(pr.data).cuda()
    pa.job.profiles = pp.seqset(d_prof.data_ptr())
    pa.job.refs = pr.seqset(d_wild.data_ptr())
    payloads = ("ops", "rows0", "rows1")
    dres = {k: torch.full((total,), 0x7e, dtype=torch.uint8, device="cuda") if k in payloads else torch.zeros(v.nbytes, dtype=torch.uint8, device="cuda")
            for k, v in pa.res.items()}
    for k, v in dres.items():
        setattr(pa.out, k, v.data_ptr())
    pa.out.score_prelim = None
    torch.cuda.synchronize()
    capi._check(capi.lib().tracyhip_align_traces(ctx._h, C.byref(pa.job), C.byref(pa.prm), capi.MEM_DEVICE, C.byref(pa.out)))
    torch.cuda.synchronize()
    for k, v in dres.items():
        h = v.cpu().numpy()
        pa.res[k] = h if k in payloads else h.view(pa.res[k].dtype)
    assert not pa.res["score_prelim"].any()  # (not handed to the call)
    for k in payloads:
        for t in range(nt):
            end = int(pa.off[t]) + int(cap[t])
            assert (pa.res[k][end:end + 16] == 0x7e).all(), (k, t)
    got = pa.results()
    for i, w in enumerate(b["want"]):
        for k in wo.FIELDS:
            if k != "score_prelim":
                assert int(got[k][i]) == int(w[k]), (i, k)
        assert (got["btr"][i], got["rows0"][i], got["rows1"][i]) == (w["btr"], w["rows0"], w["rows1"]), i


# ---- decompose -------------------------------------------------------------------------------------------------------------------
def decompose(c, d, refs=None, profiles=None, oriented=None, rep=1, ridx=True):
    from tracy_amd import capi
    tr = d["traces"] * rep
    hbc = capi.HostBaseCalls([t["sig"] for t in tr], [t["bcpos"] for t in tr], [t["pri"] for t in tr], [t["sec"] for t in tr])
    return c.decompose_traces([t["prof"] for t in tr], hbc, [w["primary"] for w in d["wild"]] if refs is None else refs, SCORE,
                              np.tile(d["tl"], rep), np.tile(d["tr"], rep), oriented=oriented,
                              ref_profiles=[w["prof"] for w in d["wild"]] if profiles is None else profiles,
                              ref_index=np.tile(d["ridx"], rep) if ridx else None)


def check_chain(got, want):
    """the field list of test_gpu_wildtype_decompose.test_unoriented_call_equals_the_oracle_and_the_oriented_call"""
    for i, w in enumerate(want):
        for k in ("status", "score_fwd", "score_rev", "forward", "score_trim"):
            assert int(got[k][i]) == int(w[k]), (i, k, int(got[k][i]), int(w[k]))
        g = got["bp"][i]
        assert (g.indelshift, g.traceleft, g.breakpoint) == (w["bp"].indelshift, w["bp"].traceleft, w["bp"].breakpoint), i
        assert got["primary"][i] == w["primary"] and got["secondary"][i] == w["secondary"] and got["secdecomp_list"][i] == w["secdecomp"], i
        assert got["dcp"][i] == w["dcp"], i
        assert (float(got["fractions"][2 * i]), float(got["fractions"][2 * i + 1])) == w["af"], i
        for k in range(3):
            assert int(got["score%d" % k][i]) == w["score%d" % k] and got["btr%d" % k][i] == w["btr%d" % k], (i, k)
        for k in range(2):
            for nm in ("slice_begin", "slice_len", "ref_pos"):
                assert int(got["%s%d" % (nm, k)][i]) == int(w["%s%d" % (nm, k)]), (i, nm, k)


def same_call(a, b, nt, strand_scores=True):
    for k in FIELDS + (("score_fwd", "score_rev") if strand_scores else ()):
        assert np.array_equal(np.asarray(a[k])[:nt], np.asarray(b[k])[:nt]), k
    assert np.array_equal(a["fractions"], b["fractions"]) and a["dcp"] == b["dcp"]
    for k in ("primary", "secondary", "secdecomp_list", "btr0", "btr1", "btr2"):
        assert a[k] == b[k], k
    for x, y in zip(list(a["bp"])[:nt], list(b["bp"])[:nt]):
        assert (x.indelshift, x.traceleft, x.breakpoint, x.best_diff) == (y.indelshift, y.traceleft, y.breakpoint, y.best_diff)
    for x, y in zip(list(a["dstatus"])[:nt], list(b["dstatus"])[:nt]):
        assert (x.kind, x.best_ins, x.best_del, x.best_fr, x.dcp_n) == (y.kind, y.best_ins, y.best_del, y.best_fr, y.dcp_n)


def test_d1_every_strip_height_of_the_trimmed_view(ctx):
    import pyoracle as orc
    from sage_oracle import revcomp
    d = wc.d1()
    nt = len(d["traces"])
    got = decompose(ctx, d)
    check_chain(got, d["want"])
    # the call as it was: the caller orients the profile and the string (per trace) and says which strand it is
    fwd = np.array([w["forward"] for w in d["want"]], np.uint8)
    refs_o = [d["wild"][int(r)]["primary"] if f else revcomp(d["wild"][int(r)]["primary"]) for r, f in zip(d["ridx"], fwd)]
    prof_o = [d["wild"][int(r)]["prof"] if f else np.ascontiguousarray(orc.revcomp_profile(d["wild"][int(r)]["prof"])) for r, f in zip(d["ridx"], fwd)]
    old = decompose(ctx, d, refs=refs_o, profiles=prof_o, oriented=fwd, ridx=False)
    assert not old["score_fwd"][:nt].any() and not old["score_rev"][:nt].any()
    same_call(got, old, nt, strand_scores=False)


def test_d2_device_memory(ctx):
    from tracy_amd import capi
    d = wc.d1()
    nt = len(d["traces"])
    host = decompose(ctx, d)  # (its profiles are those of the host chain: hostlib.basecall + create_profile, wildtype_cases._trace)
    pb = capi.PreparedBasecall([t["sig"] for t in d["traces"]], [t["pos"] for t in d["traces"]], 0.33, 0, device=True).run(ctx)
    assert not pb.meta["status"].any()
    assert list(pb.meta["bc_len"][:nt]) == [len(t["pri"]) for t in d["traces"]]
    got = ctx.decompose_traces(None, None, [w["primary"] for w in d["wild"]], SCORE, d["tl"], d["tr"], device_bc=pb,
                               ref_profiles=[w["prof"] for w in d["wild"]], ref_index=d["ridx"])
    same_call(got, host, nt)
    check_chain(got, d["want"])


def test_d3_a_tie_is_reverse(ctx):
    d = wc.d3()
    got = decompose(ctx, d)
    for i, s in enumerate(d["strand"]):
        assert int(got["score_fwd"][i]) == int(got["score_rev"][i]) == s["score_fwd"] and int(got["forward"][i]) == 0
        assert int(got["score_trim"][i]) == s["score_trim"]
    check_chain(got, d["want"])  # (the oracle's chain runs on this input: every field, not the strand fields alone)


def test_d4_an_n_row_and_a_stranger(ctx):
    d = wc.d4()
    check_chain(decompose(ctx, d), d["want"])


def test_d5_chunks_lanes_and_a_group(ctx):
    from tracy_amd import capi
    d = wc.d1()
    nt = 3 * len(d["traces"])
    plain = decompose(ctx, d, rep=3)
    check_chain(plain, d["want"] * 3)
    # run_dp (capi.hip) cuts a traceback launch where the planes pass the limit: passes x (n + 63) x 64 words of 8 bytes per pair, e.g.
    # 2 x (1140 + 63) x 512 = 1 231 872 bytes for 780 rows against the 1140 columns of their wildtype and 7.8 MB for the eleven traces
    # of D1: 6 MB holds every single pair and cuts the 33 traces into four chunks at least
    ctx.set_workspace_limit(6 << 20)
    try:
        same_call(decompose(ctx, d, rep=3), plain, nt)
    finally:
        ctx.set_workspace_limit(0)
    # lanes and groups cut a batch of 64 traces per part at least (33 traces go whole, 132 are cut in two): every part takes the
    # wildtype set along and reverse-complements it again
    for rep in (3, 12):
        ref = plain if rep == 3 else decompose(ctx, d, rep=rep)
        if rep != 3:
            check_chain(ref, d["want"] * rep)
        ctx.set_lanes(2)
        try:
            same_call(decompose(ctx, d, rep=rep), ref, rep * len(d["traces"]))
        finally:
            ctx.set_lanes(1)
        g = capi.Group([0, 0])
        try:
            same_call(decompose(g, d, rep=rep), ref, rep * len(d["traces"]))
        finally:
            g.close()
