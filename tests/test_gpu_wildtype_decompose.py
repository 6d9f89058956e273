"""tracyhip_decompose_traces against wildtype traces WITHOUT `oriented` (indigo.h:252-291): the call scores the trimmed trace profile
against the forward wildtype profile and its reverse complement, chooses the strand and runs the rest of the chain against the chosen
strand of the profile and of the wildtype's primary basecalls.  Held to the oracle chain (tests/wildtype_oracle.py over
indigo_oracle.decompose_trace) and, field by field, to the call as it was: the caller orients profile and string and sets `oriented`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decomp_cases import SC  # noqa: E402

# (seed, basecalls, kind of tracyhost_synth_decompose: 0 heterozygous indel, 3 no variant; wildtype; the wildtype holds the reverse strand)
CASES = ((31, 480, 0, 0, False), (31, 440, 0, 0, False), (32, 500, 0, 1, True), (32, 460, 0, 1, True), (35, 420, 3, 2, False), (36, 380, 3, 3, True))
WINDOW = 700
FIELDS = ("status", "forward", "score_trim", "score0", "score1", "score2", "slice_begin0", "slice_begin1", "slice_len0", "slice_len1",
          "ref_pos0", "ref_pos1")


def wildtype_chromatogram(seq):
    """one clean peak per base, as tests/test_gpu_cli.py draws a wildtype trace"""
    wt = np.zeros((4, 12 * len(seq) + 12), np.int32)
    wpos = 6 + 12 * np.arange(len(seq), dtype=np.int32)
    tri = (900 * (1.0 - np.abs(np.arange(-5, 6)) / 6.0)).astype(np.int32)
    for j, ch in enumerate(seq):
        wt[b"ACGT".index(ch), wpos[j] - 5:wpos[j] + 6] += tri
    return wt, wpos


@pytest.fixture(scope="module")
def batch():
    import wildtype_oracle as wo
    from sage_oracle import revcomp
    from tracy_amd import hostlib
    traces, wild, ridx, indels = [], {}, [], []
    for seed, mf, kind, w, reverse in CASES:
        ref, sig, pos, indel = hostlib.synth_decompose(seed, WINDOW, mf, 25, kind, 0.6)
        pri, sec, con, bcpos = hostlib.basecall(sig, pos, 0.33)
        traces.append(dict(sig=sig, bcpos=bcpos, pri=pri, sec=sec, prof=hostlib.create_profile(sig, bcpos, pri, sec, 0, 0)))
        indels.append(indel)
        ridx.append(w)
        if w not in wild:  # basecalled like any trace: its profile and its primary calls are the reference
            wsig, wpos = wildtype_chromatogram(revcomp(ref) if reverse else ref)
            gpri, gsec, _, gpos = hostlib.basecall(wsig, wpos, 0.33)
            wild[w] = dict(primary=gpri, prof=hostlib.create_profile(wsig, gpos, gpri, gsec, 0, 0), ref=ref)
        else:
            assert wild[w]["ref"] == ref  # (the same seed and window: two traces over one reference)
    wild = [wild[w] for w in range(len(wild))]
    want = [wo.decompose_trace(t, wild[w]["prof"], wild[w]["primary"], SC) for t, w in zip(traces, ridx)]
    return traces, wild, np.array(ridx, np.uint32), indels, want


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def run(ctx, traces, refs, profiles, ref_index=None, oriented=None):
    from tracy_amd import capi
    hbc = capi.HostBaseCalls([t["sig"] for t in traces], [t["bcpos"] for t in traces], [t["pri"] for t in traces], [t["sec"] for t in traces])
    return ctx.decompose_traces([t["prof"] for t in traces], hbc, refs, SC, oriented=oriented, ref_profiles=profiles, ref_index=ref_index)


def test_the_cases_hold_what_they_should(batch):
    """asserted on the inputs and on the oracle's own results (no GPU)"""
    traces, wild, ridx, indels, want = batch
    assert len(traces) == 6 and all(300 <= len(t["pri"]) <= 560 for t in traces)
    assert any(x < 0 for x in indels) and any(x > 0 for x in indels) and any(x == 0 for x in indels)  # deletion, insertion, none
    assert sorted(list(ridx).count(w) for w in set(ridx.tolist())) == [1, 1, 2, 2]                   # two wildtypes are shared
    assert [w["forward"] for w in want] == [int(not c[4]) for c in CASES] and {w["forward"] for w in want} == {0, 1}
    assert all(w["status"] == 0 for w in want)
    assert all(w["score_fwd"] != w["score_rev"] for w in want)


@pytest.mark.gpu
def test_unoriented_call_equals_the_oracle_and_the_oriented_call(ctx, batch):
    import pyoracle as orc
    from sage_oracle import revcomp
    traces, wild, ridx, indels, want = batch
    got = run(ctx, traces, [w["primary"] for w in wild], [w["prof"] for w in wild], ref_index=ridx)
    # the oracle chain
    for i, w in enumerate(want):
        assert int(got["status"][i]) == w["status"] == 0
        for k in ("score_fwd", "score_rev", "forward", "score_trim"):
            assert int(got[k][i]) == int(w[k]), (i, k)
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
    # score_fwd / score_rev are the two profile x profile scores (the oriented call leaves them zero)
    import wildtype_oracle as wo
    for i, t in enumerate(traces):
        gf, gr, _ = wo.strand_scores(wo.trimmed_view(t["prof"], 50, 50), wild[int(ridx[i])]["prof"], SC)
        assert (int(got["score_fwd"][i]), int(got["score_rev"][i])) == (gf, gr), i
    # the call as it was: the caller orients the profile and the string (per trace) and says which strand it is
    fwd = np.array([w["forward"] for w in want], np.uint8)
    refs_o = [wild[int(r)]["primary"] if f else revcomp(wild[int(r)]["primary"]) for r, f in zip(ridx, fwd)]
    prof_o = [wild[int(r)]["prof"] if f else np.ascontiguousarray(orc.revcomp_profile(wild[int(r)]["prof"])) for r, f in zip(ridx, fwd)]
    old = run(ctx, traces, refs_o, prof_o, oriented=fwd)
    assert not old["score_fwd"][:len(traces)].any() and not old["score_rev"][:len(traces)].any()
    for k in FIELDS:
        assert np.array_equal(np.asarray(got[k])[:len(traces)], np.asarray(old[k])[:len(traces)]), k
    assert np.array_equal(got["fractions"], old["fractions"]) and got["dcp"] == old["dcp"]
    for k in ("primary", "secondary", "secdecomp_list", "btr0", "btr1", "btr2"):
        assert got[k] == old[k], k
    for a, b in zip(got["bp"], old["bp"]):
        assert (a.indelshift, a.traceleft, a.breakpoint, a.best_diff) == (b.indelshift, b.traceleft, b.breakpoint, b.best_diff)
    for a, b in zip(got["dstatus"], old["dstatus"]):
        assert (a.kind, a.best_ins, a.best_del, a.best_fr, a.dcp_n) == (b.kind, b.best_ins, b.best_del, b.best_fr, b.dcp_n)
