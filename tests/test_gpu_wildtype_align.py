"""tracyhip_align_traces with a wildtype-trace reference (refs of kind PROFILE: sage.h:261-300 + :311, wildtype.hip) against the oracle
composition of tests/wildtype_oracle.py, field by field: both strand scores over the trimmed view, the strand chosen on the device
(a tie is reverse), the final alignment of the FULL profile against the chosen strand, and its two rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_consensus_batch import arith16_holds, column_profile, mutate, passes, strip_height, with_n_row  # noqa: E402

SCORE = (3, -5, -10, -4)
TRIM = 50
FULL = (140, 300, 356, 560, 612, 820, 869)      # rows of the full profiles; the trimmed views have 100 fewer
TRACE_N = (140, 356, 560)                       # full lengths whose FORWARD trace of part A has a non-zero N row
WILD_N = (612, 820)                             # ... whose forward trace's wildtype has one
SHARED = ((330, (300, 300, 356, 356, 300)), (585, (560, 560, 612, 612)), (845, (820, 820, 869, 869, 869)))  # (wildtype columns, its traces)
SHARED_N = {(0, 4), (1, 3), (2, 4)}             # (shared wildtype, trace of it) with an N row in the TRACE: the wildtypes have none
WIDE = 4.0


def _genome(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).tolist())


def make_batch(seed=1311):
    """part A: every full length on both strands, each trace with a wildtype of its own; part B: 14 traces that share three wildtypes.
    Returns (traces, wildtypes, ref_index)."""
    import pyoracle as orc
    rng = np.random.default_rng(seed)
    traces, wild, ridx = [], [], []
    for L in FULL:
        for strand in (0, 1):
            g = _genome(rng, 2 * L)
            n = L - int(rng.integers(0, L // 8 + 1))
            s2 = int(rng.integers(0, L // 8 + 1))
            t = column_profile(rng, mutate(rng, g[:L], 0.02))
            w = column_profile(rng, mutate(rng, g[s2:s2 + n], 0.02))
            if strand == 0 and L in TRACE_N:
                t = with_n_row(rng, t)
            if strand == 0 and L in WILD_N:
                w = with_n_row(rng, w)
            if strand:  # the trace read from the other strand
                t = np.ascontiguousarray(orc.revcomp_profile(t))
            traces.append(t)
            ridx.append(len(wild))
            wild.append(w)
    for wi, (n, lens) in enumerate(SHARED):
        g = _genome(rng, n + 80)
        w = len(wild)
        wild.append(column_profile(rng, g[20:20 + n]))
        for ti, L in enumerate(lens):
            t = column_profile(rng, mutate(rng, g[:L], 0.02))
            if (wi, ti) in SHARED_N:
                t = with_n_row(rng, t)
            if ti % 2:
                t = np.ascontiguousarray(orc.revcomp_profile(t))
            traces.append(t)
            ridx.append(w)
    return traces, wild, np.array(ridx, np.uint32)


def oracle_batch(traces, wild, ridx, tl=TRIM, tr=TRIM, oriented=None):
    import wildtype_oracle as wo
    tl = np.broadcast_to(tl, len(traces))
    tr = np.broadcast_to(tr, len(traces))
    return [wo.align_trace(t, wild[int(ridx[i])], SCORE, int(tl[i]), int(tr[i]), None if oriented is None else int(oriented[i]))
            for i, t in enumerate(traces)]


@pytest.fixture(scope="module")
def batch():
    traces, wild, ridx = make_batch()
    return traces, wild, ridx, oracle_batch(traces, wild, ridx)


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def check(got, want, idx=None):
    import wildtype_oracle as wo
    for i, w in enumerate(want):
        wo.check_trace(got, i if idx is None else idx[i], w)


def same(a, b):
    import wildtype_oracle as wo
    for k in wo.FIELDS:
        assert np.array_equal(a[k], b[k]), k
    assert a["btr"] == b["btr"] and a["rows0"] == b["rows0"] and a["rows1"] == b["rows1"]


def test_the_batch_holds_every_case(batch):
    """asserted on the inputs and on the oracle's own results (no GPU).  The strip-height rule of capi.hip restated: 4 rows per lane up
    to 256 rows, 8 up to 512, 4 again (three passes) up to 768, 8 (two passes) from 769 on; the scores follow the trimmed height, the
    traceback the full one; a pair takes the 16-term body iff row 4 is zero in the trace and in its wildtype."""
    traces, wild, ridx, want = batch
    assert [strip_height(m) for m in (40, 256, 257, 512, 513, 768, 769, 800)] == [4, 4, 8, 8, 4, 4, 8, 8]
    mf = [t.shape[1] for t in traces]
    mt = [m - 2 * TRIM for m in mf]
    assert sorted(set(mf)) == list(FULL) and sorted(set(mt)) == [40, 200, 256, 460, 512, 720, 769]
    for heights in (mt, mf):  # both strip heights with one pass and with several, among the score and among the traceback launches
        for k in (4, 8):
            assert {passes(m) > 1 for m in heights if strip_height(m) == k} == {False, True}
    assert (strip_height(200), strip_height(300)) == (4, 8)                           # 300: the two heights in different strips
    assert (strip_height(460), passes(460), strip_height(560), passes(560)) == (8, 1, 4, 3)  # 560: one pass of 8 / three of 4
    assert all(abs(t.shape[1] - wild[int(r)].shape[1]) <= t.shape[1] // 8 for t, r in zip(traces, ridx))
    fwd = [w["forward"] for w in want]
    assert set(fwd) == {0, 1} and abs(sum(fwd) - len(fwd) / 2) <= 1                   # half of the traces from the other strand
    zero = lambda p: not p[4].any()
    r4 = [zero(t) and zero(wild[int(r)]) for t, r in zip(traces, ridx)]
    assert any(not zero(t) for t in traces) and any(not zero(w) for w in wild)
    for heights in (mt, mf):
        assert {(strip_height(m), z) for m, z in zip(heights, r4)} == {(4, True), (4, False), (8, True), (8, False)}
    shared = [int(r) for r in ridx if list(ridx).count(r) > 1]
    assert len(shared) == 14 and len(set(shared)) == 3                                # 14 traces share three wildtypes
    assert any({want[i]["forward"] for i in range(len(traces)) if ridx[i] == w} == {0, 1} for w in set(shared))
    assert any({r4[i] for i in range(len(traces)) if ridx[i] == w} == {True, False} for w in set(shared))  # same wildtype, other term count
    assert all(arith16_holds(t.shape[1] - 2 * TRIM + wild[int(r)].shape[1], 5) for t, r in zip(traces, ridx))


@pytest.mark.gpu
@pytest.mark.parametrize("option", [None, "no_fused_walk", "no_screen", "no_narrow"])
def test_batch_matches_oracle(ctx, batch, option):
    traces, wild, ridx, want = batch
    if option:
        ctx.set_option(option, 1)
    try:
        got = ctx.align_traces(traces, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=wild, rows=True)
    finally:
        if option:
            ctx.set_option(option, 0)
    check(got, want)
    st = ctx.last_call_stats()
    assert st["host_syncs"] == 2 and st["wt_chunks"] == 1 and st["traces"] == len(traces)  # the classes, the end


@pytest.mark.gpu
def test_tie_is_reverse(ctx):
    """a wildtype that is its own reverse complement: gsFwd == gsRev, the reference takes the reverse strand (sage.h:293)"""
    import pyoracle as orc
    import wildtype_oracle as wo
    rng = np.random.default_rng(5)
    w = np.ascontiguousarray(orc.create_profile_str(b"ACGT" * 60), dtype=np.float32)
    assert np.array_equal(orc.revcomp_profile(w), w)
    t = column_profile(rng, mutate(rng, b"ACGT" * 65, 0.03))
    want = wo.align_trace(t, w, SCORE, TRIM, TRIM)
    assert want["score_fwd"] == want["score_rev"] and want["forward"] == 0
    got = ctx.align_traces([t], None, SCORE, TRIM, TRIM, ref_profiles=[w], rows=True)
    check(got, [want])
    assert int(got["forward"][0]) == 0


@pytest.mark.gpu
def test_trims_each_and_scalars(ctx, batch):
    traces, wild, ridx, want = batch
    nt = len(traces)
    rng = np.random.default_rng(9)
    tl = rng.integers(0, 90, nt).astype(np.uint32)
    tr = rng.integers(0, 90, nt).astype(np.uint32)
    tl[0], tr[0] = 0, 0
    tl[1], tr[1] = 100, 40          # 140 columns: l + r >= mf, clamped to 0 / 0
    tl[2], tr[2] = 120, 3
    tl[3], tr[3] = 2, 190
    got = ctx.align_traces(traces, None, SCORE, tl, tr, ref_index=ridx, ref_profiles=wild, rows=True)
    w2 = oracle_batch(traces, wild, ridx, tl, tr)
    assert w2[1]["score_fwd"] == oracle_batch(traces[1:2], wild, ridx[1:2], 0, 0)[0]["score_fwd"]
    check(got, w2)
    eq = ctx.align_traces(traces, None, SCORE, np.full(nt, TRIM), np.full(nt, TRIM), ref_index=ridx, ref_profiles=wild, rows=True)
    same(eq, ctx.align_traces(traces, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=wild, rows=True))
    check(eq, want)


@pytest.mark.gpu
def test_device_memory_and_chunks(ctx, batch):
    traces, wild, ridx, want = batch
    whole = ctx.align_traces(traces, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=wild, rows=True, device=True)
    syncs = ctx.last_call_stats()["host_syncs"]
    check(whole, want)
    # the planes of an 869 x 869 pair take 2 x 932 x 64 x 8 = 954 368 bytes: 4 MB holds a few traces at a time
    ctx.set_workspace_limit(4 << 20)
    try:
        cut = ctx.align_traces(traces, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=wild, rows=True, device=True)
        st = ctx.last_call_stats()
        cut_host = ctx.align_traces(traces, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=wild, rows=True)
    finally:
        ctx.set_workspace_limit(0)
    assert st["wt_chunks"] >= 3 and st["host_syncs"] == syncs == 2
    same(whole, cut)
    same(whole, cut_host)


@pytest.mark.gpu
def test_repeat_on_int32(ctx, batch):
    """every profile x 4.0: range_verdict sees Q = 82 and refuses the 16-bit score launches whose m + n reaches 730 (the rule restated in
    test_gpu_consensus_batch.py); the call repeats on int32 with twice the synchronisations"""
    traces, wild, ridx, _ = batch
    mn = [t.shape[1] - 2 * TRIM + wild[int(r)].shape[1] for t, r in zip(traces, ridx)]
    assert max(mn) >= 730 and not arith16_holds(max(mn), 82)
    wt = [np.ascontiguousarray(t * np.float32(WIDE)) for t in traces]
    ww = [np.ascontiguousarray(w * np.float32(WIDE)) for w in wild]
    got = ctx.align_traces(wt, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=ww, rows=True)
    assert ctx.last_call_stats()["host_syncs"] == 4
    check(got, oracle_batch(wt, ww, ridx))


@pytest.mark.gpu
def test_oriented(ctx, batch):
    """the caller passes profiles oriented as the oracle orients them: one score in both fields, the rest as the plain call"""
    traces, wild, ridx, want = batch
    ow = [w["chosen"] for w in want]
    fl = np.array([w["forward"] for w in want], np.uint8)
    got = ctx.align_traces(traces, None, SCORE, TRIM, TRIM, ref_profiles=ow, oriented=fl, rows=True)
    assert ctx.last_call_stats()["host_syncs"] == 2
    for i, w in enumerate(want):
        s = w["score_prelim"]
        assert (int(got["score_fwd"][i]), int(got["score_rev"][i]), int(got["score_prelim"][i])) == (s, s, s), i
        assert int(got["forward"][i]) == w["forward"]
        for k in ("slice_begin", "slice_len", "ref_pos", "score_final"):
            assert int(got[k][i]) == int(w[k]), (i, k)
        assert (got["btr"][i], got["rows0"][i], got["rows1"][i]) == (w["btr"], w["rows0"], w["rows1"]), i


@pytest.mark.gpu
def test_lanes_and_group(ctx, batch):
    """a batch large enough to be cut (64 traces per part at least): the shared wildtype set goes whole with every chunk"""
    from tracy_amd import capi
    traces, wild, ridx, want = batch
    rep = 7
    many, midx = traces * rep, np.tile(ridx, rep)
    assert len(many) >= 3 * 64
    plain = ctx.align_traces(many, None, SCORE, TRIM, TRIM, ref_index=midx, ref_profiles=wild, rows=True)
    check(plain, want * rep)
    ctx.set_lanes(2)
    try:
        same(plain, ctx.align_traces(many, None, SCORE, TRIM, TRIM, ref_index=midx, ref_profiles=wild, rows=True))
    finally:
        ctx.set_lanes(1)
    g = capi.Group([0, 0, 0])
    try:
        same(plain, g.align_traces(many, None, SCORE, TRIM, TRIM, ref_index=midx, ref_profiles=wild, rows=True))
        # without ref_index every chunk takes its own wildtypes along
        own = [wild[int(r)] for r in midx]
        same(plain, g.align_traces(many, None, SCORE, TRIM, TRIM, ref_profiles=own, rows=True))
    finally:
        g.close()


@pytest.mark.gpu
def test_async_and_no_traces(ctx, batch):
    from tracy_amd import capi
    traces, wild, ridx, want = batch
    p = capi.PreparedAlign(traces[:14], None, SCORE, TRIM, TRIM, ref_index=ridx[:14], ref_profiles=wild, rows=True)
    q = capi.PreparedAlign(traces[14:], None, SCORE, TRIM, TRIM, ref_index=ridx[14:], ref_profiles=wild)
    ctx.align_traces_async(p.job, p.prm, p.out, capi.MEM_HOST)
    ctx.align_traces_async(q.job, q.prm, q.out, capi.MEM_HOST)
    ctx.synchronize()
    check(p.results(), want[:14])
    check(q.results(), want[14:])  # (no rows asked for)
    z = ctx.align_traces([], None, SCORE, TRIM, TRIM, ref_profiles=capi.PackedSeqs([], capi.SEQ_PROFILE), rows=True)
    assert z["btr"] == [] and z["rows0"] == []
