"""The 16-bit query-profile sweeps in their offset form (dp_kernels.h, DIAG: six operations per cell) on the device, against the form
on values as they are (option no_sweep_diag), a forced short re-base period (sweep_diag_period = 64) and the oracle: pair lists
through tracyhip_gotoh_score, then both pipelines -- stream-ordered, and planned by the host, whose checkpointed launch leaves row m
and the wavefront checkpoints the band traceback then reads.  The call statistics say which form ran, so a silent fall-back cannot
pass as coverage.

The offset form exists for strips of fifteen and sixteen rows -- traces of 769 to 1 024 rows.  The 300-base batches below therefore
check that the options change nothing where the form does not apply to the full sweeps (and say so: none counted); the 1 000-base
batches run it."""
import numpy as np
import pytest

import pyoracle as orc

pytestmark = pytest.mark.gpu
SC = (3, -5, -10, -4)
ALIGN_KEYS = ("forward", "score_fwd", "score_rev", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final")
MS = [1, 14, 15, 16, 31, 130, 899, 900, 960]
NS = [1, 3, 4, 5, 63, 64, 65, 200, 700]
SETTINGS = {"auto": {}, "period64": {"sweep_diag_period": 64}, "plain": {"no_sweep_diag": 1}}


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def under(ctx, options, fn, lanes=1, pipeline=True):
    """fn() with the options set, and the offset-form launches it counted: a pipeline call resets the counters when it begins, a
    plain score / align call adds to them"""
    before = ctx.last_call_stats()
    for k, v in options.items():
        ctx.set_option(k, v)
    if lanes != 1:
        ctx.set_lanes(lanes)
    try:
        out = fn()
        st = ctx.last_call_stats()
    finally:
        for k in options:
            ctx.set_option(k, 0)
        if lanes != 1:
            ctx.set_lanes(1)
    d = {k: st[k] - (0 if pipeline else before[k]) for k in ("sweep_diag_launches", "prefix_diag_launches")}
    return out, d, st


def rand_profile(rng, n, sharp):
    p = np.zeros((6, n), dtype=np.float32)
    x = rng.random((4, n)).astype(np.float32)
    if sharp:
        x = x ** 6
    p[:4] = x / x.sum(axis=0, keepdims=True)
    return p


def test_pair_lists_score(ctx):
    rng = np.random.default_rng(909)
    sizes = [(m, n) for m in MS for n in NS]
    sizes += [(MS[int(i)], NS[int(j)]) for i, j in zip(rng.integers(6, 9, 119), rng.integers(0, 9, 119))]  # 200 pairs, most of them tall
    profs = [rand_profile(rng, m, sharp=k % 2 == 0) for k, (m, n) in enumerate(sizes)]
    refs = [bytes(rng.choice(list(b"ACGT" if k % 3 else b"ACGTNn-x"), size=n).tolist()) for k, (m, n) in enumerate(sizes)]
    want = [orc.gotoh_score_prof(p, orc.create_profile_str(r), 1, 0, SC) for p, r in zip(profs, refs)]
    for name, opt in SETTINGS.items():
        scores, ds, _ = under(ctx, opt, lambda: ctx.score(profs, refs, SC + (1, 0)), pipeline=False)
        assert [int(x) for x in scores] == want, name
        assert (ds["sweep_diag_launches"] > 0) == (name != "plain"), (name, ds)  # (the pairs of 899 to 960 rows: strips of fifteen)


def same_align(a, b, exact, what):
    keys = ALIGN_KEYS if exact else tuple(k for k in ALIGN_KEYS if k not in ("score_fwd", "score_rev"))
    for k in ALIGN_KEYS if what[0] != "no_stream" else keys:  # (the host-planned pipeline bounds the loser's score its own way)
        assert np.array_equal(a[k], b[k]), (what, k, np.nonzero(np.asarray(a[k]) != np.asarray(b[k]))[0][:8])
    assert a["btr"] == b["btr"], what


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("mf,n,nt", [(300, 1500, 64), (1000, 2500, 32)])
def test_align_traces(ctx, exact, mf, n, nt):
    from tracy_amd import hostlib
    refs, profs, rev = hostlib.synth_align(77 + mf, nt, n, mf, 2)
    refs = refs.copy()
    refs[3, n // 3] = ord("N")
    refs[nt - 2, n // 2:n // 2 + 3] = ord("N")  # two windows holding N: the six-code table
    refl = [r.tobytes() for r in refs]
    run = lambda: ctx.align_traces(list(profs), refl, SC, 50, 50, exact_scores=exact)
    base, d0, _ = under(ctx, {"no_sweep_diag": 1}, run)
    assert d0 == {"sweep_diag_launches": 0, "prefix_diag_launches": 0}, d0
    tall = mf - 100 > 768  # strips of fifteen rows: the offset form applies
    for what, opt, lanes in (("defaults", {}, 1), ("period64", {"sweep_diag_period": 64}, 1), ("no_stream", {"no_stream": 1}, 1), ("two lanes", {}, 2)):
        got, d, st = under(ctx, opt, run, lanes)
        same_align(got, base, exact, (what, mf))
        if what != "no_stream":
            assert st["stream_ordered"] == 1 and (d["sweep_diag_launches"] > 0) == tall and (d["prefix_diag_launches"] > 0) == tall, (what, d, st)
        else:
            # planned by the host: a strand decided by its certificate is not swept in full, and a launch of prefix groups alone runs
            # in the kernel of the fifteen-row strips whatever the traces' height -- so the prefix rows may take the form on short traces too
            assert st["stream_ordered"] == 0 and (d["sweep_diag_launches"] > 0) == (tall and exact), (what, d, st)
            assert d["prefix_diag_launches"] > 0 or exact, (what, d, st)
    if tall and exact:
        # planned by the host, preliminary alignments by band traceback: the checkpointed launch's row m and wavefront checkpoints are read back
        old = {"no_stream": 1, "no_band16": 1, "no_prelim_origin": 1}
        plain, d1, _ = under(ctx, dict(old, no_sweep_diag=1), run)
        for period in (0, 64):
            got, d, st = under(ctx, dict(old, sweep_diag_period=period) if period else old, run)
            same_align(got, plain, exact, ("checkpoints", period))
            same_align(got, base, exact, ("checkpoints vs default", period))
            assert d["sweep_diag_launches"] > 0 and d1["sweep_diag_launches"] == 0, (period, d, d1)
    want, _ = orc.sage_chain_batch(profs[:16], refs[:16], SC, 50, 50, 2)
    for i, w in enumerate(want):
        for k in ALIGN_KEYS:
            if exact or k not in ("score_fwd", "score_rev"):
                assert int(base[k][i]) == int(w[k]), (i, k)
        assert base["btr"][i] == w["btr"], i
    assert 0 < int(np.sum(rev)) < nt


def test_decompose_traces(ctx):
    from tracy_amd import capi, hostlib
    nd = 32
    d = hostlib.synth_decompose_batch(4712, nd, 3000, 1000, 0, mix=1)
    refs = [d["refs"][i].tobytes() for i in range(nd)]

    def run():
        hbc = capi.HostBaseCalls([d["signal"][i] for i in range(nd)], [d["bcpos"][i] for i in range(nd)],
                                 [d["primary"][i].tobytes() for i in range(nd)], [d["secondary"][i].tobytes() for i in range(nd)])
        return ctx.decompose_traces([d["profiles"][i] for i in range(nd)], hbc, refs, SC)
    res = {}
    for name, opt in SETTINGS.items():
        res[name], dd, st = under(ctx, opt, run)
        assert (dd["sweep_diag_launches"] > 0) == (name != "plain"), (name, dd, st)
    for name in ("auto", "period64"):
        a, b = res[name], res["plain"]
        for k in a:
            x, y = a[k], b[k]
            if k in ("dcp_indel", "dcp_err", "ops"):  # raw tables: compared through the rows written and the tracebacks
                continue
            if k == "bp":
                assert [(v.indelshift, v.traceleft, v.breakpoint, v.best_diff) for v in x] == [(v.indelshift, v.traceleft, v.breakpoint, v.best_diff) for v in y], (name, k)
            elif k == "dstatus":
                assert [(v.kind, v.best_ins, v.best_del, v.best_fr, v.dcp_n) for v in x] == [(v.kind, v.best_ins, v.best_del, v.best_fr, v.dcp_n) for v in y], (name, k)
            elif isinstance(x, np.ndarray):
                assert np.array_equal(x, y), (name, k)
            else:
                assert x == y, (name, k)
