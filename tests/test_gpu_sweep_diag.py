"""The 16-bit query-profile sweeps in their offset form (dp_kernels.h, DIAG: six operations per cell) on the device, against the form
on values as they are (option no_sweep_diag), a forced short re-base period (sweep_diag_period = 64) and the oracle: pair lists
through tracyhip_gotoh_score, then both pipelines -- stream-ordered, and planned by the host, whose checkpointed launch leaves row m
and the wavefront checkpoints the band traceback then reads.  The call statistics say which form ran, so a silent fall-back cannot
pass as coverage.

The offset form exists for strips of fifteen and sixteen rows -- traces of 769 to 1 024 rows.  The 300-base batches below therefore
check that the options change nothing where the form does not apply to the full sweeps (and say so: none counted); the 1 000-base
batches run it on strips of fifteen rows, the 1 100-base batches (1 000 rows behind the trims) on strips of sixteen -- whose last
chunk is the one strip_left16<8, LAST, DIAG> that fifteen rows (8 + 7 cells) never instantiate.  The host emulator runs the C++ branch
of every cell helper in dp_lane.h; the asm strings of the device branch run only here.

Scorings other than the benchmark's: test_scorings_at_the_edges_of_the_range_rule, at the periods sweep_diag_period_rule gives them."""
import os
import sys

import numpy as np
import pytest

import pyoracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_sweep_diag as sd  # noqa: E402  (the range rules of sweep_range.h, as the emulator's library exports them)

pytestmark = pytest.mark.gpu
SC = (3, -5, -10, -4)
ALIGN_KEYS = ("forward", "score_fwd", "score_rev", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final")
MS = [1, 14, 15, 16, 31, 130, 899, 900, 960]
NS = [1, 3, 4, 5, 63, 64, 65, 200, 700]
MS16 = [961, 1000, 1009, 1023, 1024]  # strips of sixteen rows: 61 lanes, 63, one row in the last lane (63 x 16 + 1), one short of full, full
NS16 = NS + [1100]                    # (a reference longer than the trace)
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


def choose_k(m):
    """capi.hip choose_k restated for profile rows against strings: the smallest passes x K, ties to the taller strip"""
    return min((16, 15, 12, 8, 4), key=lambda k: -(-max(m, 1) // (64 * k)) * k)


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


def test_pair_lists_score_sixteen_row_strips(ctx):
    """heights of 961 to 1 024 rows (K = 16), references over ACGT (the four-code table) and over ACGTNn-x (the six-code one)"""
    rng = np.random.default_rng(1616)
    sizes = [(m, n) for m in MS16 for n in NS16]
    sizes += [(MS16[int(i)], NS16[int(j)]) for i, j in zip(rng.integers(0, 5, 150), rng.integers(4, 10, 150))]  # 200 pairs
    assert all(choose_k(m) == 16 for m, n in sizes)
    profs = [rand_profile(rng, m, sharp=k % 2 == 0) for k, (m, n) in enumerate(sizes)]
    refs = [bytes(rng.choice(list(b"ACGT" if k % 3 else b"ACGTNn-x"), size=n).tolist()) for k, (m, n) in enumerate(sizes)]
    want = [orc.gotoh_score_prof(p, orc.create_profile_str(r), 1, 0, SC) for p, r in zip(profs, refs)]
    for name, opt in SETTINGS.items():
        scores, ds, _ = under(ctx, opt, lambda: ctx.score(profs, refs, SC + (1, 0)), pipeline=False)
        assert [int(x) for x in scores] == want, name
        assert (ds["sweep_diag_launches"] > 0) == (name != "plain"), (name, ds)


def same_align(a, b, exact, what):
    keys = ALIGN_KEYS if exact else tuple(k for k in ALIGN_KEYS if k not in ("score_fwd", "score_rev"))
    for k in ALIGN_KEYS if what[0] != "no_stream" else keys:  # (the host-planned pipeline bounds the loser's score its own way)
        assert np.array_equal(a[k], b[k]), (what, k, np.nonzero(np.asarray(a[k]) != np.asarray(b[k]))[0][:8])
    assert a["btr"] == b["btr"], what


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("mf,n,nt", [(300, 1500, 64), (1000, 2500, 32), (1100, 2600, 16)])
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
    K = choose_k(mf - 100)  # (the trims leave mf - 100 rows)
    assert K == {300: 4, 1000: 15, 1100: 16}[mf]
    tall = K in (15, 16)  # the offset form applies
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
    """1 000 basecalls: 900 rows behind the trims, strips of fifteen"""
    decompose_batch(ctx, 4712, 32, 3000, 1000)


def test_decompose_traces_sixteen_row_strips(ctx):
    """1 100 basecalls.  `tracy decompose` sweeps the trimmed trace (trims 50 / 50, createProfile's rule: both trims apply while
    their sum is below the number of basecalls), so the swept rows are 1 100 - 100 = 1 000: strips of sixteen"""
    assert choose_k(1100 - 50 - 50) == 16
    decompose_batch(ctx, 4716, 16, 3100, 1100)


def decompose_batch(ctx, seed, nd, n, mf):
    from tracy_amd import capi, hostlib
    d = hostlib.synth_decompose_batch(seed, nd, n, mf, 0, mix=1)
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


# scoring, K -> the period of sweep_diag_period_rule for whole-wave sweeps of K rows (0: no room, the form on values as they are runs)
EDGE_PERIODS = [((3, -5, -10, -18), 15, 256), ((3, -5, -10, -18), 16, 256),
                ((10, -12, -10, -19), 15, 64),
                ((25, -27, -10, -4), 15, 64), ((25, -27, -10, -4), 16, 0),
                ((10, -12, -10, -17), 16, 64),
                ((20, -22, -10, -7), 16, 64),
                ((5, -4, -10, -1), 15, 16384), ((5, -4, -10, -1), 16, 16384),
                ((2, -3, 0, -2), 15, 8192), ((2, -3, 0, -2), 16, 8192)]


@pytest.mark.parametrize("sc,K,period", EDGE_PERIODS, ids=["%d_%d_%d_%d-K%d" % (e[0] + (e[1],)) for e in EDGE_PERIODS])
def test_scorings_at_the_edges_of_the_range_rule(ctx, sc, K, period):
    """Scorings whose own period is the shortest the rule gives (64), short (256), none at all, and far longer than any sweep (a small
    |ge|, and go = 0), at full waves of K rows.  Five pairs built to reach the bounds the rule reasons with -- rows A as a one-hot
    profile against columns that make every cell a mismatch (the values fall as far as they can), every cell a match (they rise as
    far as they can: 64 K x match), half and half either way round, and all N -- and eight random profiles.  The periods are those
    of sweep_range.h today; they are asserted first, so a change of the rule is noticed here."""
    m, n = 64 * K, 1100
    assert sd.narrow_ok(sc, m, K) and sd.diag_period(sc, K) == period, (sd.narrow_ok(sc, m, K), sd.diag_period(sc, K))
    rng = np.random.default_rng(1000 * K + sum(sc))
    rows = orc.create_profile_str(b"A" * m)
    profs = [rows] * 5
    refs = [b"C" * n, b"A" * n, b"A" * (n // 2) + b"C" * (n - n // 2), b"C" * (n // 2) + b"A" * (n - n // 2), b"N" * n]
    for k in range(8):
        profs.append(rand_profile(rng, int(rng.integers(m - 15, m + 1)), sharp=k % 2 == 0))
        refs.append(bytes(rng.choice(list(b"ACGT" if k % 4 < 2 else b"ACGTNn-x"), size=(700, 1100)[k % 2]).tolist()))
    assert all(choose_k(p.shape[1]) == K for p in profs)
    want = [orc.gotoh_score_prof(p, orc.create_profile_str(r), 1, 0, sc) for p, r in zip(profs, refs)]
    assert want[1] == m * sc[0]
    for name in ("auto", "plain"):
        scores, ds, _ = under(ctx, SETTINGS[name], lambda: ctx.score(profs, refs, sc + (1, 0)), pipeline=False)
        assert [int(x) for x in scores] == want, name
        assert (ds["sweep_diag_launches"] > 0) == (name == "auto" and period > 0), (name, ds)


@pytest.mark.parametrize("K", [15, 16])
def test_align_traces_at_a_short_period(ctx, K):
    """3/-5/-10/-18 through the pipeline: the rule gives 256 steps between two re-bases (4 096 at the benchmark's scoring), so every
    sweep of these references re-bases several times at the rule's own period -- 960 rows (K = 15) and 1 000 rows (K = 16) behind
    the trims.  Every field and the traceback against the oracle, and the same with the form switched off."""
    from tracy_amd import hostlib
    from sage_oracle import align_trace
    sc = (3, -5, -10, -18)
    mf = {15: 1060, 16: 1100}[K]
    assert choose_k(mf - 100) == K and sd.diag_period(sc, K) == 256
    refs, profs, rev = hostlib.synth_align(500 + K, 16, 2500, mf, 2)
    refl = [r.tobytes() for r in refs]
    want = [align_trace(profs[i], refl[i], sc, 50, 50) for i in range(16)]
    for exact in (True, False):
        run = lambda: ctx.align_traces(list(profs), refl, sc, 50, 50, exact_scores=exact)
        got, d, _ = under(ctx, {}, run)
        base, d0, _ = under(ctx, {"no_sweep_diag": 1}, run)
        assert d["sweep_diag_launches"] > 0 and d0 == {"sweep_diag_launches": 0, "prefix_diag_launches": 0}, (exact, d, d0)
        same_align(got, base, exact, ("3/-5/-10/-18", K))
        for i, w in enumerate(want):
            win, lose = ("score_fwd", "score_rev") if w["forward"] else ("score_rev", "score_fwd")
            for k in ALIGN_KEYS:
                if exact or k not in ("score_fwd", "score_rev"):
                    assert int(got[k][i]) == int(w[k]), (exact, i, k)
            assert int(got[win][i]) == int(w[win]) and int(got[lose][i]) >= int(w[lose]), (exact, i)  # (the loser may carry its certified bound)
            assert got["btr"][i] == w["btr"], (exact, i)
    assert 0 < int(np.sum(rev)) < 16
