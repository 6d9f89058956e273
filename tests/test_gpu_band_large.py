"""The large-batch form of a band stage of the stream-ordered pipelines (launch_band16_counted, band16.hip: above `b16_multi_max` =
49 152 units strip height 12 gets a launch of its own over its counted list -- on a side stream -- beside band16_multi3_counted_kernel
over the lists of strip height 8 / 4 / quad form), forced on batches of a few dozen traces through the option, against the one-launch
form, the host-planned pipeline and the oracle.  The counters band_list_pairs / band_large_launches of tracyhip_call_stats show which
lists a batch fills and which form its stages took, so that every test can say what it ran.

The pools: an align pool and a decompose pool of 64 traces each.  A pair's list depends on its own band only (s_bucket, stream.hip) and
on whether the launch has room for the quad form -- b16_quad_lds(code_cap) <= 64 KiB, where code_cap follows from the LONGEST TRACE of
the call (StreamCall::size_ncap), not from the windows: with traces of at most 1 010 rows the quad form always fits, whatever the
selection.  The synthetic windows of a pool are of one length; the windows of test_gpu_front.cases are taken as they are."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_stream import ALIGN_KEYS, SC, both_ways, decompose_both_ways, same_align, same_decompose

pytestmark = pytest.mark.gpu
DEFAULT_MAX = 49152
LISTS = ("strip height 12", "strip height 8", "strip height 4", "quad form")
KINDS = ("traceback", "origin sweep")
# what no planning rule lets happen: (kind, list) -> why.  Empty: over the two pools every list of both kinds is reached (the final
# alignments of `tracy align` alone could not: s_final_band gives them 2 w + 1 + |n - m| >= 65 diagonals, strip height 8 or 12).
IMPOSSIBLE = {}


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def mutate(rng, win, rate):
    """substitutions (70 %), deletions and insertions (15 % each) at `rate` per base; the window keeps its length"""
    n = len(win)
    hit = rng.random(n) < rate
    out = bytearray()
    for j, ch in enumerate(win):
        if not hit[j]:
            out.append(ch)
            continue
        u = rng.random()
        if u < 0.70:
            out.append(int(rng.choice([c for c in b"ACGT" if c != ch])))
        elif u >= 0.85:
            out.append(int(rng.choice(list(b"ACGT"))))
            out.append(ch)
    out += bytes(rng.choice(list(b"ACGT"), size=max(0, n - len(out))).tolist())
    return bytes(out[:n])


ALIGN_RATES = (0.0, 0.0, 0.003, 0.006, 0.010, 0.015, 0.020, 0.026, 0.032, 0.040)
DEC_RATES = (0.0, 0.0, 0.0, 0.003, 0.006, 0.012, 0.020, 0.030)


def align_run(ctx, pool, idx):
    r = ctx.align_traces([pool["profs"][i] for i in idx], [pool["wins"][i] for i in idx], SC, 50, 50)
    return r, ctx.last_call_stats()


def sub_dec(pool, idx):
    d = pool["d"]
    return {k: [d[k][i] for i in idx] for k in ("signal", "bcpos", "primary", "secondary", "profiles")}, [pool["refs"][i] for i in idx]


def dec_run(ctx, pool, idx):
    from tracy_amd import capi
    d, refs = sub_dec(pool, idx)
    n = len(idx)
    hbc = capi.HostBaseCalls([d["signal"][i] for i in range(n)], [d["bcpos"][i] for i in range(n)], [d["primary"][i].tobytes() for i in range(n)],
                             [d["secondary"][i].tobytes() for i in range(n)])
    r = ctx.decompose_traces([d["profiles"][i] for i in range(n)], hbc, refs, SC)
    return r, ctx.last_call_stats()


RUN = {"align": align_run, "decompose": dec_run}


def same(which, a, b, what):
    if which == "align":
        same_align(a, b, True, what)
    else:
        same_decompose(a, b, what)


def align_row(r, j):
    return tuple(int(r[k][j]) for k in ALIGN_KEYS) + (r["btr"][j],)


def dec_row(r, j):
    """everything tracyhip_decompose_traces says about trace j of a call (the flat tables through "dcp", "btr*" and "secdecomp_list")"""
    out = []
    for k in sorted(r):
        v = r[k]
        if k in ("dcp_indel", "dcp_err", "ops", "secdecomp"):
            continue
        if k == "bp":
            out.append((k, v[j].indelshift, v[j].traceleft, v[j].breakpoint, v[j].best_diff))
        elif k == "dstatus":
            out.append((k, v[j].kind, v[j].best_ins, v[j].best_del, v[j].best_fr, v[j].dcp_n))
        elif k == "fractions":
            out.append((k, np.asarray(v[2 * j:2 * j + 2]).tobytes()))
        elif isinstance(v, np.ndarray):
            out.append((k, v[j].item()))
        else:
            out.append((k, v[j]))
    return out


ROW = {"align": align_row, "decompose": dec_row}


def forced(ctx, value, fn):
    """fn() with b16_multi_max = value; the default comes back whatever happens"""
    ctx.set_option("b16_multi_max", value)
    try:
        return fn()
    finally:
        ctx.set_option("b16_multi_max", DEFAULT_MAX)


def large(ctx, which, pool, idx):
    """RUN[which] in the large form -- behind a call over OTHER traces of the pool in every slot, so that a pair no workgroup took is
    not found holding the right results of an earlier call over the same batch (the result arrays of a call lie where the last one's lay)"""
    RUN[which](ctx, pool, [(i + 5) % pool["n"] for i in idx])
    return forced(ctx, 0, lambda: RUN[which](ctx, pool, idx))


def band_stages(which, no_fork):
    """band stages a stream-ordered call queues.  `tracy align` has two (preliminary alignment: origin sweep; final alignment: traceback)
    and, with side streams and both exact scores, queues them twice: for the traces decided early beside the other strand's full sweeps,
    then for the rest (AlignStream::queue_stages).  `tracy decompose` has four: the trace (traceback), the alleles' origin sweeps, the
    alleles against their slices and allele 1 against allele 2 (tracebacks)."""
    return (2 if no_fork else 4) if which == "align" else 4


@pytest.fixture(scope="module")
def pools(ctx):
    """the two pools, every trace run alone once (default threshold: the one-launch form), the whole pools on the host-planned pipeline,
    and the oracle's results for every third trace"""
    import indigo_oracle
    import sage_oracle
    from test_gpu_front import cases
    from tracy_amd import hostlib
    rng = np.random.default_rng(2026)
    ns = 40
    refs, profs, _ = hostlib.synth_align(2024, ns, 3000, 900, 2)
    front = cases(np.random.default_rng(77))[:24]  # three of every kind; strip heights 8 / 12 / 15 / 16 of the sweeps in one batch
    al = {"profs": [np.ascontiguousarray(profs[i]) for i in range(ns)] + [c[0] for c in front],
          "wins": [mutate(rng, refs[i].tobytes(), ALIGN_RATES[i % len(ALIGN_RATES)]) for i in range(ns)] + [c[1] for c in front]}
    assert len({len(w) for w in al["wins"][:ns]}) == 1
    nd = 64
    d = hostlib.synth_decompose_batch(4242, nd, 2600, 900, 0, mix=1)
    de = {"d": d, "refs": [mutate(rng, d["refs"][i].tobytes(), DEC_RATES[i % len(DEC_RATES)]) for i in range(nd)]}
    assert len({len(w) for w in de["refs"]}) == 1
    out = {"align": al, "decompose": de}
    for which, pool in out.items():
        n = len(pool["wins"] if which == "align" else pool["refs"])
        pool["n"] = n
        pool["single"] = []
        for i in range(n):
            r, st = RUN[which](ctx, pool, [i])
            assert st["stream_ordered"] == 1 and st["band_large_launches"] == 0, (which, i, st)
            pool["single"].append({"row": ROW[which](r, 0), "lists": np.asarray(st["band_list_pairs"]), "fallback": st["fallback_traces"]})
    a, sa, b, sb = both_ways(ctx, lambda: align_run(ctx, al, range(al["n"]))[0])
    assert sa["stream_ordered"] == 1 and sb["stream_ordered"] == 0 and sb["band_large_launches"] == 0, (sa, sb)
    assert sb["band_list_pairs"] == [[0] * 4] * 2, sb  # planned by the host: no scan, no lists
    al["default"], al["host"] = a, b
    a, sa, b, sb = decompose_both_ways(ctx, *sub_dec(de, range(nd)), nd)
    assert sa["stream_ordered"] == 1 and sb["stream_ordered"] == 0 and sb["band_large_launches"] == 0, (sa, sb)
    assert sb["band_list_pairs"] == [[0] * 4] * 2, sb
    de["default"], de["host"] = a, b
    third = list(range(0, al["n"], 3))
    with ThreadPoolExecutor(16) as ex:
        al["oracle"] = dict(zip(third, ex.map(lambda i: sage_oracle.align_trace(al["profs"][i], al["wins"][i], SC, 50, 50), third)))
        third = list(range(0, nd, 3))
        de["oracle"] = dict(zip(third, ex.map(lambda i: indigo_oracle.decompose_trace(d["signal"][i], d["bcpos"][i], d["primary"][i].tobytes(),
                                                                                       d["secondary"][i].tobytes(), de["refs"][i], SC), third)))
    return out


def equals_oracle(which, pool, got):
    for i, w in pool["oracle"].items():
        if which == "align":
            for k in ("forward", "score_fwd", "score_rev", "slice_begin", "slice_len", "ref_pos"):
                assert int(got[k][i]) == int(w[k]), (i, k)
            assert got["btr"][i] == w["btr"], i
        else:
            assert int(got["status"][i]) == w["status"], i
            if w["status"] != 0:  # (strings of a trace that is not decomposed are not compared anywhere: test_gpu_stream.py)
                continue
            for k in ("btr0", "btr1", "btr2", "primary", "secondary", "dcp"):
                assert got[k][i] == w[k], (i, k)


# ---- 1. what the pools hold ---------------------------------------------------------------------------------------------------------
def test_pools_reach_every_list_of_both_kinds(pools):
    """over the two pools some trace files a pair under every [kind][list] -- except what IMPOSSIBLE names, which stays 0"""
    total = np.zeros((2, 4), np.int64)
    for which, pool in pools.items():
        mine = sum(s["lists"] for s in pool["single"])
        print("%s pool: %d traces, %d with a fallback alone; pairs [traceback / origin sweep][12, 8, 4, quad] = %s" %
              (which, pool["n"], sum(s["fallback"] > 0 for s in pool["single"]), mine.tolist()))
        total += mine
    for k in range(2):
        for b in range(4):
            if (k, b) in IMPOSSIBLE:
                assert total[k][b] == 0, (KINDS[k], LISTS[b], IMPOSSIBLE[(k, b)])
            else:
                assert total[k][b] > 0, (KINDS[k], LISTS[b], total.tolist())


# ---- 2. the large form equals the one-launch form, the host-planned pipeline and the oracle --------------------------------------
@pytest.mark.parametrize("no_quads", [0, 1])
@pytest.mark.parametrize("no_fork", [0, 1])
@pytest.mark.parametrize("which", ["align", "decompose"])
def test_large_form_equals_one_launch_host_planned_and_oracle(ctx, pools, which, no_fork, no_quads):
    pool = pools[which]
    idx = range(pool["n"])
    run = lambda: RUN[which](ctx, pool, idx)  # noqa: E731
    with_quads = RUN[which](ctx, pool, idx)[1]["band_list_pairs"] if no_quads else None
    ctx.set_option("no_fork", no_fork)
    ctx.set_option("no_quads", no_quads)
    try:
        big, sbig = large(ctx, which, pool, idx)
        one, sone = run()
    finally:
        ctx.set_option("no_fork", 0)
        ctx.set_option("no_quads", 0)
    assert sbig["stream_ordered"] == 1 and sone["stream_ordered"] == 1, (sbig, sone)
    assert sbig["band_large_launches"] == band_stages(which, no_fork) > 0 and sone["band_large_launches"] == 0, (sbig, sone)
    assert sbig["band_list_pairs"] == sone["band_list_pairs"], (sbig, sone)
    lists = np.asarray(sbig["band_list_pairs"])
    assert lists[:, 0].sum() > 0 and lists[:, 1:].sum() > 0, lists  # (the batch gives the separate launch and the other one work)
    if no_quads:
        wq = np.asarray(with_quads)
        assert wq[:, 3].sum() > 0 and lists[:, 3].tolist() == [0, 0], (wq, lists)
        assert (lists[:, 2] == wq[:, 2] + wq[:, 3]).all() and (lists[:, :2] == wq[:, :2]).all(), (wq, lists)
    same(which, big, one, "large form vs one launch")
    same(which, big, pool["default"], "large form vs the defaults")
    same(which, big, pool["host"], "large form vs host-planned")
    equals_oracle(which, pool, big)


# ---- 3. list sizes at the rounding edges of the grids ---------------------------------------------------------------------------
def members(pool, kind, lst, count):
    """`count` traces of the pool (repeated where it has fewer) that alone filed exactly one pair of `kind`, under list `lst`, and
    needed no fallback"""
    fit = [i for i, s in enumerate(pool["single"]) if s["fallback"] == 0 and s["lists"][kind].sum() == 1 and s["lists"][kind][lst] == 1
           and s["lists"][1 - kind].sum() == 1]
    assert fit or count == 0, (KINDS[kind], LISTS[lst])
    return [fit[j % len(fit)] for j in range(count)]


# pairs under strip height 12 / 8 / 4 / quad form in the origin-sweep stage of `tracy align` (one launch of it with no_early_tail)
EDGE_PLANS = [(0, 5, 1, 17),   # strip height 12 empty: band16_kernel<12> over a full grid with *count == 0; the other three end in a part workgroup
              (3, 0, 0, 0),    # strip height 12 alone: band16_multi3_counted_kernel has nothing
              (1, 1, 5, 15),   # 1 + 2 + 1 workgroups for 22 pairs
              (4, 4, 4, 16),   # whole workgroups only
              (5, 5, 5, 17),   # one pair over, everywhere
              (0, 1, 1, 1)]    # three workgroups for three pairs: the grid's ceil(3 / 4) + 3 spare ones, all used


@pytest.mark.parametrize("no_early_tail", [1, 0])
@pytest.mark.parametrize("plan", EDGE_PLANS)
def test_align_list_sizes_at_the_rounding_edges(ctx, pools, plan, no_early_tail):
    """sub-batches of the align pool whose origin-sweep lists have the planned sizes.  With no_early_tail the stage is ONE launch over
    all of them (otherwise the early traces' pairs and the others' go in two); the tracebacks of the same traces come as they come.
    A workgroup that took the wrong list, or was missing, leaves a pair's results untouched or wrong."""
    pool = pools["align"]
    idx = sum((members(pool, 1, b, plan[b]) for b in range(4)), [])
    idx = [idx[j] for j in np.random.default_rng(len(idx)).permutation(len(idx))]  # (lists are in unit order: interleave them)
    want = sum(pool["single"][i]["lists"] for i in idx)
    assert tuple(want[1]) == plan
    ctx.set_option("no_early_tail", no_early_tail)
    try:
        big, sbig = large(ctx, "align", pool, idx)
        one, sone = align_run(ctx, pool, idx)
    finally:
        ctx.set_option("no_early_tail", 0)
    assert sbig["stream_ordered"] == 1 and sbig["fallback_traces"] == 0, sbig
    assert sbig["band_large_launches"] == (2 if no_early_tail else 4) and sone["band_large_launches"] == 0, (sbig, sone)
    assert sbig["band_list_pairs"] == want.tolist() == sone["band_list_pairs"], (plan, sbig, sone)
    same_align(big, one, True, "large form vs one launch")
    for j, i in enumerate(idx):
        assert align_row(big, j) == pool["single"][i]["row"], (plan, j, i)


@pytest.mark.parametrize("with12", [False, True])
def test_decompose_lists_with_and_without_strip_height_12(ctx, pools, with12):
    """decompose traces that file nothing under strip height 12 (every stage's separate launch finds *count == 0), and traces that do
    beside three that do not: the counters are the sum of the traces' own, every field the trace's own result"""
    pool = pools["decompose"]
    ok = [i for i, s in enumerate(pool["single"]) if s["fallback"] == 0]
    tall = [i for i in ok if pool["single"][i]["lists"][:, 0].sum() > 0]
    flat = [i for i in ok if pool["single"][i]["lists"][:, 0].sum() == 0]
    assert tall and len(flat) >= 5, (tall, flat)
    idx = (tall[:6] + flat[:3]) if with12 else flat[:17]
    want = sum(pool["single"][i]["lists"] for i in idx)
    big, sbig = large(ctx, "decompose", pool, idx)
    one, sone = dec_run(ctx, pool, idx)
    assert sbig["stream_ordered"] == 1 and sbig["band_large_launches"] == 4 and sone["band_large_launches"] == 0, (sbig, sone)
    assert sbig["band_list_pairs"] == want.tolist() == sone["band_list_pairs"], (sbig, sone)
    assert (want[:, 0].sum() > 0) == with12
    same_decompose(big, one, "large form vs one launch")
    for j, i in enumerate(idx):
        assert dec_row(big, j) == pool["single"][i]["row"], (j, i)


# ---- 4. the threshold ---------------------------------------------------------------------------------------------------------------
def test_threshold_is_inclusive_and_per_stage(ctx, pools):
    """a stage of n units takes the one-launch form up to b16_multi_max = n and the large form from n - 1 down; the allele stages of
    `tracy decompose` have twice the units of its trace stages, so a value in between splits one call across both forms"""
    al, de = pools["align"], pools["decompose"]
    n = al["n"]
    for value, large in ((n, 0), (n - 1, band_stages("align", 0))):
        r, st = forced(ctx, value, lambda: align_run(ctx, al, range(n)))
        assert st["stream_ordered"] == 1 and st["band_large_launches"] == large, (value, st)
        same_align(r, al["default"], True, "b16_multi_max %d" % value)
    nd = de["n"]
    for value, large in ((2 * nd, 0), (2 * nd - 1, 2), (nd, 2), (nd - 1, 4)):
        r, st = forced(ctx, value, lambda: dec_run(ctx, de, range(nd)))
        assert st["stream_ordered"] == 1 and st["band_large_launches"] == large, (value, st)
        same_decompose(r, de["default"], "b16_multi_max %d" % value)


# ---- 5. both forms back to back on one context ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["align", "decompose"])
def test_forms_back_to_back_on_one_context(ctx, pools, which):
    """large, one launch, large over two different batches: a count word, an event or a side stream left over from the call before
    would show against a fresh context's results"""
    import tracy_amd
    pool = pools[which]
    batch_a = list(range(pool["n"]))
    batch_b = list(range(pool["n"] - 1, -1, -3)) * 2  # other traces in another order, another size
    got = [large(ctx, which, pool, batch_a), RUN[which](ctx, pool, batch_b), forced(ctx, 0, lambda: RUN[which](ctx, pool, batch_a))]
    assert [g[1]["band_large_launches"] for g in got] == [band_stages(which, 0), 0, band_stages(which, 0)], [g[1] for g in got]
    fresh = tracy_amd.Context(0)
    try:
        want_a, want_b = RUN[which](fresh, pool, batch_a)[0], RUN[which](fresh, pool, batch_b)[0]
    finally:
        fresh.close()
    same(which, got[0][0], want_a, "large form first")
    same(which, got[1][0], want_b, "one launch after the large form")
    same(which, got[2][0], want_a, "large form after one launch")
    assert got[0][1]["band_list_pairs"] == got[2][1]["band_list_pairs"]


# ---- 6. the option ----------------------------------------------------------------------------------------------------------------
def test_option_is_described_checked_and_read_from_the_environment(ctx, monkeypatch):
    import tracy_amd
    assert ctx.describe()["b16_multi_max"] == str(DEFAULT_MAX)
    try:
        ctx.set_option("b16_multi_max", 0)
        assert ctx.describe()["b16_multi_max"] == "0"
        ctx.set_option("B16_MULTI_MAX", 0x7fffffff)
        assert ctx.describe()["b16_multi_max"] == "2147483647"
        for bad in ("-1", "x", "", "12x", "2147483648"):
            with pytest.raises(tracy_amd.capi.TracyHipError):
                ctx.set_option("b16_multi_max", bad)
            assert ctx.describe()["b16_multi_max"] == "2147483647", bad
    finally:
        ctx.set_option("b16_multi_max", DEFAULT_MAX)
    monkeypatch.setenv("TRACYHIP_B16_MULTI_MAX", "77")
    c2 = tracy_amd.Context(0)
    monkeypatch.delenv("TRACYHIP_B16_MULTI_MAX")
    try:
        assert c2.describe()["b16_multi_max"] == "77" and ctx.describe()["b16_multi_max"] == str(DEFAULT_MAX)
    finally:
        c2.close()
