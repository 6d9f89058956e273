"""The two scan launches of a band stage of the stream-ordered pipelines (tracy_amd/csrc/stream.hip: s_scan_count_kernel counts the
candidates of every block of 256 units per list with wave ballots, s_scan_place_kernel sums the blocks before its own and hands every
pair its place in its list and the offset of its traceback words).  What can go wrong is arithmetic at the edges -- a wave, a block,
the strided loop over the blocks' totals -- and the order of the lists, so the batches here have stage sizes at those edges, and every
result is compared with the host-planned pipeline (no_stream), which has no scan, and with the oracle.

The generators are those of test_gpu_band_large.py and test_gpu_early_tail.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_band_large import ALIGN_RATES, DEC_RATES, KINDS, LISTS, align_run, dec_run, mutate, sub_dec
from test_gpu_early_tail import ALIGN_KEYS, COMP, SC, same_align, short_traces
from test_gpu_stream import both_ways, decompose_both_ways, same_decompose

pytestmark = pytest.mark.gpu
SCAN_BLOCK = 256  # stream.hip kScanBlock


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def oracle_rows(profs, wins, which, cache=None, key=None):
    """sage_oracle.align_trace of the traces `which`; cache / key: results kept per key[i] (batches that repeat the traces of a pool)"""
    import sage_oracle as so
    cache = {} if cache is None else cache
    key = key if key is not None else list(range(len(profs)))
    todo = sorted({key[i]: i for i in which if key[i] not in cache}.items())
    with ThreadPoolExecutor(16) as ex:
        for (k, _), w in zip(todo, ex.map(lambda ki: so.align_trace(profs[ki[1]], wins[ki[1]], SC, 50, 50), todo)):
            cache[k] = w
    return [cache[key[i]] for i in which]


def equals_oracle(got, want, which):
    for i, w in zip(which, want):
        for k in ALIGN_KEYS:
            assert int(got[k][i]) == int(w[k]), (i, k)
        assert got["btr"][i] == w["btr"], i


# ---- 1. stage sizes at every edge of the scan's arithmetic -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_pool():
    """160 distinct traces: short ones (class 1: both strands in full, narrow bands) and plain ones of 900 rows whose windows carry
    more and more differences (wider bands: other lists); a batch of n units takes them in a fixed shuffled order, again and again"""
    from tracy_amd import hostlib
    rng = np.random.default_rng(4711)
    short = short_traces(rng, 120)
    refs, profs, _ = hostlib.synth_align(2024, 40, 3000, 900, 2)
    pool = {"profs": [s[0] for s in short] + [np.ascontiguousarray(profs[i]) for i in range(40)],
            "wins": [s[1] for s in short] + [mutate(rng, refs[i].tobytes(), ALIGN_RATES[i % len(ALIGN_RATES)]) for i in range(40)]}
    pool["order"] = [int(i) for i in rng.permutation(len(pool["profs"]))]
    pool["plain"] = list(range(len(short), len(pool["profs"])))
    pool["oracle"] = {}
    return pool


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_stage_sizes_at_the_edges_of_waves_and_blocks(ctx, mixed_pool, n):
    """one unit, a wave less / exactly / more than one, a block less / exactly / more than one, two and four blocks and a unit: every
    array and every traceback string is the host-planned pipeline's, and for sixteen traces of the batch the oracle's"""
    pool = mixed_pool
    idx = [pool["order"][(j + n) % len(pool["order"])] for j in range(n)]
    idx[0] = pool["plain"][n % len(pool["plain"])]  # (a call without a pruned sweep is planned by the host: plan_common)
    profs, wins = [pool["profs"][i] for i in idx], [pool["wins"][i] for i in idx]
    a, sa, b, sb = both_ways(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50))
    print("n = %d: lists [traceback / origin sweep][12, 8, 4, quad] = %s, fallback %d" % (n, sa["band_list_pairs"], sa["fallback_traces"]))
    assert sa["stream_ordered"] == 1 and sb["stream_ordered"] == 0, (sa, sb)
    lists = np.asarray(sa["band_list_pairs"])
    assert lists.sum() > 0
    if n >= 63:
        assert (lists.sum(axis=0) > 0).sum() >= 2, lists  # several lists at once: their members interleave in unit order
    same_align(a, b, True, "n = %d: stream-ordered vs host-planned" % n)
    which = sorted(int(i) for i in np.random.default_rng(n).choice(n, size=min(n, 16), replace=False))
    equals_oracle(a, oracle_rows(profs, wins, which, pool["oracle"], idx), which)


# ---- 2. more blocks than the place kernel has threads: the loop over the blocks' totals runs twice -----------------------------------
def tiny_traces(rng, count, lo=90, hi=110):
    """(profile, window): lo to hi - 1 bases between two flanks, every other one on the reverse strand; for trims 0 / 0.  About the 100
    rows of test_gpu_early_tail.short_traces: class 1, both strands in full, and an origin sweep and a final alignment on the bands"""
    from test_gpu_front import noisy, profile_of, rand_seq
    out = []
    for it in range(count):
        seq = rand_seq(rng, int(rng.integers(lo, hi)))
        win = rand_seq(rng, int(rng.integers(20, 60))) + noisy(rng, seq, float(rng.choice([0.0, 0.03]))) + rand_seq(rng, int(rng.integers(20, 60)))
        if it % 2:
            win = win.translate(COMP)[::-1]
        out.append((profile_of(rng, seq), win))
    return out


def test_one_call_of_258_blocks_equals_two_calls_of_half_the_size(ctx):
    """66 000 units are 258 blocks: block 257 sums 257 totals, one more than the place kernel has threads, so its strided loop takes a
    second round (65 537 units, 257 blocks, would still be one round: block 256 sums 256 totals).  A wrong base shifts every pair of a
    block in its list or moves its traceback words onto another pair's; the two halves have 129 blocks each and bases of their own."""
    n = 66000
    assert (n + SCAN_BLOCK - 1) // SCAN_BLOCK - 1 > SCAN_BLOCK
    rng = np.random.default_rng(258)
    tiny = tiny_traces(rng, 96) + tiny_traces(rng, 4, 300, 340)  # (a few with rows below the prefix: some trace must take the pruned sweep, plan_common)
    pick = rng.integers(0, len(tiny), size=n)
    pick[::1000] = 96 + np.arange(len(pick[::1000])) % 4  # in both halves
    profs, wins = [tiny[i][0] for i in pick], [tiny[i][1] for i in pick]
    whole = ctx.align_traces(profs, wins, SC, 0, 0)
    s = ctx.last_call_stats()
    print("whole: lists %s prelim_banded %d final_banded %d fallback %d" % (s["band_list_pairs"], s["prelim_banded"], s["final_banded"], s["fallback_traces"]))
    assert s["stream_ordered"] == 1, s
    lists = np.asarray(s["band_list_pairs"])
    # the blocks behind the 257th hold pairs of both stages: nearly every unit is a candidate
    assert lists[1].sum() >= n - n // 20 and lists[0].sum() >= n - n // 20, s
    h = n // 2
    halves, hlists = [], np.zeros((2, 4), np.int64)
    for lo, hi in ((0, h), (h, n)):
        halves.append(ctx.align_traces(profs[lo:hi], wins[lo:hi], SC, 0, 0))
        hlists += np.asarray(ctx.last_call_stats()["band_list_pairs"])
    assert lists.tolist() == hlists.tolist()
    for k in ALIGN_KEYS:
        both = np.concatenate([halves[0][k], halves[1][k]])
        assert np.array_equal(whole[k], both), (k, np.nonzero(whole[k] != both)[0][:8])
    assert whole["btr"] == halves[0]["btr"] + halves[1]["btr"]


# ---- 3. all four lists of both kinds: sizes and statistics --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def list_pools(ctx):
    """the align pool and the decompose pool of test_gpu_band_large.py (the same generators, seeds and rates), with the lists every
    trace files when it runs alone -- a stage of one unit, where the scan has nothing to add up"""
    from test_gpu_front import cases
    from tracy_amd import hostlib
    rng = np.random.default_rng(2026)
    ns = 40
    refs, profs, _ = hostlib.synth_align(2024, ns, 3000, 900, 2)
    front = cases(np.random.default_rng(77))[:24]
    al = {"profs": [np.ascontiguousarray(profs[i]) for i in range(ns)] + [c[0] for c in front],
          "wins": [mutate(rng, refs[i].tobytes(), ALIGN_RATES[i % len(ALIGN_RATES)]) for i in range(ns)] + [c[1] for c in front]}
    nd = 64
    d = hostlib.synth_decompose_batch(4242, nd, 2600, 900, 0, mix=1)
    de = {"d": d, "refs": [mutate(rng, d["refs"][i].tobytes(), DEC_RATES[i % len(DEC_RATES)]) for i in range(nd)]}
    al["n"], de["n"] = ns + len(front), nd
    for pool, run in ((al, align_run), (de, dec_run)):
        alone = [run(ctx, pool, [i])[1] for i in range(pool["n"])]
        pool["alone"] = sum(np.asarray(st["band_list_pairs"], np.int64) for st in alone)
        pool["alone_banded"] = sum(np.asarray(banded(st), np.int64) for st in alone)
    return {"align": al, "decompose": de}


def banded(st):
    return [st["prelim_banded"], st["final_banded"]] + st["allele_banded"]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("no_quads", [0, 1])
def test_list_sizes_and_statistics_of_all_four_lists(ctx, list_pools, no_quads, lanes):
    """the two pools file pairs under every list of both kinds.  The sizes the scan reports, and prelim_banded / final_banded /
    allele_banded, are the sum of what the traces report alone (without the quad form: its pairs under strip height 4), and every
    result is the host-planned pipeline's -- with the quad form and without, on one lane and on two.

    The host-planned pipeline's own prelim_banded / final_banded / allele_banded are printed, not compared: its tiers count their own
    launches (measured on the align pool: 0 / 62 where the stream-ordered call reports 49 / 49; decompose pool: allele_banded
    58 / 52 / 64 against 52 / 52 / 52), with the three-launch scan as with this one: the planning kernels that count are the same."""
    al, de = list_pools["align"], list_pools["decompose"]
    assert ((al["alone"] + de["alone"]) > 0).all(), (al["alone"], de["alone"])
    ctx.set_option("no_quads", no_quads)
    ctx.set_lanes(lanes)
    try:
        a, sa, b, sb = both_ways(ctx, lambda: ctx.align_traces(al["profs"], al["wins"], SC, 50, 50, device=lanes > 1))
        da, dsa, db, dsb = decompose_both_ways(ctx, *sub_dec(de, range(de["n"])), de["n"])
    finally:
        ctx.set_lanes(1)
        ctx.set_option("no_quads", 0)
    for which, pool, s, h in (("align", al, sa, sb), ("decompose", de, dsa, dsb)):
        print("%s, no_quads %d, lanes %d: lists [%s][%s] = %s; banded %s / host-planned %s" %
              (which, no_quads, lanes, " / ".join(KINDS), ", ".join(LISTS), s["band_list_pairs"],
               banded(s), banded(h)))
        assert s["stream_ordered"] == 1 and h["stream_ordered"] == 0, (which, s, h)
        want = pool["alone"].copy()
        if no_quads:
            want[:, 2] += want[:, 3]
            want[:, 3] = 0
        assert np.asarray(s["band_list_pairs"]).tolist() == want.tolist(), (which, s["band_list_pairs"], want)
        assert banded(s) == pool["alone_banded"].tolist(), (which, banded(s), pool["alone_banded"])
    same_align(a, b, True, "align pool: stream-ordered vs host-planned")
    same_decompose(da, db, "decompose pool: stream-ordered vs host-planned")


# ---- 4. pairs whose traceback words do not fit the workspace (SD_MEM) -----------------------------------------------------------------
def band_words_cap(rows, npairs, budget_left):
    """stream.hip band_words_cap"""
    return max(min(rows * 131 + npairs * 10240, budget_left // 2), 1 << 20)


def test_pairs_past_the_workspace_take_the_host_planned_tiers(ctx):
    """64 traces of 900 rows under a workspace limit of 3 MiB.  The cap of the final alignments' words is band_words_cap(rows, 64, limit -
    fixed) with 0 <= fixed <= limit (stream-ordered at all: fixed <= limit), so between 1 MiB and 1.5 MiB whatever `fixed` is.  A final
    alignment has at least 65 diagonals (s_final_band: w >= 32), and b16_store_words gives at least strips x window words: per row 70 / 4
    words of 2 bytes (strip height 4), 72 / 8 of 4 (8) or 78 / 12 of 8 (12) -- 35 bytes a row at least, and at most the planner's 131 a
    row + 10 240.  So the first pairs fit (not all are dropped) and the 64 do not (at least 64 - 1.5 MiB / (35 x 900) are).  The pass is
    one launch (no_early_tail): the offsets run through all 64."""
    from tracy_amd import hostlib
    n, mf, limit = 64, 900, 3 << 20
    cap_lo, cap_hi = band_words_cap(n * mf, n, 0), band_words_cap(n * mf, n, limit)
    assert (cap_lo, cap_hi) == (1 << 20, limit // 2)
    pair_lo, pair_hi = 35 * mf, 131 * mf + 10240
    assert pair_hi <= cap_lo  # the first pair fits
    assert n * pair_lo > cap_hi  # not all of them do
    dropped_at_least = n - cap_hi // pair_lo
    assert 1 <= dropped_at_least < n
    refs, profs, rev = hostlib.synth_align(77, n, 1200, mf, 2)
    profs, wins = list(profs), [r.tobytes() for r in refs]
    ctx.set_workspace_limit(limit)
    ctx.set_option("no_early_tail", 1)
    try:
        got = ctx.align_traces(profs, wins, SC, 50, 50)
        s = ctx.last_call_stats()
    finally:
        ctx.set_option("no_early_tail", 0)
        ctx.set_workspace_limit(0)
    print("limit %d: fallback %d (at least %d by the formula), lists %s, final_banded %d" %
          (limit, s["fallback_traces"], dropped_at_least, s["band_list_pairs"], s["final_banded"]))
    assert s["stream_ordered"] == 1, s
    assert np.asarray(s["band_list_pairs"])[0].sum() == n, s  # every final alignment was a candidate: the lists stay dense
    assert n > s["fallback_traces"] >= dropped_at_least, s
    equals_oracle(got, oracle_rows(profs, wins, range(n)), range(n))
    assert [int(x) for x in got["forward"]] == [1 - int(r) for r in rev]


# ---- 5. the shape of the prefix rows beside the full sweeps ---------------------------------------------------------------------------
@pytest.mark.parametrize("mf", [1000, 1100])
@pytest.mark.parametrize("exact", [True, False])
def test_headline_shape_in_miniature_with_either_prefix_shape(ctx, exact, mf):
    """test_gpu_early_tail.test_headline_shape_in_miniature with the voted strands' prefix rows as eight lanes of sixteen rows (the
    default beside the full sweeps; with strand_by_certificate only through prefix_tall_min = 0) and as sixteen lanes of eight rows
    (no_prefix_tall_beside: the threshold, which 128 pairs do not reach): the same arrays and strings, with the early tail, without it
    and on the host-planned pipeline.  mf = 1 100: 1 000 rows after the trims, so the full sweeps take strips of sixteen rows."""
    from test_gpu_early_tail import three_ways
    from tracy_amd import hostlib
    assert ctx.describe()["prefix_tall_min"] == "40000" and ctx.describe()["no_prefix_tall_beside"] == "0"
    refs, profs, rev = hostlib.synth_align(311, 128, 4000, mf, 2)
    assert 961 <= mf - 100 <= 1024 or mf == 1000
    refl = [r.tobytes() for r in refs]
    run = lambda: ctx.align_traces(list(profs), refl, SC, 50, 50, exact_scores=exact)  # noqa: E731
    got = {}
    for what, opts in (("tall beside the sweeps", {}), ("eight rows", {"no_prefix_tall_beside": 1}), ("tall everywhere", {"prefix_tall_min": 0})):
        for k, v in opts.items():
            ctx.set_option(k, v)
        try:
            got[what], s_early, s_late, _ = three_ways(ctx, run, exact)
        finally:
            ctx.set_option("no_prefix_tall_beside", 0)
            ctx.set_option("prefix_tall_min", 40000)
        if mf == 1000:  # (the batch of test_headline_shape_in_miniature, and what it asserts)
            assert s_early["fallback_traces"] == 0 and s_early["pruned"] == 128 and s_early["final_banded"] == 128, (what, s_early)
    for what in got:
        same_align(got[what], got["eight rows"], exact, what + " vs eight rows")
    assert [int(x) for x in got["eight rows"]["forward"]] == [1 - int(r) for r in rev]
    for bad in ("-1", "x", "", "2147483648"):
        with pytest.raises(Exception):
            ctx.set_option("prefix_tall_min", bad)
        assert ctx.describe()["prefix_tall_min"] == "40000", bad
