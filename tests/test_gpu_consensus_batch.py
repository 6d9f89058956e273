"""tracyhip_consensus_traces (the hot section of `tracy consensus` for a batch of trace pairs) against the oracle restatement
(consensus_oracle / pyoracle), field by field, and `tracy_amd_cli consensus --batch` against the two-file command, byte by byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tracy_amd", "bin", "tracy_amd_cli")
SCORE = (3, -5, -10, -4)


def column_profile(rng, seq, noise=0.06):
    """a trace-like profile of a base string: the called base carries most of each column, rows 4 (N) and 5 (gap) are zero"""
    n = len(seq)
    p = np.zeros((6, n), np.float32)
    w = rng.random((4, n), dtype=np.float32) * noise
    idx = np.array([b"ACGT".index(c) for c in seq])
    w[idx, np.arange(n)] += rng.uniform(0.75, 1.0, n).astype(np.float32)
    p[:4] = w / w.sum(0, keepdims=True)
    return p


def mutate(rng, seq, rate):
    s = bytearray(seq)
    for k in range(len(s)):
        if rng.random() < rate:
            s[k] = int(rng.choice(list(b"ACGT")))
    return bytes(s)


def make_pairs(seed, n, maxlen=700):
    """n pairs with ragged lengths (down to one column), both strands, some without enough overlap"""
    import pyoracle as orc
    rng = np.random.default_rng(seed)
    first, second, kinds = [], [], []
    for i in range(n):
        kind = i % 10
        if kind == 0:  # unrelated traces: NO_OVERLAP by match fraction
            a = bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(40, maxlen))).tolist())
            b = bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(40, maxlen))).tolist())
        elif kind == 1:  # tiny: 1 .. 30 columns (NO_OVERLAP by length at the default minimum)
            g = bytes(rng.choice(list(b"ACGT"), size=64).tolist())
            a = g[: int(rng.integers(1, 31))]
            b = g[int(rng.integers(0, 8)):][: int(rng.integers(1, 31))]
        else:
            L = int(rng.integers(60, maxlen))
            g = bytes(rng.choice(list(b"ACGT"), size=2 * L).tolist())
            s1 = int(rng.integers(0, L // 2))
            s2 = int(rng.integers(0, L // 2))
            a = mutate(rng, g[s1:s1 + L - int(rng.integers(0, L // 3))], 0.02)
            b = mutate(rng, g[s2:s2 + L - int(rng.integers(0, L // 3))], 0.02)
        p1 = column_profile(rng, a)
        p2 = column_profile(rng, b)
        if i % 2:  # the second trace read from the other strand
            p2 = np.ascontiguousarray(orc.revcomp_profile(p2))
        first.append(p1)
        second.append(p2)
        kinds.append(kind)
    return first, second


def oracle_pair(p1, f2, score, union, iupac, min_overlap, frac):
    import assemble_oracle as ao
    import consensus_oracle as co
    import pyoracle as orc
    r2 = np.ascontiguousarray(orc.revcomp_profile(f2))
    gf = orc.gotoh_score_prof(p1, f2, 1, 1, score)
    gr = orc.gotoh_score_prof(p1, r2, 1, 1, score)
    fwd = gf > gr
    p2 = f2 if fwd else r2
    sc, btr = orc.gotoh_prof(p1, np.ascontiguousarray(p2), 1, 1, score)
    row0, row1, _ = ao.rows_of(p1, p2, btr)
    aligned = sum(1 for a, b in zip(row0, row1) if a != "-" and b != "-")
    matches = sum(1 for a, b in zip(row0, row1) if a != "-" and b != "-" and a == b)
    ok = not (aligned < min_overlap or (matches / aligned if aligned else 0.0) < float(np.float32(frac)))
    cons, qual = co.pairwise_consensus(row0, row1, p1, p2, union, iupac) if ok else ("", [])
    return dict(score_fwd=gf, score_rev=gr, forward=int(fwd), score=sc, rows=(row0.encode(), row1.encode()), num_aligned=aligned,
                num_match=matches, status=0 if ok else 1, cons=cons.encode(), qual=list(qual))


def check_pair(got, i, want):
    for k in ("score_fwd", "score_rev", "forward", "score", "num_aligned", "num_match", "status"):
        assert int(got[k][i]) == int(want[k]), (i, k, int(got[k][i]), want[k])
    assert got["rows"][i] == want["rows"], i
    assert got["cons"][i] == want["cons"], i
    assert [int(q) for q in got["qual"][i]] == want["qual"], i


def check(got, first, second, score, union=True, iupac=False, min_overlap=25, frac=0.5, sample=None):
    idx = range(len(first)) if sample is None else sample
    for i in idx:
        check_pair(got, i, oracle_pair(first[i], second[i], score, union, iupac, min_overlap, frac))


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pairs():
    return make_pairs(2024, 240)


def test_batch_matches_oracle(ctx, pairs):
    first, second = pairs
    got = ctx.consensus_traces(first, second, SCORE)
    check(got, first, second, SCORE)
    st = got["status"]
    assert (st == 1).sum() >= 24 and (st == 0).sum() >= 150
    assert set(got["forward"].tolist()) == {0, 1}
    stats = ctx.last_call_stats()
    assert stats["traces"] == len(first) and stats["cons_chunks"] >= 1


@pytest.mark.parametrize("union,iupac", [(False, False), (True, True), (False, True)])
def test_union_intersect_iupac(ctx, pairs, union, iupac):
    first, second = pairs
    got = ctx.consensus_traces(first, second, SCORE, union=union, iupac=iupac)
    check(got, first, second, SCORE, union, iupac)


def test_nondefault_scoring_and_overlap(ctx, pairs):
    first, second = pairs
    score = (2, -3, -6, -2)
    got = ctx.consensus_traces(first, second, score, min_overlap=5, match_fraction=0.3)
    check(got, first, second, score, min_overlap=5, frac=0.3)


def test_device_memory_and_chunks(ctx, pairs):
    first, second = pairs
    got = ctx.consensus_traces(first, second, SCORE, iupac=True, device=True)
    check(got, first, second, SCORE, iupac=True)
    # a workspace limit that fits a few pairs at a time: the batch runs in chunks, same results
    ctx.set_workspace_limit(3 << 20)
    try:
        got2 = ctx.consensus_traces(first, second, SCORE, iupac=True)
        assert ctx.last_call_stats()["cons_chunks"] > 4
    finally:
        ctx.set_workspace_limit(0)
    for k in ("score_fwd", "score_rev", "forward", "score", "status", "num_aligned", "num_match"):
        assert np.array_equal(got[k], got2[k]), k
    assert got["rows"] == got2["rows"] and got["cons"] == got2["cons"]
    assert all(np.array_equal(a, b) for a, b in zip(got["qual"], got2["qual"]))


def test_async_and_zero_pairs(ctx, pairs):
    from tracy_amd import capi
    first, second = pairs
    p = capi.PreparedConsensus(first[:60], second[:60], SCORE)
    q = capi.PreparedConsensus(first[60:120], second[60:120], SCORE, union=False)
    ctx.consensus_traces_async(p.job, p.prm, p.out)
    ctx.consensus_traces_async(q.job, q.prm, q.out)
    ctx.synchronize()
    check(p.results(), first[:60], second[:60], SCORE)
    check(q.results(), first[60:120], second[60:120], SCORE, union=False)
    z = ctx.consensus_traces([], [], SCORE)
    assert len(z["cons"]) == 0


def test_bad_input(ctx):
    from tracy_amd import capi
    p1 = np.zeros((6, 0), np.float32)
    p2 = np.full((6, 5), 0.2, np.float32)
    with pytest.raises(capi.TracyHipError) as e:
        ctx.consensus_traces([p1], [p2], SCORE)
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.TracyHipError) as e:
        ctx.consensus_traces([p2], [p2], (40000, -5, -10, -4))
    assert e.value.code == capi.ERR_RANGE


# ---- the launch loops: runs of equal strip height and term count, sweeps of several passes, the repeat on int32 ----------

RUN_LENGTHS = (40, 250, 256, 257, 300, 512, 513, 600, 700, 120, 400, 800)  # columns of the first profile
N_FIRST, N_SECOND = (250, 300, 700), (40, 512, 600)                        # pairs whose first / second profile has a non-zero N row
WIDE = 4.0  # every column x 4.0: substitution scores x 16, range_verdict sees Q = (int)(4 * 4 * 5 * 1.0001 + 1) + 1 = 82


def strip_height(m):
    """choose_k for profile x profile (capi.hip): the cheaper of 8 and 4 rows per lane by passes x height, 8 on a tie"""
    return min((8, 4), key=lambda k: -(-m // (64 * k)) * k)


def passes(m):
    return -(-m // (64 * strip_height(m)))


def arith16_holds(mn, q):
    """arith16_ok (capi.hip) for scoring 3/-5/-10/-4 and a largest substitution score q"""
    return 3 * 10 + (mn + 2) * 4 + q < 20000 - 1000 and (mn // 2 + 1) * q < 30000


def with_n_row(rng, p, every=7):
    """half of every `every`-th column moved to row 4 ('N'): column sums stay 1"""
    p = p.copy()
    cols = np.arange(int(rng.integers(0, every)), p.shape[1], every)
    p[:4, cols] *= np.float32(0.5)
    p[4, cols] = np.float32(0.5)
    return p


def with_gap_row(rng, p, every=11):
    """half of every `every`-th column moved to row 5 (gap): column sums stay 1"""
    p = p.copy()
    cols = np.arange(int(rng.integers(0, every)), p.shape[1], every)
    p[:5, cols] *= np.float32(0.5)
    p[5, cols] = np.float32(0.5)
    return p


def make_runs(seed=913):
    import pyoracle as orc
    rng = np.random.default_rng(seed)
    first, second = [], []
    for i, L in enumerate(RUN_LENGTHS):
        g = bytes(rng.choice(list(b"ACGT"), size=2 * L).tolist())
        L2 = L - int(rng.integers(0, L // 8 + 1))
        p1 = column_profile(rng, mutate(rng, g[:L], 0.02))
        s2 = int(rng.integers(0, L // 4 + 1))
        p2 = column_profile(rng, mutate(rng, g[s2:s2 + L2], 0.02))
        if L in N_FIRST:
            p1 = with_n_row(rng, p1)
        if L in N_SECOND:
            p2 = with_n_row(rng, p2)
        if i % 2:  # the second trace read from the other strand
            p2 = np.ascontiguousarray(orc.revcomp_profile(p2))
        first.append(p1)
        second.append(p2)
    return first, second


@pytest.fixture(scope="module")
def runs():
    first, second = make_runs()
    want = [oracle_pair(a, b, SCORE, True, False, 25, 0.5) for a, b in zip(first, second)]
    return first, second, want


@pytest.fixture(scope="module")
def wide_runs(runs):
    first = [np.ascontiguousarray(p * np.float32(WIDE)) for p in runs[0]]
    second = [np.ascontiguousarray(p * np.float32(WIDE)) for p in runs[1]]
    want = [oracle_pair(a, b, SCORE, True, False, 25, 0.5) for a, b in zip(first, second)]
    return first, second, want


def test_the_runs_hold_every_case(runs, wide_runs):
    """asserted on the inputs and on the oracle's own results (no GPU): every case the launch loops can go wrong on is present.
    The rules of capi.hip are restated above: strip height 4 up to 256 rows, 8 up to 512, 4 again (three passes) up to 768, 8 (two
    passes) from 769 on; a pair takes the 16-term body iff row 4 of both profiles is zero."""
    first, second, want = runs
    assert [p.shape[1] for p in first] == list(RUN_LENGTHS)
    assert [strip_height(m) for m in (40, 256, 257, 512, 513, 768, 769, 800)] == [4, 4, 8, 8, 4, 4, 8, 8]
    assert [passes(m) for m in (256, 257, 512, 513, 700, 800)] == [1, 1, 1, 3, 3, 2]
    assert all(abs(a.shape[1] - b.shape[1]) <= a.shape[1] // 8 for a, b in zip(first, second))
    zero = lambda p: not p[4].any()
    terms = {(strip_height(a.shape[1]), zero(a) and zero(b)) for a, b in zip(first, second)}
    assert terms == {(4, True), (4, False), (8, True), (8, False)}                  # each strip height holds both term counts
    assert any(not zero(a) for a in first) and any(not zero(b) for b in second)     # an N row on either side
    for k in (4, 8):                                                                # one pass and several, at each strip height
        assert {passes(a.shape[1]) > 1 for a in first if strip_height(a.shape[1]) == k} == {False, True}
    assert any(passes(a.shape[1]) > 1 and not (zero(a) and zero(b)) for a, b in zip(first, second))  # boundary rows under the 25-term body
    assert {w["forward"] for w in want} == {0, 1} and sum(w["status"] == 0 for w in want) >= 10
    # the repeat on int32: Q = 82 where every column is x 4.0; a 16-bit launch is refused from m + n = 730 on and the batch lies on both
    # sides of it; a priori (Q = 5) every launch is narrow; the int32 kernels hold the values ((m + n + 2) (14 + Q) + 10^6 < 2^26)
    assert int(WIDE * WIDE * 5 * 1.0001 + 1.0) + 1 == 82  # range_verdict: column masses x largest |score| x 1.0001 + 1, rounded up
    assert arith16_holds(729, 82) and not arith16_holds(730, 82)
    mn = [a.shape[1] + b.shape[1] for a, b in zip(first, second)]
    assert min(mn) < 730 <= max(mn) and all(arith16_holds(x, 5) for x in mn)
    assert (max(mn) + 2) * (14 + 82) + 1000000 < 1 << 26
    assert all(np.array_equal(w, np.float32(WIDE) * p) for w, p in zip(wide_runs[0], first))


@pytest.mark.parametrize("option", [None, "no_fused_walk", "no_screen", "no_narrow"])
def test_runs_match_oracle(ctx, runs, option):
    first, second, want = runs
    if option:
        ctx.set_option(option, 1)
    try:
        got = ctx.consensus_traces(first, second, SCORE)
    finally:
        if option:
            ctx.set_option(option, 0)
    for i, w in enumerate(want):
        check_pair(got, i, w)
    assert ctx.last_call_stats()["host_syncs"] == 2  # the classes, the end


def test_runs_repeat_on_int32(ctx, runs, wide_runs):
    """un-normalised profiles: the first run's 16-bit score launches are refused by range_verdict at the end of the call (kWiden) and
    the call runs again on int32 -- twice the synchronisations of the unscaled call"""
    first, second, want = wide_runs
    ctx.consensus_traces(runs[0], runs[1], SCORE)
    plain = ctx.last_call_stats()["host_syncs"]
    got = ctx.consensus_traces(first, second, SCORE)
    syncs = ctx.last_call_stats()["host_syncs"]
    for i, w in enumerate(want):
        check_pair(got, i, w)
    assert (plain, syncs) == (2, 4)


# ---- the command line -------------------------------------------------------------------------------------------------


def run(args, cwd, timeout=600):
    return subprocess.run([CLI, "consensus"] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_cli_batch_matches_single_pair(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_cli import tiled_traces
    rng = np.random.default_rng(77)
    _, paths = tiled_traces(rng, str(tmp_path), 24, region_len=2400, tlen=420, noisy_ends=False)  # every third tile reversed
    (tmp_path / "other").mkdir()
    _, other = tiled_traces(np.random.default_rng(5), str(tmp_path / "other"), 1, region_len=500, tlen=420)
    jobs = [(paths[i], paths[i + 1]) for i in range(len(paths) - 1)]
    jobs.append((paths[0], other[0]))  # unrelated: not enough overlap
    single = tmp_path / "single"
    batch = tmp_path / "batch"
    single.mkdir()
    batch.mkdir()
    opts = ["-a", "-g", "-9", "-e", "-3"]
    rc_single = []
    for k, (a, b) in enumerate(jobs):
        r = run(opts + ["-o", str(single / ("p%02d" % k)), a, b], str(tmp_path))
        rc_single.append(r.returncode)
    assert rc_single[-1] == 1 and all(rc == 0 for rc in rc_single[:-1]), (rc_single, r.stderr[-2000:])
    man = tmp_path / "manifest.tsv"
    with open(man, "w") as f:
        f.write("# trace1\ttrace2\toutprefix\n")
        for k, (a, b) in enumerate(jobs):
            f.write("%s\t%s\t%s\n" % (a, b, batch / ("p%02d" % k)))
    r = run(opts + ["--batch", str(man)], str(tmp_path))
    assert r.returncode == 1, r.stderr[-2000:]  # one pair lacked overlap
    assert "No sufficient trace overlap" in r.stderr
    for k in range(len(jobs)):
        for ext in ("_1st.abif", "_2nd.abif", ".align.fa", ".fa", ".fq", ".txt"):
            s, b = single / ("p%02d%s" % (k, ext)), batch / ("p%02d%s" % (k, ext))
            assert s.exists() == b.exists(), (k, ext)
            if s.exists():
                assert s.read_bytes() == b.read_bytes(), (k, ext)
    assert not (batch / ("p%02d.fa" % (len(jobs) - 1))).exists()
    # an unwritable prefix: exit code 2, the other pairs are still written
    with open(man, "a") as f:
        f.write("%s\t%s\t%s\n" % (jobs[0][0], jobs[0][1], tmp_path / "no_such_dir" / "x"))
    r = run(opts + ["--batch", str(man)], str(tmp_path))
    assert r.returncode == 2, r.stderr[-2000:]
    assert (batch / "p00.fa").read_bytes() == (single / "p00.fa").read_bytes()
