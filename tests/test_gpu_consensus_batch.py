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


def check(got, first, second, score, union=True, iupac=False, min_overlap=25, frac=0.5, sample=None):
    idx = range(len(first)) if sample is None else sample
    for i in idx:
        want = oracle_pair(first[i], second[i], score, union, iupac, min_overlap, frac)
        for k in ("score_fwd", "score_rev", "forward", "score", "num_aligned", "num_match", "status"):
            assert int(got[k][i]) == int(want[k]), (i, k, int(got[k][i]), want[k])
        assert got["rows"][i] == want["rows"], i
        assert got["cons"][i] == want["cons"], i
        assert [int(q) for q in got["qual"][i]] == want["qual"], i


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
