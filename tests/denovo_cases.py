"""Inputs and oracle results of the batched de novo assembly (tracyhip_denovo_traces), shared by tests/test_denovo_cases.py,
tests/test_emu_denovo.py and tests/test_gpu_denovo_batch.py.  The oracle is msa_oracle.rev_seq_based_on_dist, the overlap filter of
assemble_oracle.assemble_denovo restated over profiles, msa_oracle.upgma / palign / consensus, all over pyoracle's Gotoh.  Every
group kind is seeded; test_denovo_cases.py asserts on the oracle's own results that the inputs hold the cases they are named for."""
import functools

import numpy as np

import msa_oracle as mo
import pyoracle as orc
from test_gpu_assemble_batch import bases, column_profile, mutate

SCORE = (3, -5, -10, -4)
CALLED = 0.1
FRACTIONS = (0.5, 0.75)
NONE = 0xffffffff
WIDE = 4.0
KINDS = ("tiled5", "tiled7", "pairs4", "stranger", "lonely", "dup", "short", "cross64", "cross256", "longleft", "ncols", "empty", "one", "long2")
# longleft: (start, columns) and substitution rate of five traces over 700 columns.  Traces 0, 1, 2 span 520 columns with overlaps of
# 130 each; trace 3 overlaps trace 2 by 50 only and traces 3, 4 are noisier reads, so that UPGMA joins 0, 1, 2 before it joins (3, 4):
# the root's left child is the node of three traces (with clean reads no tiling of 200 .. 260 columns over 700 gives that order)
LONGLEFT = ((0, 260), (130, 260), (260, 260), (470, 230), (450, 200))
LONGLEFT_NOISE = (0.02, 0.02, 0.02, 0.1, 0.15)


def revcomp(p):
    return np.ascontiguousarray(orc.revcomp_profile(p))


def tiled(rng, n, tlen, region_len, reverse=(), rate=0.02):
    region = bases(rng, region_len)
    out = []
    for i in range(n):
        st = int(i * (region_len - tlen) / max(n - 1, 1))
        p = column_profile(rng, mutate(rng, region[st:st + tlen], rate))
        out.append(revcomp(p) if i in reverse else p)
    return out


def with_n_columns(p):
    """weight in row 4 on every ninth column, heavier than the called base (test_gpu_assemble_batch.make_long_groups)"""
    p = p.copy()
    cols = np.arange(3, p.shape[1], 9)
    p[:4, cols] *= np.float32(0.5)
    p[4, cols] = np.float32(0.5)
    return p


def make_group(kind):
    rng = np.random.default_rng(9000 + KINDS.index(kind))
    if kind == "tiled5":
        return tiled(rng, 5, 180, 420, reverse=(1, 4))
    if kind == "tiled7":
        return tiled(rng, 7, 200, 600, reverse=(2, 5))
    if kind == "pairs4":
        region = bases(rng, 300)
        halves = (region[:150], region[150:])
        return [column_profile(rng, mutate(rng, halves[i // 2], 0.02)) for i in range(4)]
    if kind == "stranger":
        g = tiled(rng, 3, 150, 300)
        g.insert(1, column_profile(rng, bases(rng, 160)))
        return g
    if kind == "lonely":
        return [column_profile(rng, bases(rng, 120)), column_profile(rng, bases(rng, 140))]
    if kind == "dup":
        p = column_profile(rng, bases(rng, 90))
        return [p, p.copy(), p.copy()]
    if kind == "short":
        region = bases(rng, 60)
        return [column_profile(rng, region[0:40]), column_profile(rng, region[20:60]), column_profile(rng, region[34:60])]
    if kind == "cross64":
        return tiled(rng, 2, 60, 90)
    if kind == "cross256":
        return tiled(rng, 3, 270, 400, reverse=(1,))
    if kind == "longleft":
        region = bases(rng, 700)
        return [column_profile(rng, mutate(rng, region[st:st + ln], rate)) for (st, ln), rate in zip(LONGLEFT, LONGLEFT_NOISE)]
    if kind == "ncols":
        g = tiled(rng, 3, 150, 260)
        g[1] = with_n_columns(g[1])
        return g
    if kind == "empty":
        return []
    if kind == "one":
        return [column_profile(rng, bases(rng, 77))]
    if kind == "long2":
        return tiled(rng, 2, 400, 600)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def groups():
    return tuple(make_group(k) for k in KINDS)


def strand_table(traces, score=SCORE):
    """T[i][j][oi][oj] = gotohScore(strand oi of trace i as a1, strand oj of trace j as a2), int32 [K][K][2][2] (the diagonal is 0)"""
    K = len(traces)
    both = [(p, revcomp(p)) for p in traces]
    T = np.zeros((K, K, 2, 2), np.int32)
    for i in range(K):
        for j in range(K):
            if i != j:
                for oi in range(2):
                    for oj in range(2):
                        T[i, j, oi, oj] = orc.gotoh_score_prof(both[i][oi], both[j][oj], 1, 1, score)
    return T


def strands_from_table(T):
    """msa_oracle.rev_seq_based_on_dist with every score read from the table -> (rev flags, final matrix)"""
    K = T.shape[0]
    rev = [0] * K
    d = [[0] * K for _ in range(K)]
    total = 0
    for i in range(K):
        for j in range(i + 1, K):
            d[i][j] = d[j][i] = int(T[i, j, 0, 0])
            total += d[i][j]
    while True:
        quality = sorted((sum(d[i]), i) for i in range(K))
        for _, who in quality:
            new = [0] * K
            ssum = old = 0
            for i in range(K):
                if i != who:
                    new[i] = int(T[i, who, rev[i], 1 - rev[who]])
                    old += d[i][who]
                    ssum += new[i]
            if ssum >= old:
                rev[who] ^= 1
                for i in range(K):
                    d[i][who] = d[who][i] = new[i]
        updated = sum(sum(r) for r in d)
        if total < updated:
            total = updated
        else:
            break
    return rev, d


def overlap_threshold(na, fracmatch, score):
    """assemble.h:441 as tests/assemble_oracle.py:186 restates it: int x float products, a float sum, then promoted"""
    f32 = np.float32
    return float(f32(f32(f32(na) * f32(fracmatch)) * f32(score[0])) + f32(f32(f32(na) * (f32(1) - f32(fracmatch))) * f32(score[1])))


def overlap_ok(na, gs, size, fracmatch, score):
    return na / float(size) > 0.1 and na > 25 and gs > overlap_threshold(na, fracmatch, score)


def tree_heights(p, num, root):
    h = [-1] * len(p)
    for i in range(num):
        h[i] = 0
    for i in range(num, root + 1):
        if p[i][1] >= 0 and p[i][2] >= 0:
            h[i] = max(h[p[i][1]], h[p[i][2]]) + 1
    return h


def oracle_group(traces, fracmatch, score=SCORE, called=CALLED):
    K = len(traces)
    profs, fwdp = mo.rev_seq_based_on_dist(list(traces), score)
    res = dict(forward=[int(f) for f in fwdp], partner=[NONE] * K, row=[NONE] * K, tries=[0] * K, profs=profs)
    keep = []
    for i in range(K):
        for j in range(K):
            if i == j:
                continue
            res["tries"][i] += 1
            gs, btr = orc.gotoh_prof(profs[i], profs[j], 1, 1, score)
            if overlap_ok(btr.count(b"s"), gs, profs[i].shape[1], fracmatch, score):
                res["partner"][i] = j
                keep.append(i)
                break
    res["keep"] = keep
    res["rounds"] = max(res["tries"]) if K else 0
    if len(keep) < 2:
        res.update(nrows=0, ncol=0, rows=[], gapped=b"", cons=b"", qual=b"", heights=0, tree=None)
        return res
    sps = [np.ascontiguousarray(profs[i]) for i in keep]
    num = len(sps)
    d = [[-1] * (2 * num + 1) for _ in range(2 * num + 1)]
    for a in range(num):
        for b in range(a + 1, num):
            d[a][b] = orc.gotoh_score_prof(sps[a], sps[b], 1, 1, score)
    dist = [r[:num] for r in d[:num]]
    root, p = mo.upgma(d, num)
    rows, _, sidx = mo.palign(sps, p, root, score)
    for r, s in enumerate(sidx):
        res["row"][keep[s]] = r
    gapped, cs, qs = mo.consensus(rows, called, False)
    h = tree_heights(p, num, root)
    res.update(nrows=len(rows), ncol=len(rows[0]), rows=[r.encode() for r in rows], gapped=gapped.encode(), cons=cs.encode(), qual=qs.encode(),
               heights=h[root], tree=dict(num=num, root=root, p=p, height=h, dist=dist, sps=sps, sidx=sidx))
    return res


@functools.lru_cache(maxsize=None)
def oracle(fracmatch):
    return tuple(oracle_group(g, fracmatch) for g in groups())


def scaled(profiles):
    return [np.ascontiguousarray(p * np.float32(WIDE)) for p in profiles]


WIDE_KINDS = ("longleft", "ncols", "long2")


@functools.lru_cache(maxsize=None)
def wide():
    """the groups of WIDE_KINDS with every profile x 4.0, and the oracle's results on them"""
    gs = tuple(scaled(groups()[KINDS.index(k)]) for k in WIDE_KINDS)
    return gs, tuple(oracle_group(g, 0.5) for g in gs)


def expected_syncs(want):
    """the formula of include/tracy_hip.h for ONE chunk: classes, table, the rounds of the slowest trace, the tallest tree, the end"""
    return 2 + max(w["rounds"] for w in want) + max(w["heights"] for w in want) + 1


def check(got, want, grps):
    """every group, every field"""
    t = 0
    for g, w in enumerate(want):
        for i in range(len(grps[g])):
            for k in ("forward", "partner", "row"):
                assert int(got[k][t]) == int(w[k][i]), (g, i, k, int(got[k][t]), w[k][i])
            t += 1
        assert int(got["nrows"][g]) == w["nrows"], g
        assert int(got["ncol"][g]) == w["ncol"], g
        assert got["rows"][g] == w["rows"], g
        assert got["gapped"][g] == w["gapped"], g
        assert got["cons"][g] == w["cons"] and int(got["cons_len"][g]) == len(w["cons"]), g
        assert got["qual"][g] == w["qual"], g
