"""tracyhip_assemble_traces (the reference-guided chain of `tracy assemble -r` for a batch of trace groups) against the chain of
tests/assemble_oracle.py::assemble_ref_guided restated over profiles (pyoracle / msa_oracle), every group and every field, and
`tracy_amd_cli assemble -r --batch` against the one-group command, byte by byte."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tracy_amd", "bin", "tracy_amd_cli")
SCORE = (3, -5, -10, -4)
FRACMATCH, CALLED = 0.5, 0.1
KS = (1, 2, 3, 5, 8)


def column_profile(rng, seq, noise=0.06):
    """a trace-like profile of a base string (test_gpu_consensus_batch.py::column_profile): the called base carries most of each
    column, rows 4 (N) and 5 (gap) are zero"""
    n = len(seq)
    p = np.zeros((6, n), np.float32)
    w = rng.random((4, n), dtype=np.float32) * noise
    idx = np.array([b"ACGT".index(c) for c in seq])
    w[idx, np.arange(n)] += rng.uniform(0.75, 1.0, n).astype(np.float32)
    p[:4] = w / w.sum(0, keepdims=True)
    return p


def bases(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).tolist())


def mutate(rng, seq, rate):
    s = bytearray(seq)
    for k in range(len(s)):
        if rng.random() < rate:
            s[k] = int(rng.choice(list(b"ACGT")))
    return bytes(s)


def make_groups(seed=4242, ngroups=40):
    """groups of K in {1, 2, 3, 5, 8} traces (1 .. 300 columns) over references of 50 .. 600 columns; the kinds the test asserts on
    the oracle's results are built in by construction"""
    import pyoracle as orc
    rng = np.random.default_rng(seed)
    groups, refs, kinds = [], [], []
    for g in range(ngroups):
        kind = ("plain", "excluded", "single", "tie", "insertion", "cross64", "cross256", "onecol")[g % 8]
        K = KS[g % len(KS)]
        nref = int(rng.integers(50, 601))
        if kind == "cross64":
            nref, K = 60, max(K, 2)
        elif kind == "cross256":
            nref, K = 250, max(K, 3)
        elif kind in ("tie", "insertion"):
            K = max(K, 3)
        elif kind == "single":
            K = min(K, 2)
        region = bases(rng, nref)
        traces = []
        for i in range(K):
            ln = int(rng.integers(20, min(nref, 300) + 1))
            st = int(rng.integers(0, nref - ln + 1))
            seq = mutate(rng, region[st:st + ln], 0.03)
            if kind == "excluded" or (kind == "single" and i == 1):
                seq = bases(rng, int(rng.integers(100, 301)))  # unrelated
            elif kind == "tie" and i == 2:
                traces.append(traces[0].copy())  # the same trace twice: equal scores, the input index orders them
                continue
            elif kind in ("insertion", "cross64", "cross256") and i >= 1:
                # a later (shorter, so lower-scoring) trace carrying bases the reference lacks
                ln = int(rng.integers(40, min(nref, 200) + 1))  # (flanks long enough that the gap beats a shifted half)
                st = int(rng.integers(0, nref - ln + 1))
                seq = region[st:st + ln]
                at = ln // 2
                seq = seq[:at] + bases(rng, 8 if kind != "cross256" else 10) + seq[at:]
            elif kind == "onecol" and i == 0:
                seq = region[nref // 2:nref // 2 + 1]
            p = column_profile(rng, seq)
            if (g + i) % 3 == 1:  # read from the other strand
                p = np.ascontiguousarray(orc.revcomp_profile(p))
            traces.append(p)
        if kind in ("insertion", "cross64", "cross256"):  # the best trace: the whole region, so that the inserted ones come later
            traces[0] = column_profile(rng, region[:min(nref, 300)])
        groups.append(traces)
        refs.append(orc.create_profile_str(region))
        kinds.append(kind)
    return groups, refs, kinds


def oracle_group(traces, pref, score, fracmatch, called, incref):
    """assemble_oracle.assemble_ref_guided from the profiles on"""
    import assemble_oracle as ao
    import msa_oracle as mo
    import pyoracle as orc
    f32 = np.float32
    res = dict(score_fwd=[], score_rev=[], forward=[], rank=[0xffffffff] * len(traces), steps=[])
    profiles, score_idx = [], []
    for i, p in enumerate(traces):
        rev = np.ascontiguousarray(orc.revcomp_profile(p))
        gf = orc.gotoh_score_prof(p, pref, 1, 0, score)
        gr = orc.gotoh_score_prof(rev, pref, 1, 0, score)
        res["score_fwd"].append(gf)
        res["score_rev"].append(gr)
        res["forward"].append(int(gf >= gr))
        size = float(p.shape[1])
        thr = size * float(f32(fracmatch)) * score[0] + size * float(f32(1) - f32(fracmatch)) * score[1]
        if gf > thr or gr > thr:
            score_idx.append(dict(score=max(gf, gr), idx=i, newidx=len(score_idx)))
            profiles.append(p if gf >= gr else rev)
    score_idx.sort(key=lambda s: (-s["score"], s["idx"]))
    for k, s in enumerate(score_idx):
        res["rank"][s["idx"]] = k
    res["order"] = score_idx
    if not score_idx:
        res.update(nrows=0, ncol=0, rows=[], gapped=b"", cons=b"", qual=b"")
        return res
    p0 = profiles[score_idx[0]["newidx"]]
    _, btr = orc.gotoh_prof(p0, pref, 1, 0, score)
    r0, r1, ops = ao.rows_of(p0, pref, btr)
    align = [r0, r1]
    res["steps"].append((ops, len(r0)))
    for s in score_idx[1:]:
        ap = np.ascontiguousarray(mo.profile_of_alignment(align))
        pn = profiles[s["newidx"]]
        _, btr = orc.gotoh_prof(pn, ap, 1, 0, score)
        new0, _, ops = ao.rows_of(pn, ap, btr)
        comb = [list(new0)] + [[] for _ in align]
        a = 0
        for op in ops:
            for k in range(len(align)):
                comb[k + 1].append(align[k][a] if op != "v" else "-")
            a += op != "v"
        align = ["".join(r) for r in comb]
        res["steps"].append((ops, len(align[0])))
    gapped, cs, qs = mo.consensus(align, called, not incref)
    res.update(nrows=len(align), ncol=len(align[0]), rows=[r.encode() for r in align], gapped=gapped.encode(), cons=cs.encode(), qual=qs.encode())
    return res


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    groups, refs, kinds = make_groups()
    want = {inc: [oracle_group(t, r, SCORE, FRACMATCH, CALLED, inc) for t, r in zip(groups, refs)] for inc in (False, True)}
    return groups, refs, kinds, want


def check(got, want, groups):
    t = 0
    for g, w in enumerate(want):
        for i in range(len(groups[g])):
            for k in ("score_fwd", "score_rev", "forward", "rank"):
                assert int(got[k][t]) == int(w[k][i]), (g, i, k, int(got[k][t]), w[k][i])
            t += 1
        assert int(got["nrows"][g]) == w["nrows"], g
        assert int(got["ncol"][g]) == w["ncol"], g
        assert got["rows"][g] == w["rows"], g
        assert got["gapped"][g] == w["gapped"], g
        assert got["cons"][g] == w["cons"] and int(got["cons_len"][g]) == len(w["cons"]), g
        assert got["qual"][g] == w["qual"], g


def same(a, b):
    for k in ("score_fwd", "score_rev", "forward", "rank", "nrows", "ncol", "cons_len"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("rows", "gapped", "cons", "qual"):
        assert a[k] == b[k], k


def test_the_inputs_hold_every_case(batch):
    """asserted on the oracle's own results: the test cannot pass on easy inputs"""
    groups, refs, kinds, want = batch
    w = want[False]
    assert len(groups) == 40 and {len(g) for g in groups} == set(KS)
    assert all(50 <= r.shape[1] <= 600 for r in refs) and all(1 <= p.shape[1] <= 300 for g in groups for p in g)
    assert any(x["nrows"] == 0 and len(groups[g]) > 1 for g, x in enumerate(w))            # every trace excluded
    assert any(x["nrows"] == 2 for x in w)                                                  # one matching trace
    assert any(x["nrows"] == 2 and len(groups[g]) == 2 for g, x in enumerate(w))            # ... beside an excluded one
    assert sum(1 for x in w for i, f in enumerate(x["forward"]) if not f and x["rank"][i] != 0xffffffff) >= 10  # reverse strand chosen
    ties = [x for x in w if any(a["score"] == b["score"] and a["idx"] < b["idx"] for a, b in zip(x["order"], x["order"][1:]))]
    assert ties                                                                             # equal scores: the input index decides
    assert any("v" in ops for x in w for ops, _ in x["steps"][1:])                          # old rows gain gap columns at a step k >= 1
    cross = lambda lim: any(a[1] <= lim < b[1] for x in w for a, b in zip(x["steps"], x["steps"][1:]))
    assert cross(64) and cross(256)                                                         # ncol crosses a round / four rounds between steps
    assert any(p.shape[1] == 1 and x["rank"][i] != 0xffffffff for g, x in enumerate(w) for i, p in enumerate(groups[g]))  # a one-column trace, matching
    assert max(x["nrows"] for x in w) == 9
    assert any(a["gapped"] != b["gapped"] for a, b in zip(want[False], want[True]))         # include_reference changes a consensus


@pytest.mark.parametrize("include_reference", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_batch_matches_oracle(ctx, batch, device, include_reference):
    groups, refs, kinds, want = batch
    got = ctx.assemble_traces(groups, refs, SCORE, FRACMATCH, CALLED, include_reference, device=device)
    check(got, want[include_reference], groups)
    stats = ctx.last_call_stats()
    assert stats["traces"] == sum(len(g) for g in groups) and stats["asm_chunks"] == 1 and stats["asm_steps"] == 8
    assert stats["host_syncs"] == 2 + 8 + 1  # classes, scores, one per chain step, the end


def test_async_and_chunks_give_the_same(ctx, batch):
    from tracy_amd import capi
    groups, refs, kinds, want = batch
    base = ctx.assemble_traces(groups, refs, SCORE, FRACMATCH, CALLED, False)
    p = capi.PreparedAssemble(groups[:20], refs[:20], SCORE, FRACMATCH, CALLED, False)
    q = capi.PreparedAssemble(groups[20:], refs[20:], SCORE, FRACMATCH, CALLED, True)
    ctx.assemble_traces_async(p.job, p.prm, p.out)
    ctx.assemble_traces_async(q.job, q.prm, q.out)
    ctx.synchronize()
    check(p.results(), want[False][:20], groups[:20])
    check(q.results(), want[True][20:], groups[20:])
    # a workspace limit that fits a few groups at a time: the batch runs in chunks of groups, same results
    ctx.set_workspace_limit(4 << 20)
    try:
        got = ctx.assemble_traces(groups, refs, SCORE, FRACMATCH, CALLED, False)
        stats = ctx.last_call_stats()
        assert stats["asm_chunks"] > 1 and stats["asm_steps"] > 8
        dev = ctx.assemble_traces(groups, refs, SCORE, FRACMATCH, CALLED, False, device=True)
    finally:
        ctx.set_workspace_limit(0)
    same(got, base)
    same(dev, base)


def test_shared_reference_empty_batch_and_bad_input(ctx, batch):
    from tracy_amd import capi
    groups, refs, kinds, want = batch
    # two groups on one reference through ref_index, a group without traces between them
    got = ctx.assemble_traces([groups[0], [], groups[0]], [refs[0]], SCORE, FRACMATCH, CALLED, ref_index=[0, 0, 0])
    assert got["rows"][0] == want[False][0]["rows"] and got["rows"][2] == want[False][0]["rows"] and int(got["nrows"][1]) == 0
    z = ctx.assemble_traces([], [], SCORE)
    assert len(z["rows"]) == 0
    with pytest.raises(capi.TracyHipError) as e:
        ctx.assemble_traces([[np.zeros((6, 0), np.float32)]], [refs[0]], SCORE)
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.TracyHipError) as e:
        ctx.assemble_traces([groups[0]], [refs[0]], (40000, -5, -10, -4))
    assert e.value.code == capi.ERR_RANGE


def run_traceless(ctx, p, symbol, device):
    """a prepared batch whose groups hold no trace, through `symbol` with nrows / ncol / cons_len prefilled where the call finds them;
    returns results() and the call's host_syncs"""
    import ctypes as C
    from tracy_amd import capi
    counts = ("nrows", "ncol", "cons_len")
    if device:
        import torch
        p.to_device()
        for k in counts:
            p.dres[k].fill_(0xa5)
        torch.cuda.synchronize()
    else:
        for k in counts:
            p.res[k][:] = 0xa5a5a5a5
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    capi._check(getattr(capi.lib(), symbol)(ctx._h, C.byref(p.job), C.byref(p.prm), mem, C.byref(p.out)))
    if device:
        torch.cuda.synchronize()
        p.from_device()
    else:
        assert all(int(x) == 0 for k in counts for x in p.res[k])
    return p.results(), ctx.last_call_stats()["host_syncs"]


@pytest.mark.parametrize("device", [False, True])
def test_a_batch_without_any_trace_clears_the_counts(ctx, batch, device):
    """[[], []] over two references: nrows / ncol / cons_len come back zero whatever they held, nothing else runs.  The call does
    not wait for the device over host arrays and waits once, behind its three clears, over device arrays: 0 and 1 are what the
    library reported for this call before the group plumbing of assemble and de novo became one copy."""
    from tracy_amd import capi
    groups, refs, kinds, want = batch
    got, syncs = run_traceless(ctx, capi.PreparedAssemble([[], []], refs[:2], SCORE, FRACMATCH, CALLED), "tracyhip_assemble_traces", device)
    for k in ("nrows", "ncol", "cons_len"):
        assert got[k].tolist() == [0, 0], k
    assert got["rows"] == [[], []] and got["gapped"] == [b"", b""] and len(got["rank"]) == 0
    assert syncs == (1 if device else 0)


# ---- the launch loops: long traces (sweeps of several passes), N rows (the 25-term body), the repeat on int32 ----------------

LONG_TRACES = (700, 520, 300, 130)  # columns, over a reference of 900
WIDE = 4.0


def strip_height(m):
    """choose_k for profile x profile (capi.hip): the cheaper of 8 and 4 rows per lane by passes x height, 8 on a tie"""
    return min((8, 4), key=lambda k: -(-m // (64 * k)) * k)


def passes(m):
    return -(-m // (64 * strip_height(m)))


def arith16_holds(mn, q):
    """arith16_ok (capi.hip) for scoring 3/-5/-10/-4 and a largest substitution score q"""
    return 3 * 10 + (mn + 2) * 4 + q < 20000 - 1000 and (mn // 2 + 1) * q < 30000


def make_long_groups(seed=77):
    import pyoracle as orc
    rng = np.random.default_rng(seed)
    # the long group: four traces over 900 columns, the second with N columns, the third read from the other strand
    region = bases(rng, 900)
    long_group = []
    for ln, st in zip(LONG_TRACES, (60, 330, 120, 700)):
        p = column_profile(rng, mutate(rng, region[st:st + ln], 0.02))
        if ln == 520:
            cols = np.arange(3, ln, 9)
            p[:4, cols] *= np.float32(0.5)
            p[4, cols] = np.float32(0.5)
        if ln == 300:
            p = np.ascontiguousarray(orc.revcomp_profile(p))
        long_group.append(p)
    # a reference that holds N bases: step 0 of this group takes the 25-term body
    nregion = bytearray(bases(rng, 400))
    for at in (50, 51, 200, 333):
        nregion[at] = ord("N")
    nregion = bytes(nregion)
    clean = nregion.replace(b"N", b"A")
    n_group = [column_profile(rng, mutate(rng, clean[st:st + ln], 0.02)) for ln, st in ((280, 20), (150, 180), (90, 300))]
    # a small group of the kind make_groups builds
    sregion = bases(rng, 200)
    s_group = [column_profile(rng, mutate(rng, sregion[st:st + ln], 0.03)) for ln, st in ((150, 10), (60, 120))]
    s_group[1] = np.ascontiguousarray(orc.revcomp_profile(s_group[1]))
    groups = [long_group, n_group, s_group]
    refs = [orc.create_profile_str(region), orc.create_profile_str(nregion), orc.create_profile_str(sregion)]
    return groups, refs


@pytest.fixture(scope="module")
def long_batch():
    groups, refs = make_long_groups()
    want = [oracle_group(t, r, SCORE, FRACMATCH, CALLED, False) for t, r in zip(groups, refs)]
    return groups, refs, want


def scaled(profiles):
    return [np.ascontiguousarray(p * np.float32(WIDE)) for p in profiles]


@pytest.fixture(scope="module")
def wide_batch(long_batch):
    """[0]: the same traces x 4.0 over the same references; [1]: the references x 4.0 as well"""
    groups, refs, _ = long_batch
    out = []
    for r in (refs, scaled(refs)):
        g = [scaled(t) for t in groups]
        out.append((g, r, [oracle_group(t, p, SCORE, FRACMATCH, CALLED, False) for t, p in zip(g, r)]))
    return out


def test_the_long_inputs_hold_every_case(long_batch, wide_batch):
    """asserted on the inputs and on the oracle's own results (no GPU).  The rules of capi.hip are restated above: strip height 4 up to
    256 rows, 8 up to 512, 4 again (three passes) up to 768; a pair takes the 16-term body iff row 4 of both profiles is zero, and
    only at step 0 (later steps align against the profile of the rows so far and always take the 25-term body)."""
    groups, refs, want = long_batch
    assert [p.shape[1] for p in groups[0]] == list(LONG_TRACES) and refs[0].shape[1] == 900
    assert [strip_height(m) for m in LONG_TRACES] == [4, 4, 8, 4] and [passes(m) for m in LONG_TRACES] == [3, 3, 1, 1]
    assert groups[0][1][4].any() and not any(groups[0][i][4].any() for i in (0, 2, 3)) and not refs[0][4].any()
    w = want[0]
    assert w["nrows"] == 5 and w["forward"] == [1, 1, 0, 1] and w["ncol"] >= 900    # all four match, the third on the other strand
    assert [s["idx"] for s in w["order"]] == [0, 1, 2, 3]                            # longest first: steps 0 and 1 sweep in three passes
    assert refs[1][4].any() and not any(p[4].any() for p in groups[1]) and want[1]["nrows"] == 4  # N in the reference only
    assert not refs[2][4].any() and want[2]["nrows"] == 3
    # the score launches hold runs of both strip heights and both term counts; so does step 0 (long: 16 terms, N reference: 25)
    zero = lambda p: not p[4].any()
    runs = {(strip_height(p.shape[1]), zero(p) and zero(refs[g])) for g, t in enumerate(groups) for p in t}
    assert runs == {(4, True), (4, False), (8, True), (8, False)}
    first = [groups[g][want[g]["order"][0]["idx"]] for g in range(3)]
    assert {(strip_height(p.shape[1]), zero(p) and zero(refs[g])) for g, p in enumerate(first)} == {(4, True), (8, False)}
    # the repeat on int32.  Traces x 4.0 over normalised references: range_verdict sees Q = (int)(4 * 1.001 * 5 * 1.0001 + 1) + 1 = 22, which
    # arith16_ok takes at every length here -- no repeat.  References x 4.0 as well: Q = 82, refused from m + n = 730 on -- a repeat.
    assert int(WIDE * 1.001 * 5 * 1.0001 + 1.0) + 1 == 22 and int(WIDE * WIDE * 5 * 1.0001 + 1.0) + 1 == 82
    mn = [p.shape[1] + refs[g].shape[1] for g, t in enumerate(groups) for p in t]
    assert all(arith16_holds(x, 5) and arith16_holds(x, 22) for x in mn)
    assert min(mn) < 730 <= max(mn) and not arith16_holds(730, 82) and arith16_holds(729, 82)
    bound = max(refs[g].shape[1] + sum(p.shape[1] for p in t) for g, t in enumerate(groups))
    assert (bound + 2) * (14 + 82) + 1000000 < 1 << 26
    for g, r, ww in wide_batch:
        assert ww[0]["nrows"] == 5 and ww[1]["nrows"] == 4 and ww[2]["nrows"] == 3


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("option", [None, "no_fused_walk", "no_screen"])
def test_long_groups_match_oracle(ctx, long_batch, option, device):
    groups, refs, want = long_batch
    if option:
        ctx.set_option(option, 1)
    try:
        got = ctx.assemble_traces(groups, refs, SCORE, FRACMATCH, CALLED, False, device=device)
    finally:
        if option:
            ctx.set_option(option, 0)
    check(got, want, groups)
    stats = ctx.last_call_stats()
    assert stats["asm_chunks"] == 1 and stats["asm_steps"] == 4
    assert stats["host_syncs"] == 2 + stats["asm_steps"] + 1  # classes, scores, one per chain step, the end


@pytest.mark.parametrize("refs_too", [False, True])
def test_long_groups_repeat_on_int32(ctx, wide_batch, refs_too):
    """un-normalised profiles.  Both sides x 4.0: the 16-bit score launches are refused at the score synchronisation (kWiden) and the call
    runs again on int32 -- the first run adds its two synchronisations.  Traces alone x 4.0: the 16-bit range still holds (Q = 22)."""
    groups, refs, want = wide_batch[int(refs_too)]
    got = ctx.assemble_traces(groups, refs, SCORE, FRACMATCH, CALLED, False)
    check(got, want, groups)
    stats = ctx.last_call_stats()
    assert stats["asm_steps"] == 4
    assert stats["host_syncs"] == (2 if refs_too else 0) + (2 + stats["asm_steps"] + 1)


# ---- the command line -------------------------------------------------------------------------------------------------


def tiled_traces(rng, tmp, n, region_len=1500, tlen=420, some_reverse=True, noisy_ends=True):
    """ABIF files of n reads tiled over a random region (tests/test_gpu_cli.py::tiled_traces): every third one from the other strand"""
    import sage_oracle as so
    from tracy_amd import hostlib
    region = bytes(rng.choice(list(b"ACGT"), size=region_len).tolist())
    paths = []
    for i in range(n):
        start = int(i * (region_len - tlen) / max(n - 1, 1))
        seq = bytearray(region[start:start + tlen])
        for k in range(len(seq)):
            if rng.random() < 0.01:
                seq[k] = int(rng.choice(list(b"ACGT")))
        seq = bytes(seq)
        if some_reverse and i % 3 == 1:
            seq = so.revcomp(seq)
        nb = len(seq)
        tr = np.zeros((4, 12 * nb + 12), np.int32)
        pos = 6 + 12 * np.arange(nb, dtype=np.int32)
        tri = 1.0 - np.abs(np.arange(-5, 6)) / 6.0
        for j, ch in enumerate(seq):
            amp = rng.uniform(500, 1100)
            tr[b"ACGT".index(ch), pos[j] - 5:pos[j] + 6] += (amp * tri).astype(np.int32)
            noisy = noisy_ends and (j < 25 or j > nb - 30)
            tr[int(rng.integers(0, 4)), pos[j] - 5:pos[j] + 6] += (amp * (0.6 if noisy else 0.06) * tri).astype(np.int32)
        p = os.path.join(tmp, "tile%02d.ab1" % i)
        hostlib.write_abif(p, tr, pos, seq, np.full(nb, 40, np.uint8))
        paths.append(p)
    return region, paths


def run_cli(args, cwd, timeout=600):
    return subprocess.run([CLI, "assemble"] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_cli_batch_matches_one_group_command(tmp_path):
    sizes = (2, 5, 3)
    groups = []
    for k, n in enumerate(sizes):
        d = tmp_path / ("g%d" % k)
        d.mkdir()
        region, paths = tiled_traces(np.random.default_rng(100 + k), str(d), n, region_len=700, tlen=260)
        ref = str(d / "region.fa")
        open(ref, "w").write(">region%d\n%s\n" % (k, region.decode()))
        groups.append([ref, paths])
    (tmp_path / "junk").mkdir()
    _, junk = tiled_traces(np.random.default_rng(9), str(tmp_path / "junk"), 1, region_len=400, tlen=260)
    groups[1][1].insert(2, junk[0])  # a trace that matches nothing: the warning path
    single, batch = tmp_path / "single", tmp_path / "batch"
    single.mkdir()
    batch.mkdir()
    opts = ["-i", "-a", "fastq", "-g", "-9", "-e", "-3"]
    for k, (ref, paths) in enumerate(groups):
        r = run_cli(opts + ["-r", ref, "-o", str(single / ("a%d" % k))] + paths, str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("is not matching to the reference" in r.stderr) == (k == 1)
    man = tmp_path / "manifest.tsv"
    lines = [(p, ref, str(batch / ("a%d" % k))) for k, (ref, paths) in enumerate(groups) for p in paths]
    lines = lines[0::2] + lines[1::2]  # the lines of the groups interleaved: a group is the lines of one outprefix, in manifest order
    order = {k: [p for p, _, pre in lines if pre.endswith("a%d" % k)] for k in range(3)}
    with open(man, "w") as f:
        f.write("# trace\treference\toutprefix\n")
        for p, ref, pre in lines:
            f.write("%s\t%s\t%s\n" % (p, "-" if ref == groups[0][0] else ref, pre))
    # (the one-group runs above took the traces in their own order; run them again in the manifest's where that differs)
    for k, (ref, paths) in enumerate(groups):
        if order[k] != paths:
            r = run_cli(opts + ["-r", ref, "-o", str(single / ("a%d" % k))] + order[k], str(tmp_path))
            assert r.returncode == 0, r.stderr[-2000:]
    r = run_cli(opts + ["-r", groups[0][0], "--batch", str(man)], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.count("is not matching to the reference! Trace file will be excluded!") == 1 and "Warning: tile00 " in r.stderr
    for k in range(3):
        for ext in (".align.fa", ".json", ".vertical", ".cons.fq", ".cons.fa"):
            s, b = single / ("a%d%s" % (k, ext)), batch / ("a%d%s" % (k, ext))
            assert s.exists() == b.exists(), (k, ext)
            if s.exists():
                assert s.read_bytes() == b.read_bytes(), (k, ext)
        assert (batch / ("a%d.json" % k)).stat().st_size > 1000
    # two references under one outprefix: refused, the message names the line
    with open(man, "a") as f:
        f.write("%s\t%s\t%s\n" % (groups[0][1][0], groups[1][0], batch / "a0"))
    r = run_cli(opts + ["-r", groups[0][0], "--batch", str(man)], str(tmp_path))
    assert r.returncode == 1 and "line %d" % (len(lines) + 2) in r.stderr, r.stderr[-2000:]
    # no reference: refused (de novo assembly has no batch mode)
    r = run_cli(opts + ["--batch", str(man)], str(tmp_path))
    assert r.returncode == 1 and "-r" in r.stderr
