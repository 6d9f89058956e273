"""What tracyhip_denovo_traces decides on the host (tracy_amd/csrc/denovo_plan.h: strand assignment from the strand table, the overlap
verdict, the UPGMA tree plan) and the 's' count body of assemble_wave.h on the 64-fiber host wave, against the Python restatements
of tests/msa_oracle.py / tests/denovo_cases.py; the tree composed from the emulated wave bodies against msa_oracle.msa + consensus;
and the argument checks and command-line refusals of the call, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denovo_cases as dc
import msa_oracle as mo
import test_emu_assemble as ea

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_denovo.so")
    srcs = [os.path.join(HERE, "emu", "emu_denovo.cpp"), os.path.join(HERE, "emu", "emu_assemble.cpp"), os.path.join(HERE, "emu", "host_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/denovo_plan.h"), os.path.join(ROOT, "tracy_amd/csrc/assemble_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/dp_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]], stderr=subprocess.DEVNULL)
    return C.CDLL(so)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def run_strands(emu, T):
    K = T.shape[0]
    flat = np.ascontiguousarray(T.reshape(-1), np.int32) if K else np.zeros(1, np.int32)
    rev = np.full(max(K, 1), 7, np.uint8)
    d = np.full(max(K * K, 1), -9, np.int32)
    assert emu.emu_denovo_strands(_p(flat), C.c_uint32(K), _p(rev), _p(d)) == 0
    return rev[:K].tolist(), d[:K * K].reshape(K, K).tolist()


def run_tree(emu, dist):
    num = len(dist)
    dim = 2 * num + 1
    flat = np.ascontiguousarray(np.array(dist, np.int32).reshape(-1))
    p = np.full(3 * dim, -7, np.int32)
    height = np.full(dim, -7, np.int32)
    below = np.full(dim, 7, np.uint8)
    order = np.full(num, 0xdead, np.uint32)
    out = np.zeros(3, np.int32)
    assert emu.emu_denovo_tree(_p(flat), C.c_int32(num), _p(p), _p(height), _p(below), _p(order), _p(out)) == 0
    return dict(p=p.reshape(dim, 3).tolist(), height=height.tolist(), below=below.tolist(), order=order[:out[2]].tolist(), root=int(out[0]),
                maxh=int(out[1]))


def oracle_tree(dist):
    num = len(dist)
    d = [[-1] * (2 * num + 1) for _ in range(2 * num + 1)]
    for a in range(num):
        for b in range(a + 1, num):
            d[a][b] = int(dist[a][b])
    root, p = mo.upgma(d, num)

    def leaves(v):
        return [v] if v < num else leaves(p[v][1]) + leaves(p[v][2])
    return root, p, dc.tree_heights(p, num, root), leaves(root)


def test_strands_from_the_table_are_rev_seq_based_on_dist(emu):
    for name, g, w in zip(dc.KINDS, dc.groups(), dc.oracle(0.5)):
        T = dc.strand_table(g)
        rev, d = run_strands(emu, T)
        assert [1 - r for r in rev] == w["forward"], name              # msa_oracle.rev_seq_based_on_dist on the profiles
        assert (rev, d) == dc.strands_from_table(T), name              # ... and its final matrix, through the table restatement
    rng = np.random.default_rng(515)
    flipped = ties = 0
    for n in range(200):
        K = 2 + n % 8
        T = rng.integers(0, 51, size=(K, K, 2, 2)).astype(np.int32)
        if n % 4 == 0:
            T[:] = T[:, :, :1, :1]  # every strand scores alike: the flip is taken on >=
            ties += 1
        got = run_strands(emu, T)
        assert got == dc.strands_from_table(T), n
        flipped += sum(got[0])
    assert flipped > 100 and ties == 50


def test_overlap_verdict_is_the_restated_threshold(emu):
    f32 = np.float32
    fractions = [0.5, 0.75, 0.1, 0.3, 0.9, 1.0, 0.0, float(f32(1) / f32(3)), 0.7]
    seen = set()
    for fm in fractions:
        for match, mismatch in ((3, -5), (5, -4), (1, -1)):
            for na in (0, 1, 20, 25, 26, 27, 33, 100, 101, 333, 1000):
                thr = dc.overlap_threshold(na, fm, (match, mismatch))
                for gs in sorted({int(np.floor(thr)) - 1, int(np.floor(thr)), int(np.floor(thr)) + 1, int(np.ceil(thr)), -na, 0, 3 * na}):
                    for size in (na, max(1, 10 * na - 1), 10 * na, 10 * na + 1, 260):
                        if size < 1:
                            continue
                        want = dc.overlap_ok(na, gs, size, float(f32(fm)), (match, mismatch))
                        got = emu.emu_denovo_overlap_ok(na, gs, size, C.c_float(fm), match, mismatch)
                        assert bool(got) == want, (fm, match, mismatch, na, gs, size)
                        seen.add((want, na > 25, na / float(size) > 0.1, gs > thr))
    assert {s[0] for s in seen} == {True, False}
    assert (False, True, True, False) in seen and (False, True, False, True) in seen and (False, False, True, True) in seen
    # a float-rounding edge: 0.7f * 3 * 101 rounds away from the double product
    assert dc.overlap_threshold(101, 0.7, (3, -5)) != 101 * 0.7 * 3 + 101 * (1 - 0.7) * -5


def test_tree_plan_is_upgma(emu):
    rng = np.random.default_rng(77)
    tables = [w["tree"]["dist"] for f in dc.FRACTIONS for w in dc.oracle(f) if w["tree"]]
    for n in range(200):
        num = 2 + n % 8
        lo = -20 if n % 5 == 0 else 0  # negative scores: UPGMA stops before everything is joined
        tables.append(rng.integers(lo, 51 if n % 2 else 6, size=(num, num)).tolist())
    early = leafroot = 0
    for dist in tables:
        num = len(dist)
        got = run_tree(emu, dist)
        root, p, height, leaves = oracle_tree(dist)
        assert got["root"] == root and got["p"] == p and got["order"] == leaves
        assert got["height"][:root + 1] == height[:root + 1] and got["maxh"] == height[root]
        assert [v for v in range(2 * num + 1) if got["below"][v]] == sorted(set(leaves) | {v for v in range(num, root + 1) if set(oracle_leaves(p, num, v)) <= set(leaves)})
        early += len(leaves) < num
        leafroot += root < num
    assert early > 5 and leafroot > 0


def oracle_leaves(p, num, v):
    return [v] if v < num else oracle_leaves(p, num, p[v][1]) + oracle_leaves(p, num, p[v][2])


@pytest.mark.parametrize("L", [1, 63, 64, 65, 300])
def test_count_body_is_str_count(emu, L):
    rng = np.random.default_rng(L)
    for pattern in ("s" * L, "h" * L, "".join(rng.choice(list("sshv"), size=L).tolist()), "".join(rng.choice(list("shvS"), size=L).tolist())):
        ops = np.frombuffer(pattern.encode() + b"s" * 70, np.uint8).copy()  # ('s' bytes behind the string: they must not count)
        lanes = np.full(64, 0xdead, np.uint32)
        assert emu.emu_count_aligned(_p(ops), C.c_uint32(L), _p(lanes)) == 0
        assert lanes.tolist() == [pattern.count("s")] * 64, pattern


@pytest.mark.parametrize("fracmatch", dc.FRACTIONS)
def test_tree_of_wave_bodies_is_the_oracle_msa(emu, fracmatch):
    """the tree as denovo.hip composes it -- the plan of denovo_tree, per node the dynamic program (the oracle's here), msa_merge with
    the left rows first (several rows on both sides; a leaf as its profile), msa_profile of every node below the root, and the
    consensus -- against msa_oracle.palign + consensus, for every group of the cases"""
    import pyoracle as orc
    done = wide_sides = 0
    for name, w in zip(dc.KINDS, dc.oracle(fracmatch)):
        t = w["tree"]
        if not t:
            assert w["nrows"] == 0
            continue
        plan = run_tree(emu, t["dist"])
        num, sps = t["num"], t["sps"]
        rows, prof = {}, {v: sps[v] for v in range(num)}
        for h in range(1, plan["maxh"] + 1):
            for v in range(num, plan["root"] + 1):
                if plan["height"][v] != h or not plan["below"][v]:
                    continue
                l, r = plan["p"][v][1], plan["p"][v][2]
                _, btr = orc.gotoh_prof(np.ascontiguousarray(prof[l]), np.ascontiguousarray(prof[r]), 1, 1, dc.SCORE)
                rows[v], _ = ea.run_merge(emu, btr[::-1].decode(), rows.get(l, prof[l]), rows.get(r, prof[r]))
                wide_sides += l in rows and r in rows
                if v != plan["root"]:
                    prof[v] = np.ascontiguousarray(ea.run_profile(emu, rows[v]))
        assert rows[plan["root"]] == w["rows"], name
        assert plan["order"] == t["sidx"], name
        assert ea.run_consensus(emu, rows[plan["root"]], dc.CALLED, 0) == (w["gapped"], w["cons"], w["qual"]), name
        done += 1
    assert done == (11 if fracmatch == 0.5 else 7) and (wide_sides >= 3 or fracmatch != 0.5)


# ---- the argument checks of tracyhip_denovo_traces --------------------------------------------------------------------------------


def _job(lens=((5, 7), (4,))):
    from tracy_amd import capi
    return capi.PreparedDenovo([[np.full((6, n), 0.1, np.float32) for n in g] for g in lens], (3, -5, -10, -4))


def test_argument_validation_needs_no_device():
    """tracyhip_denovo_validate: what tracyhip_denovo_traces checks before it touches a device"""
    from tracy_amd import capi
    lib = capi.lib()
    ERR_ARG = -1

    def check(p, mem=0):
        return lib.tracyhip_denovo_validate(C.byref(p.job), C.byref(p.prm), mem, C.byref(p.out))
    p = _job()
    assert check(p) == 0 and check(p, 1) == 0
    assert check(p, 2) == ERR_ARG and "mem" in lib.tracyhip_last_error().decode()
    assert lib.tracyhip_denovo_validate(None, C.byref(p.prm), 0, C.byref(p.out)) == ERR_ARG
    assert lib.tracyhip_denovo_validate(C.byref(p.job), None, 0, C.byref(p.out)) == ERR_ARG
    assert lib.tracyhip_denovo_validate(C.byref(p.job), C.byref(p.prm), 0, None) == ERR_ARG
    for field, bad in (("group_first", None), ("match_fraction", float("nan")), ("fraction_called", float("nan"))):
        p = _job()
        setattr(p.job, field, bad)
        assert check(p) == ERR_ARG, field
        assert field.split("_")[0] in lib.tracyhip_last_error().decode()
    for field in ("data", "offset", "length"):
        p = _job()
        setattr(p.job.traces, field, None)
        assert check(p) == ERR_ARG, field
    p = _job()
    p.job.traces.kind = capi.SEQ_CHAR
    assert check(p) == ERR_ARG
    for field, _ in capi.DenovoResult._fields_:
        p = _job()
        setattr(p.out, field, None)
        assert check(p) == ERR_ARG, field
    p = _job()  # group_first decreases
    p.first[1] = 3
    p.first[2] = 2
    assert check(p) == ERR_ARG and "decreases" in lib.tracyhip_last_error().decode()
    p = _job()  # ... runs past the set
    p.first[2] = 4
    assert check(p) == ERR_ARG and "the set holds 3" in lib.tracyhip_last_error().decode()
    p = _job()  # a trace without columns
    p.keep[0].length[1] = 0
    assert check(p) == ERR_ARG and "no columns" in lib.tracyhip_last_error().decode()
    for lens in ((), ((), (3,)), ((4,), (5, 6))):  # an empty batch, a group without traces, a group of one trace
        assert check(_job(lens)) == 0, lens
    p = _job()
    p.job.ngroups = 0
    assert check(p) == 0
    # the call itself answers the same before it looks for a device
    p = _job()
    p.job.match_fraction = float("nan")
    assert lib.tracyhip_denovo_traces(None, C.byref(p.job), C.byref(p.prm), 0, C.byref(p.out)) == ERR_ARG
    assert "match_fraction" in lib.tracyhip_last_error().decode()
    # the three counters close tracyhip_call_stats, mirrored here
    assert [n for n, _ in capi.CallStats._fields_][-3:] == ["denovo_chunks", "denovo_rounds", "denovo_steps"]


# ---- what `assemble --denovo` refuses before it opens a device ---------------------------------------------------------------------


def test_cli_denovo_refusals_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "tracy_amd", "bin", "tracy_amd_cli")
    assert os.path.exists(cli), "tracy_amd_cli is not built: run __graft_entry__.build()"
    for name in ("t1.ab1", "t2.ab1"):
        (tmp_path / name).write_bytes(b"x")
    (tmp_path / "r1.fa").write_text(">r\nACGT\n")
    man = tmp_path / "m.tsv"
    man.write_text("# trace\treference\toutprefix\nt1.ab1\t-\tout/a\nt2.ab1\tr1.fa\tout/a\n")
    run = lambda args: subprocess.run([cli, "assemble"] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    r = run(["--denovo", "t1.ab1", "t2.ab1"])
    assert r.returncode == 1 and "--denovo needs --batch" in r.stderr
    r = run(["--denovo", "-r", "r1.fa", "--batch", "m.tsv"])
    assert r.returncode == 1 and "--denovo" in r.stderr and "-r" in r.stderr
    r = run(["--denovo", "--batch", "m.tsv"])  # a manifest line naming a reference: the message carries the line number
    assert r.returncode == 1 and "line 3" in r.stderr and "r1.fa" in r.stderr
    man.write_text("t1.ab1\t-\n")
    r = run(["--denovo", "--batch", "m.tsv"])
    assert r.returncode == 1 and "Malformed manifest line 1" in r.stderr
    man.write_text("missing.ab1\t-\tout/a\n")
    r = run(["--denovo", "--batch", "m.tsv"])
    assert r.returncode == 1 and "Trace file is missing: missing.ab1" in r.stderr
    r = run(["--batch", "m.tsv"])  # without --denovo and -r: today's refusal, unchanged
    assert r.returncode == 1 and "--batch needs a reference (-r)" in r.stderr
    assert "--denovo" in run(["--help"]).stdout
