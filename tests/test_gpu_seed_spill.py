"""Device k-mer seeding with the option seed_spill (tracyhip_seed_traces, seed_spill_kernel): traces whose vote lists exceed the LDS
capacity seed_vote_cap are answered on the device, their votes counted in hash tables in device memory, with the results of host
seeding (Genome.seed, tracyhost_seed_batch) in every field of every trace and in the window bytes -- on the toy genome of
test_gpu_seed_device.py at small capacities (spills in both passes, ties, palindromes, N runs, clipped windows, unanchorable traces)
and on a genome of repeats at the default capacity: a 30-copy family, a 60 bp unit in 999 and one in 1000 copies, long unique reads,
a chimera that overflows in the first pass and anchors in neither."""
import ctypes as C
import os

import numpy as np
import pytest

import sage_oracle as so
from test_gpu_seed_device import FIELDS, assert_same, rand_dna, toy, toy_reads  # noqa: F401  (toy: the fixture, per module)

pytestmark = pytest.mark.gpu

TRIMS = ((50, 50), (20, 20), (14, 14))


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def spill(ctx, on, cap=2048):
    ctx.set_option("seed_spill", 1 if on else 0)
    ctx.set_option("seed_vote_cap", cap)


def raw_status(ctx, dg, reads, trim_left, trim_right, support, maxindel):
    """tracyhip_seed_traces as it answers, before DeviceGenome merges the host's results in: the status of every trace"""
    from tracy_amd import capi, hostlib
    packed = hostlib.Genome.pack_consensus(reads)
    n = packed["n"]
    cap = int(packed["lens"].max()) + 2 * maxindel + 2
    out = dict(status=np.full(n, -7, np.int32), forward=np.zeros(n, np.uint8), kmersupport=np.zeros(n, np.uint32), pos=np.zeros(n, np.uint32),
               contig=np.zeros(n, np.uint32), slice_len=np.zeros(n, np.uint32), slices=np.zeros((n, cap), np.uint8))
    blob = packed["blob"]
    ss = capi.SeqSet()
    ss.kind, ss.data, ss.count = capi.SEQ_CHAR, C.cast(C.c_char_p(blob), C.c_void_p).value, n
    ss.offset = packed["offs"].ctypes.data_as(C.POINTER(C.c_uint64))
    ss.length = packed["lens"].ctypes.data_as(C.POINTER(C.c_uint32))
    prm = capi.SeedParams(0, 0, dg.kmer, support, maxindel)
    keep = capi.trims_each(prm, trim_left, trim_right, n)
    r = capi.SeedResult()
    for k in FIELDS:
        setattr(r, k, out[k].ctypes.data)
    r.slices, r.slice_cap = out["slices"].ctypes.data, cap
    capi.seed_traces(ctx, dg._h, ss, prm, capi.MEM_HOST, r)
    del keep
    assert set(np.unique(out["status"])) <= {0, 1, 2}  # (the internal spill status never reaches a caller)
    return out["status"]


def deferred(status):
    return set(np.nonzero(status == 2)[0].tolist())


# ---- 1. the toy genome and reads of test_gpu_seed_device.py ----
@pytest.mark.parametrize("trims,support,maxindel", [((50, 50), 3, 1000), ((20, 30), 3, 500), ((14, 14), 2, 300), ((10, 5), 3, 200)])
def test_toy_spill_equals_host(ctx, toy, trims, support, maxindel):
    gs, seqs, rep, dup = toy
    g = gs["fasta"]
    dg = g.to_device(ctx)
    try:
        reads = [r.encode() for r in toy_reads(np.random.default_rng(5), seqs, rep, dup)]
        want = g.seed(reads, trims[0], trims[1], support, maxindel, 4)
        spill(ctx, False)
        base = deferred(raw_status(ctx, dg, reads, trims[0], trims[1], support, maxindel))
        for cap in (8, 64, 2048):
            spill(ctx, True, cap)
            got = dg.seed(reads, trims[0], trims[1], support, maxindel, 4)
            st = ctx.last_call_stats()
            assert_same(got, want, len(reads), (trims, cap))
            assert deferred(raw_status(ctx, dg, reads, trims[0], trims[1], support, maxindel)) == base, (trims, cap)  # none for votes any more
            assert got["n_deferred"] == len(base) and got["n_spilled"] == st["seed_spilled"] and st["seed_spill_deferred"] == 0
            if trims == (10, 5):
                assert len(base) == len(reads) and st["seed_spilled"] == 0  # trims shorter than k - 1: still the host's two scans
            elif cap == 8:
                assert st["seed_spilled"] > 100 and st["seed_spill_launches"] >= 1, st
            elif cap == 2048:
                assert st["seed_spilled"] == 0 and st["seed_spill_launches"] == 0, st
    finally:
        spill(ctx, False)
        dg.close()


# ---- 2. a genome of repeats at the default capacity ----
def repeat_genome(rng):
    """~330 kb: 30 exact copies of a 600 bp unit and two 60 bp units in 999 and 1000 copies, every copy between its own random spacers,
    and 20 kb of unique sequence"""
    fam, u999, u1000, unique = rand_dna(rng, 600), rand_dna(rng, 60), rand_dna(rng, 60), rand_dna(rng, 20000)
    parts = [rand_dna(rng, 700)]
    for _ in range(30):
        parts += [fam, rand_dna(rng, 1400)]
    left_of_last = "".join(parts[:-2])  # (the read across the unit's edge takes the last copy and its spacer)
    parts.append(unique)
    for unit, copies in ((u999, 999), (u1000, 1000)):
        for _ in range(copies):
            parts += [rand_dna(rng, 65), unit]
        parts.append(rand_dna(rng, 65))
    body = "".join(parts)
    edge = len(left_of_last) + 600  # first base behind the last copy of the family
    assert body[edge - 600:edge] == fam and body.count(fam) == 30 and body.count(u999) == 999 and body.count(u1000) == 1000
    return body, fam, u999, u1000, unique, edge


def repeat_reads(rng, body, fam, u999, u1000, unique, edge):
    rc = so._revcomp_str
    reads = [fam[50:550], rc(fam[50:550]),                                          # 0, 1: inside the 30-copy unit
             body[edge - 300:edge + 300],                                           # 2: across its edge into a unique spacer
             rand_dna(rng, 30) + u999 + rand_dna(rng, 30),                          # 3, 4: the 999-copy unit between foreign flanks
             rc(rand_dna(rng, 30) + u999 + rand_dna(rng, 30)),
             rand_dna(rng, 30) + u1000 + rand_dna(rng, 30),                         # 5, 6: the 1000-copy unit: no k-mer below 1000 occurrences
             rc(rand_dna(rng, 30) + u1000 + rand_dna(rng, 30)),
             unique[1000:4000], rc(unique[1000:4000]),                              # 7, 8: 3 kb of unique sequence
             unique[5000:7400] + rc(unique[10000:12400])]                           # 9: chimera, ~2 300 unique votes on each strand
    return [r.encode() for r in reads]


OVER = {0, 1, 3, 4, 7, 8, 9}  # the reads whose lists exceed 2048 votes at every pair of TRIMS (windows x copies, by the window rule)


@pytest.fixture(scope="module")
def rep(tmp_path_factory):
    from tracy_amd import hostlib
    rng = np.random.default_rng(20261020)  # (a seed under which no 17-mer of the family's reads occurs elsewhere by chance)
    built = repeat_genome(rng)
    path = str(tmp_path_factory.mktemp("seed_spill") / "repeats.fa")
    with open(path, "w") as f:
        f.write(">chrR\n")
        for i in range(0, len(built[0]), 60):
            f.write(built[0][i:i + 60] + "\n")
    g = hostlib.Genome(path, 15, 4)
    reads = repeat_reads(rng, *built)
    want = {t: g.seed(reads, t[0], t[1], 3, 1000, 4) for t in TRIMS}  # computed once, shared, left unchanged
    yield g, path, reads, want
    g.close()


@pytest.fixture(scope="module")
def rep_dev(ctx, rep):
    dg = rep[0].to_device(ctx)
    yield dg
    dg.close()


def test_repeat_genome_spills_and_equals_host(ctx, rep, rep_dev):
    g, path, reads, want = rep
    try:
        for t in TRIMS:
            w = want[t]
            assert list(w["status"][[0, 1, 3, 4, 7, 8]]) == [1] * 6 and w["status"][9] == 0, (t, list(w["status"]))
            assert 400 <= w["kmersupport"][0] <= 472 and w["forward"][0] == 1 and w["forward"][1] == 0
            spill(ctx, False)
            off = rep_dev.seed(reads, t[0], t[1], 3, 1000, 4)
            off_set = deferred(raw_status(ctx, rep_dev, reads, t[0], t[1], 3, 1000))
            assert_same(off, w, len(reads), (t, "off"))
            assert off["n_deferred"] == len(off_set) and off["n_spilled"] == 0 and OVER <= off_set, (t, off_set)  # as today: deferred
            spill(ctx, True)
            on = rep_dev.seed(reads, t[0], t[1], 3, 1000, 4)
            st = ctx.last_call_stats()
            on_set = deferred(raw_status(ctx, rep_dev, reads, t[0], t[1], 3, 1000))
            assert_same(on, w, len(reads), (t, "on"))
            assert on["n_deferred"] == 0 and on_set == set(), (t, on_set)
            spilled = off_set - on_set
            assert OVER <= spilled and st["seed_spilled"] == len(spilled) == on["n_spilled"] and st["seed_spill_deferred"] == 0, (t, spilled, st)
            assert st["seed_spill_launches"] == 1, st
    finally:
        spill(ctx, False)


# ---- 3. a genome built on the device without a host table ----
def test_no_host_table(ctx, rep):
    from tracy_amd import hostlib
    g, path, reads, want = rep
    g2, dg = hostlib.Genome.from_fasta_on_device(path, ctx, 15, copy_back=False)
    try:
        assert not g2.has_table()
        spill(ctx, False)
        with pytest.raises(RuntimeError):
            dg.seed(reads[:1], 50, 50, 3, 1000, 4)
        spill(ctx, True)
        got = dg.seed(reads, 50, 50, 3, 1000, 4)
        assert_same(got, want[(50, 50)], len(reads), "device-built, no host table")
        assert got["n_deferred"] == 0 and got["n_spilled"] >= len(OVER)
    finally:
        spill(ctx, False)
        dg.close()
        g2.close()


# ---- 4. the workspace limit ----
def test_workspace_limit_sub_chunks_and_deferral(ctx, rep, rep_dev):
    g, path, reads, want = rep
    w = want[(14, 14)]
    try:
        spill(ctx, True)
        # a read in the 999-copy unit casts 46 x 999 votes on one strand: 131 072 slots of 16 bytes, 2 MiB; no two of them fit 3 MiB
        ctx.set_workspace_limit(3 << 20)
        got = rep_dev.seed(reads, 14, 14, 3, 1000, 4)
        st = ctx.last_call_stats()
        assert_same(got, w, len(reads), "3 MiB")
        assert st["seed_spill_launches"] >= 2 and st["seed_spill_deferred"] == 0 and got["n_deferred"] == 0, st
        assert st["seed_spilled"] == got["n_spilled"] >= len(OVER)
        # ... and neither fits 1 MiB: those two are the host's, the merged result is the same
        ctx.set_workspace_limit(1 << 20)
        got = rep_dev.seed(reads, 14, 14, 3, 1000, 4)
        st = ctx.last_call_stats()
        assert_same(got, w, len(reads), "1 MiB")
        assert st["seed_spill_deferred"] >= 1 and got["n_deferred"] == st["seed_spill_deferred"], (st, got["n_deferred"])
        assert st["seed_spilled"] >= 1 and st["seed_spilled"] + st["seed_spill_deferred"] >= len(OVER), st
    finally:
        ctx.set_workspace_limit(0)
        spill(ctx, False)


# ---- 5. windows left on the device ----
def test_device_memory_windows(ctx, rep, rep_dev):
    import torch
    from tracy_amd import capi, hostlib
    g, path, reads, want = rep
    packed = hostlib.Genome.pack_consensus(reads)
    w = g.seed_packed(packed, 20, 20, 3, 1000, 4)
    try:
        spill(ctx, True)
        got = rep_dev.seed_packed(packed, 20, 20, 3, 1000, 4, mem=capi.MEM_DEVICE)
    finally:
        spill(ctx, False)
    assert isinstance(got["slices_2d"], torch.Tensor) and got["slices_2d"].is_cuda
    assert got["n_deferred"] == 0 and got["n_spilled"] >= len(OVER)
    n = len(reads)
    ok = w["status"][:n] == 1
    assert np.array_equal(got["status"][:n], w["status"][:n]) and np.array_equal(got["slice_len"][:n], w["slice_len"][:n])
    for k in FIELDS:
        assert np.array_equal(got[k][:n][ok], w[k][:n][ok]), k
    dev = got["slices_2d"].cpu().numpy()
    for i in range(n):
        L = int(w["slice_len"][i])
        assert dev[i, :L].tobytes() == w["slices_2d"][i, :L].tobytes(), i


# ---- 6. per-trace trims ----
def test_per_trace_trims(ctx, rep, rep_dev):
    g, path, reads, want = rep
    n = len(reads)
    for shift in range(3):
        pair = [TRIMS[(i + shift) % 3] for i in range(n)]
        tl, tr = np.array([p[0] for p in pair], np.uint32), np.array([p[1] for p in pair], np.uint32)
        try:
            spill(ctx, True)
            got = rep_dev.seed(reads, tl, tr, 3, 1000, 4)
        finally:
            spill(ctx, False)
        assert got["n_deferred"] == 0 and got["n_spilled"] >= len(OVER)
        for i in range(n):
            w = want[pair[i]]
            assert got["status"][i] == w["status"][i] and got["slice_len"][i] == w["slice_len"][i], (shift, i)
            if w["status"][i] == 1:
                for k in FIELDS:
                    assert got[k][i] == w[k][i], (shift, i, k)
            assert got["slices"][i] == w["slices"][i], (shift, i)


# ---- 7. the option ----
def test_option_plumbing(ctx):
    import tracy_amd
    from tracy_amd import capi
    fresh = tracy_amd.Context(0)
    try:
        assert fresh.describe()["seed_spill"] == "0"
        fresh.set_option("seed_spill", 1)
        assert fresh.describe()["seed_spill"] == "1"
        fresh.set_option("seed_spill", "0")
        assert fresh.describe()["seed_spill"] == "0"
        for bad in ("2", "yes", "", "10"):
            with pytest.raises(capi.TracyHipError) as e:
                fresh.set_option("seed_spill", bad)
            assert e.value.code == capi.ERR_ARG and fresh.describe()["seed_spill"] == "0"
    finally:
        fresh.close()
    old = os.environ.get("TRACYHIP_SEED_SPILL")
    os.environ["TRACYHIP_SEED_SPILL"] = "1"
    try:
        under = tracy_amd.Context(0)
    finally:
        if old is None:
            del os.environ["TRACYHIP_SEED_SPILL"]
        else:
            os.environ["TRACYHIP_SEED_SPILL"] = old
    try:
        assert under.describe()["seed_spill"] == "1"
    finally:
        under.close()
    st = ctx.last_call_stats()
    assert {"seed_spilled", "seed_spill_launches", "seed_spill_deferred"} <= set(st)
