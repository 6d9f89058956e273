"""The device loops that only large batches reach, at the smallest batch that crosses each boundary, exactly against the oracles:

  variants_kernel          (variants.hip)           grid = min(n, kVarWaves = 2048): a workgroup takes traces blockIdx.x, + gridDim.x, ...
                                                    and reuses its two event lists for each of them
  var_pack_scan_kernel     (variants.hip)           one workgroup of 1024 threads: above 1024 traces a thread sums a stretch of
                                                    per = ceil(nt / 1024) traces, the last threads a short one or none
  decompose_kernel_global  (decompose_kernels.hip)  maxindel > 4096: min(ntraces, 512) workgroups, each with one slot of scan state in
                                                    global memory (DecompSharedT<65536>, 1 296 160 bytes: 0.66 GB at 512 slots) for
                                                    traces blockIdx.x, + gridDim.x, ...

In each, the second and later rounds run on what another trace left behind.  The batches are laid out so that the traces that share
a workgroup / a slot differ in what they leave (many events before none, allele 1 longer before allele 2 longer, a truncated trace
before one that fits; long traces with wide scans before short ones, a breakpoint behind the trace before an ordinary one), and the
layouts are asserted on the CPU -- the tests without the gpu mark need no device.  Traces are the smallest the code accepts: the
counts are the point."""
import functools
import os
import re

import numpy as np
import pytest

import indigo_oracle as io
import pyoracle as orc
import variants_cases as vc
from decomp_cases import SC
from test_gpu_decompose import _random_decomp_cases
from test_gpu_variants import GUARD, TRIMS, batch, check_lists, decompose, usable_reverse  # noqa: F401  (batch: the 24-trace fixture)

gpu = pytest.mark.gpu
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tracy_amd", "csrc")

# ---- 0. the sizes, pinned to the source ----------------------------------------------------------------------------------------------
VAR_GRID = 2048      # kVarWaves
SCAN_THREADS = 1024  # block size of var_pack_scan_kernel
DECOMP_SLOTS = 512   # slots of decompose_kernel_global
MAXINDEL_GLOBAL = 5000  # > kMaxIndelLarge: the scan state lives in global memory
VAR_SIZES = (VAR_GRID, VAR_GRID + 1, 2 * VAR_GRID + 37)         # one round; workgroup 0 alone has a second; three rounds for 37
SCAN_SIZES = (SCAN_THREADS, SCAN_THREADS + 1)                   # per = 1; per = 2 (threads 0..511 two traces, thread 512 one)
DECOMP_SIZES = (DECOMP_SLOTS, DECOMP_SLOTS + 1, 2 * DECOMP_SLOTS + 19)


def source_sizes():
    """what the batch sizes of this module are built on, read from the source text (the constants are not visible through the C ABI)"""
    var = open(os.path.join(CSRC, "variants.hip")).read()
    dec = open(os.path.join(CSRC, "decompose_kernels.hip")).read()
    hdr = open(os.path.join(CSRC, "decompose_kernels.h")).read()

    def one(pattern, text, what):
        m = re.findall(pattern, text)
        assert len(m) == 1, "%s: expected one match of %r in the source, found %d -- update source_sizes() of tests/test_gpu_batch_rounds.py" % (what, pattern, len(m))
        return m[0]
    one(r"grid\s*=\s*std::min\(n,\s*kVarWaves\)", var, "grid of variants_kernel")
    one(r"global\s*=\s*a\.prm\.maxindel\s*>\s*kMaxIndelLarge\b", dec, "use of decompose_kernel_global")
    per = one(r"per\s*=\s*\(nt\s*\+\s*(\d+)u\)\s*/\s*(\d+)u", var, "stretch of var_pack_scan_kernel")
    return dict(var_grid=int(one(r"constexpr\s+uint32_t\s+kVarWaves\s*=\s*(\d+)\s*;", var, "kVarWaves")),
                scan_bounds=int(one(r"__launch_bounds__\((\d+)\)\s*void\s+var_pack_scan_kernel\b", var, "launch bounds of var_pack_scan_kernel")),
                scan_block=int(one(r"hipLaunchKernelGGL\(var_pack_scan_kernel,\s*dim3\(1\),\s*dim3\((\d+)\)", var, "block of var_pack_scan_kernel")),
                scan_per=(int(per[0]) + 1, int(per[1])),
                decomp_slots=int(one(r"slots\s*=\s*std::min<uint32_t>\(a\.ntraces,\s*(\d+)u\)", dec, "slots of decompose_kernel_global")),
                maxindel_large=int(one(r"constexpr\s+int\s+kMaxIndelLarge\s*=\s*(\d+)\s*;", hdr, "kMaxIndelLarge")))


def test_sizes_are_pinned_to_the_source():
    s = source_sizes()
    assert s["var_grid"] == VAR_GRID, \
        "kVarWaves is %d: move VAR_GRID and with it the batches of %s traces (one round, one workgroup with a second, three rounds)" % (s["var_grid"], VAR_SIZES)
    assert s["scan_bounds"] == s["scan_block"] == SCAN_THREADS and s["scan_per"] == (SCAN_THREADS, SCAN_THREADS), \
        "var_pack_scan_kernel runs %s threads: move SCAN_THREADS and with it the batches of %s traces (per = 1, per = 2) and the per = 3 of %d" % (
            (s["scan_bounds"], s["scan_block"], s["scan_per"]), SCAN_SIZES, VAR_GRID + 1)
    assert s["decomp_slots"] == DECOMP_SLOTS, \
        "decompose_kernel_global has %d slots: move DECOMP_SLOTS and with it the batches of %s traces" % (s["decomp_slots"], DECOMP_SIZES)
    assert s["maxindel_large"] < MAXINDEL_GLOBAL, \
        "kMaxIndelLarge is %d: maxindel = %d no longer reaches decompose_kernel_global, raise MAXINDEL_GLOBAL" % (s["maxindel_large"], MAXINDEL_GLOBAL)
    assert (SCAN_THREADS + 1 + SCAN_THREADS - 1) // SCAN_THREADS == 2 and (VAR_GRID + 1 + SCAN_THREADS - 1) // SCAN_THREADS == 3


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


# ---- 1. + 2. variants_kernel, var_pack_scan_kernel / var_pack_copy_kernel ---------------------------------------------------------------
MAX_VARIANTS, MAX_TEXT = 24, 192  # a few of the random cases exceed either (vc.fits says which)
EMPTY_NAMES = ("zero_length", "no_base_in_row0")
# what the three traces of a workgroup are, by workgroup & 7 (ANY: the whole pool)
VAR_PATTERNS = (("BIG", "EMPTY", "BIG"), ("EMPTY", "BIG", "EMPTY"), ("A1", "A2", "A1"), ("A2", "A1", "A2"), ("TRUNC", "BIG", "TRUNC"),
                ("EMPTY", "TRUNC", "BIG"), ("ANY", "ANY", "ANY"), ("ANY", "ANY", "ANY"))
VAR_ORDERINGS = ("many_then_empty", "empty_then_many", "allele1_longer_then_allele2_longer", "allele2_longer_then_allele1_longer",
                 "truncated_then_fits")
# (nt, rot): rot shifts the patterns by one workgroup -- trace 0 has many events and the last trace none (0), or the reverse (1)
VAR_RUNS_HOST = [(SCAN_SIZES[0], 0), (SCAN_SIZES[1], 0), (SCAN_SIZES[1], 1), (VAR_SIZES[0], 0), (VAR_SIZES[1], 0), (VAR_SIZES[1], 1),
                 (VAR_SIZES[2], 0)]
VAR_RUNS_DEVICE = [(VAR_SIZES[0], 1), (VAR_SIZES[1], 0), (VAR_SIZES[1], 1), (VAR_SIZES[2], 1)]


@functools.lru_cache(maxsize=None)
def variant_pool():
    """the distinct cases (named + random) with the oracle's list, computed once, and what the result arrays of one trace must hold:
    records and text packed in record order, ref first, behind them the caller's bytes; a trace that does not fit: nothing at all"""
    from tracy_amd import capi
    named = vc.named_cases()
    cases = [(k, named[k]) for k in sorted(named)] + [("random_%d" % i, c) for i, c in enumerate(vc.random_cases(192, seed=20251021))]
    pool = []
    for name, c in cases:
        want, n1, n2, text = vc.expected(c)
        fits = vc.fits(c, MAX_VARIANTS, MAX_TEXT)
        rec = np.full(MAX_VARIANTS * capi.VARIANT_DTYPE.itemsize, GUARD, np.uint8).view(capi.VARIANT_DTYPE)
        txt = np.full(MAX_TEXT, GUARD, np.uint8)
        if fits:
            at = 0
            for r, v in enumerate(want):
                rec[r] = (v["pos"], v["basenum"], v["gt"], v["call_index"], at, len(v["ref"]), at + len(v["ref"]), len(v["alt"]))
                both = v["ref"] + v["alt"]
                txt[at:at + len(both)] = np.frombuffer(both, np.uint8)
                at += len(both)
            assert at == text
        kinds = {"ANY"}
        if name in EMPTY_NAMES:
            kinds.add("EMPTY")
        if not want:
            kinds.add("NOVAR")
        if not fits:
            kinds.add("TRUNC")
        elif n1 >= 8 and n2 >= 8:
            kinds.add("BIG")
        if fits and n1 > n2 >= 1:
            kinds.add("A1")
        if fits and n2 > n1 >= 1:
            kinds.add("A2")
        pool.append(dict(name=name, case=c, want=want if fits else [], n1=n1, n2=n2, text=text if fits else 0, fits=fits, kinds=kinds, rec=rec, txt=txt))
    by_kind = {k: [i for i, p in enumerate(pool) if k in p["kinds"]] for k in ("ANY", "EMPTY", "NOVAR", "TRUNC", "BIG", "A1", "A2")}
    assert len(by_kind["EMPTY"]) == 2 and len(by_kind["NOVAR"]) >= 4 and 3 <= len(by_kind["TRUNC"]) <= len(pool) // 8, {k: len(v) for k, v in by_kind.items()}
    assert min(len(by_kind[k]) for k in ("BIG", "A1", "A2")) >= 8
    assert any(pool[i]["name"].startswith("random") for i in by_kind["TRUNC"])
    return pool, by_kind


def variant_layout(nt, rot):
    """pool index of every trace: workgroup g = t % VAR_GRID follows VAR_PATTERNS[(g + rot) & 7] over its rounds; runs of traces without
    a variant over whole stretches of the pack scan; first / last trace as `rot` says"""
    pool, by_kind = variant_pool()
    rng = np.random.default_rng(1000 * nt + rot)
    idx = np.zeros(nt, np.int64)
    for t in range(nt):
        g, r = t % VAR_GRID, t // VAR_GRID
        idx[t] = rng.choice(by_kind[VAR_PATTERNS[(g + rot) % 8][r]])
    per = (nt + SCAN_THREADS - 1) // SCAN_THREADS
    # two whole stretches of a thread, and a run of the same length that starts inside one
    for start in (5 * per, 40 * per + 1):
        idx[start:start + 2 * per] = rng.choice(by_kind["NOVAR"], size=2 * per)
    many, none = rng.choice(by_kind["BIG"]), by_kind["EMPTY"][nt % 2]
    idx[0], idx[nt - 1] = (many, none) if rot == 0 else (none, many)
    if rot == 0:  # the last thread with a stretch adds nothing at all
        idx[((nt - 1) // per) * per:nt - 1] = rng.choice(by_kind["NOVAR"], size=(nt - 1) % per)
    return idx


def variant_orderings(idx, first, grid=VAR_GRID):
    """which of VAR_ORDERINGS occur between a trace of [first, first + grid) and the next one of its workgroup"""
    pool, _ = variant_pool()
    seen = set()
    for t in range(first, min(first + grid, len(idx) - grid)):
        a, b = pool[idx[t]], pool[idx[t + grid]]
        if "BIG" in a["kinds"] and "EMPTY" in b["kinds"]:
            seen.add("many_then_empty")
        if "EMPTY" in a["kinds"] and "BIG" in b["kinds"]:
            seen.add("empty_then_many")
        if "A1" in a["kinds"] and "A2" in b["kinds"]:
            seen.add("allele1_longer_then_allele2_longer")
        if "A2" in a["kinds"] and "A1" in b["kinds"]:
            seen.add("allele2_longer_then_allele1_longer")
        if not a["fits"] and b["fits"] and b["want"]:
            seen.add("truncated_then_fits")
    return seen


def check_variant_layout(nt, rot, idx):
    pool, _ = variant_pool()
    novar = np.array([not p["want"] and p["fits"] for p in pool])[idx]
    per = (nt + SCAN_THREADS - 1) // SCAN_THREADS
    stretches = [novar[k * per:min(nt, (k + 1) * per)] for k in range((nt + per - 1) // per)]
    assert sum(1 for s in stretches if s.all()) >= 2 and len(stretches[-1]) == (nt - 1) % per + 1
    assert stretches[-1].all() == (rot == 0)  # the last thread that has traces: nothing to add / something
    assert bool(novar[0]) == (rot == 1) and bool(novar[nt - 1]) == (rot == 0)
    assert any(not p["fits"] for p in (pool[i] for i in idx)) or nt < VAR_GRID
    rounds = (nt + VAR_GRID - 1) // VAR_GRID
    if nt == VAR_GRID + 1:  # the one workgroup with a second round
        assert variant_orderings(idx, 0) == {"many_then_empty" if rot == 0 else "empty_then_many"}
    elif rounds > 1:  # every ordering into the second round and into the third
        for r in range(rounds - 1):
            assert variant_orderings(idx, r * VAR_GRID) == set(VAR_ORDERINGS), (r, variant_orderings(idx, r * VAR_GRID))
    else:
        assert variant_orderings(idx, 0) == set()


@pytest.mark.parametrize("nt,rot", sorted(set(VAR_RUNS_HOST + VAR_RUNS_DEVICE)))
def test_variant_batches_hold_the_orderings(nt, rot):
    """on the CPU: every batch the device tests send has the orderings between the traces of a workgroup and the empty stretches of the
    pack scan that they are there for"""
    check_variant_layout(nt, rot, variant_layout(nt, rot))
    assert {n for n, r in VAR_RUNS_HOST} == set(VAR_SIZES + SCAN_SIZES) and {n for n, r in VAR_RUNS_DEVICE} == set(VAR_SIZES)
    assert {0, 1} == {r for n, r in VAR_RUNS_HOST if n == VAR_SIZES[1]} == {r for n, r in VAR_RUNS_DEVICE if n == VAR_SIZES[1]}


def run_variant_batch(ctx, nt, rot, device):
    from tracy_amd import capi
    pool, _ = variant_pool()
    idx = variant_layout(nt, rot)
    check_variant_layout(nt, rot, idx)
    cases = [pool[i]["case"] for i in idx]
    rows, pos = [], []
    for c in cases:
        for a in (c["a"], c["b"]):
            rows.append((a[0], a[1])); pos.append(a[2])
    b = capi.VariantBuffers(nt, MAX_VARIANTS, MAX_TEXT, device, fill=GUARD)
    got, flags = ctx.call_variants(rows, pos, [c["forward"] for c in cases], [c["bc_len"] for c in cases], *vc.TRIMS, device=device, buffers=b)
    rec, text, n, fl = b.arrays()
    want_n = np.array([len(p["want"]) for p in pool], np.uint32)[idx]
    want_flags = np.array([0 if p["fits"] else 1 for p in pool], np.uint32)[idx]
    want_rec = np.stack([p["rec"] for p in pool])[idx]
    want_text = np.stack([p["txt"] for p in pool])[idx]
    for t in range(nt):  # the list, the flag, nothing for a flagged trace
        p = pool[idx[t]]
        assert flags[t] == want_flags[t] and got[t] == p["want"], (t, p["name"], int(flags[t]), got[t], p["want"])
    assert np.array_equal(n[:nt], want_n) and np.array_equal(fl[:nt], want_flags) and not n[:nt][want_flags == 1].any()
    # the records and text byte for byte, and behind them the caller's bytes
    bad = np.nonzero((rec.view(np.uint8).reshape(nt, -1) != want_rec.view(np.uint8).reshape(nt, -1)).any(axis=1) | (text != want_text).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], pool[idx[bad[0]]]["name"])
    used = np.arange(MAX_VARIANTS)[None, :] < n[:nt, None]
    assert (rec.view(np.uint8).reshape(nt, MAX_VARIANTS, -1)[~used] == GUARD).all()
    # what came back in all: the oracle's sums (a host caller's pack scan counts exactly these)
    bytes_back = int((rec["ref_len"].astype(np.int64) + rec["alt_len"])[used].sum())
    assert int(n[:nt].sum()) == sum(len(pool[i]["want"]) for i in idx) and bytes_back == sum(pool[i]["text"] for i in idx)
    assert bytes_back > 0


@gpu
@pytest.mark.parametrize("nt,rot", VAR_RUNS_HOST)
def test_variants_rounds_and_pack_stretches_in_host_memory(ctx, nt, rot):
    """results in host memory: variants_kernel in one, two and three rounds, then var_pack_scan_kernel with stretches of one, two and
    three traces (1024: every thread one trace; 1025: threads 0..511 two, thread 512 one, the rest none; 2049: three per thread, the
    last thread's stretch once without a variant) and var_pack_copy_kernel"""
    run_variant_batch(ctx, nt, rot, device=False)


@gpu
@pytest.mark.parametrize("nt,rot", VAR_RUNS_DEVICE)
def test_variants_rounds_in_device_memory(ctx, nt, rot):
    run_variant_batch(ctx, nt, rot, device=True)


# ---- 3. decompose_kernel_global -----------------------------------------------------------------------------------------------------
DECOMP_TRIMS = (50, 50)  # the whole batch has one trim pair: the cases _random_decomp_cases makes with it
# what the three traces of a slot are, by slot % 6
DECOMP_PATTERNS = (("LONG", "SHORT", "LONG"), ("SHORT", "LONG", "SHORT"), ("BEHIND", "ORDINARY", "BEHIND"), ("KIND1", "KIND2", "KIND1"),
                   ("KIND2", "KIND1", "KIND2"), ("ORDINARY", "BEHIND", "ORDINARY"))
DECOMP_ORDERINGS = ("long_then_short", "short_then_long", "behind_then_ordinary")


@functools.lru_cache(maxsize=None)
def decomp_pool():
    """short-window cases of 106..419 basecalls at trims 50 / 50 with the oracle's decomposeAlleles at maxindel 5000, computed once"""
    pool = [c for c in _random_decomp_cases(20251021, 1500) if (c["tl"], c["tr"]) == DECOMP_TRIMS]
    for c in pool:
        c["w"] = orc.decompose_alleles(c["rows"][0], c["rows"][1], c["pri"], c["sec"], c["bp"], c["reflen"], *DECOMP_TRIMS, MAXINDEL_GLOBAL, 5)
        nb, kind, scans = len(c["pri"]), c["w"][3][0], len(c["w"][2])  # (the table has one entry per shift that was scanned)
        behind = c["bp"].breakpoint >= nb - sum(DECOMP_TRIMS)
        c["kinds"] = {"ANY", "KIND%d" % kind}
        if behind:
            c["kinds"].add("BEHIND")
        elif kind == 0:
            c["kinds"].add("ORDINARY")
        if nb >= 280 and scans > 64 and not behind:  # (a sweep of the scans takes 64 shifts)
            c["kinds"].add("LONG")
        if nb < 170 and scans <= 64:
            c["kinds"].add("SHORT")
    by_kind = {k: [i for i, c in enumerate(pool) if k in c["kinds"]] for k in ("ANY", "KIND0", "KIND1", "KIND2", "BEHIND", "ORDINARY", "LONG", "SHORT")}
    assert min(len(v) for v in by_kind.values()) >= 4, {k: len(v) for k, v in by_kind.items()}
    return pool, by_kind


@functools.lru_cache(maxsize=None)
def decomp_layout():
    """pool index of the 2 * 512 + 19 traces; the batches of 512 and 513 are its first traces"""
    pool, by_kind = decomp_pool()
    rng = np.random.default_rng(513)
    nt = DECOMP_SIZES[2]
    return tuple(int(rng.choice(by_kind[DECOMP_PATTERNS[(t % DECOMP_SLOTS) % 6][t // DECOMP_SLOTS]])) for t in range(nt))


def check_decomp_layout(idx):
    """every status kind in every round; the orderings between slot-mates wherever there is a later round"""
    pool, _ = decomp_pool()
    nt = len(idx)
    for first in range(0, nt, DECOMP_SLOTS):
        assert {pool[i]["w"][3][0] for i in idx[first:first + DECOMP_SLOTS]} == {0, 1, 2} or nt - first == 1, first
        seen = set()
        for t in range(first, min(first + DECOMP_SLOTS, nt - DECOMP_SLOTS)):
            a, b = pool[idx[t]]["kinds"], pool[idx[t + DECOMP_SLOTS]]["kinds"]
            seen |= {o for o, (x, y) in zip(DECOMP_ORDERINGS, (("LONG", "SHORT"), ("SHORT", "LONG"), ("BEHIND", "ORDINARY"))) if x in a and y in b}
        later = nt - first - DECOMP_SLOTS
        assert seen == (set(DECOMP_ORDERINGS) if later >= 6 else {"long_then_short"} if later == 1 else set()), (first, seen)


def test_decompose_batches_hold_the_orderings_and_every_status_kind():
    idx = decomp_layout()
    assert len(idx) == DECOMP_SIZES[2]
    for nt in DECOMP_SIZES:
        check_decomp_layout(idx[:nt])
    pool, _ = decomp_pool()
    rev = idx[:DECOMP_SIZES[1]][::-1]  # the 513 reversed: slot 0 takes the short trace first, then the long one
    assert "SHORT" in pool[rev[0]]["kinds"] and "LONG" in pool[rev[DECOMP_SLOTS]]["kinds"]


def run_decomp_batch(ctx, idx):
    from tracy_amd import capi
    pool, _ = decomp_pool()
    cs = [pool[i] for i in idx]
    sig = [np.zeros((4, 8), np.int32) for _ in cs]
    pos = [np.zeros(len(c["pri"]), np.int32) for c in cs]
    hbc = capi.HostBaseCalls(sig, pos, [c["pri"] for c in cs], [c["sec"] for c in cs])
    bps = [capi.Breakpoint(1, 1, c["bp"].breakpoint, 0.5) for c in cs]
    pri, sec, dcp, status = ctx.decompose_alleles(hbc, [c["rows"] for c in cs], bps, [c["reflen"] for c in cs], *DECOMP_TRIMS, MAXINDEL_GLOBAL, 5)
    for i, c in enumerate(cs):
        w = c["w"]
        assert (pri[i], sec[i], dcp[i]) == (w[0], w[1], w[2]) and status[i][0] == w[3][0], (i, i % DECOMP_SLOTS, i // DECOMP_SLOTS, idx[i])
        if w[3][0] == 1:
            assert tuple(status[i][:4]) == tuple(w[3][:4]), i
    return list(zip(pri, sec, dcp, status))


@gpu
@pytest.mark.parametrize("nt", DECOMP_SIZES)
def test_decompose_global_in_later_rounds_of_a_slot(ctx, nt):
    """512: every slot one trace; 513: slot 0 a second; 1043: three rounds for 19 slots, two for the rest"""
    idx = decomp_layout()[:nt]
    check_decomp_layout(idx)
    run_decomp_batch(ctx, idx)


@gpu
def test_decompose_global_in_either_order(ctx):
    """the 513 traces and the same reversed: every slot sees other neighbours, slot 0 its two traces in the other order -- each trace
    gives what it gave before"""
    idx = decomp_layout()[:DECOMP_SIZES[1]]
    there = run_decomp_batch(ctx, idx)
    back = run_decomp_batch(ctx, idx[::-1])
    assert there == back[::-1]


@pytest.fixture(scope="module")
def batch_at_maxindel_5000(batch):
    """the oracle chain of the 24 traces at maxindel 5000, once"""
    return [io.decompose_trace(t["sig"], t["bcpos"], t["pri"], t["sec"], t["ref"], SC, *TRIMS, maxindel=MAXINDEL_GLOBAL) for t in batch]


@gpu
def test_decompose_traces_over_the_slots(ctx, batch, batch_at_maxindel_5000):
    """the pipeline at maxindel 5000 with a bit over 512 traces: the 24 of tests/test_gpu_variants.py, 22 times"""
    from tracy_amd import capi
    tr = batch * 22
    assert DECOMP_SLOTS < len(tr) < DECOMP_SLOTS + 24
    hbc = capi.HostBaseCalls([t["sig"] for t in tr], [t["bcpos"] for t in tr], [t["pri"] for t in tr], [t["sec"] for t in tr])
    got = ctx.decompose_traces([t["prof"] for t in tr], hbc, [t["ref"] for t in tr], SC, *TRIMS, maxindel=MAXINDEL_GLOBAL)
    for i in range(len(tr)):
        w = batch_at_maxindel_5000[i % 24]
        assert int(got["status"][i]) == w["status"], i
        assert got["primary"][i] == w["primary"] and got["secondary"][i] == w["secondary"] and got["dcp"][i] == w["dcp"], i
        assert (float(got["fractions"][2 * i]), float(got["fractions"][2 * i + 1])) == w["af"], i


# ---- 4. the variants pipeline with a chunk above 2048 traces -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pipeline_with_one_chunk_above_the_grid(ctx, batch, device):
    """tracyhip_decompose_variants launches variants_kernel once per chunk: 2160 traces in one chunk, 112 workgroups with a second trace"""
    tr = batch * 90
    assert VAR_GRID < len(tr) < 2 * VAR_GRID and usable_reverse(tr) == 90 * usable_reverse(batch) > 0
    outcome = decompose(ctx, tr, device)
    got, flags = ctx.decompose_variants(outcome, [t["slice_pos"] for t in tr])
    st = ctx.last_call_stats()
    assert st["var_chunks"] == 1 and st["traces"] == len(tr), st["var_chunks"]  # (the default workspace holds them; no test sets a limit that lasts)
    assert st["var_realigned"] == usable_reverse(tr) and st["var_truncated"] == 0
    check_lists(tr, got, flags)
