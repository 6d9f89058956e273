"""The screened consensus columns on the device (consensus.hip): the fix-up list, its atomic counter and slots, the host patch and
cons_patch_kernel, chunks, the overflow relaunch, the repeat on int32, queued calls, and ocml's log10 against the host gtLetter.
Inputs and expectations are tests/consensus_fixup_cases.py (asserted in tests/test_consensus_fixup_cases.py); every call is compared
field by field with the oracle and its cons_fixup_columns with the count the host build of cons_column predicts."""
import numpy as np
import pytest

import consensus_fixup_cases as fc
from test_consensus_host import cc, host_gt  # noqa: F401  (cc: the g++ build of the column body, a fixture)
from test_gpu_consensus_batch import SCORE, check_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def check_all(got, want):
    assert len(got["cons"]) == len(want)
    for i, w in enumerate(want):
        check_pair(got, i, w)
        assert int(got["ops_len"][i]) == len(w["rows"][0]) and int(got["cons_len"][i]) == len(w["cons"]), i


def fixups(ctx):
    return ctx.last_call_stats()["cons_fixup_columns"]


def run_mix(ctx, cc, union=True, iupac=False, device=False, scale=1.0):
    pairs = fc.mix()
    e = fc.expectation(cc, pairs, union, iupac, scale=scale, key="mix")
    first, second = fc.firsts(pairs), fc.seconds(pairs)
    if scale != 1.0:
        first, second = fc.scaled(first), fc.scaled(second)
    got = ctx.consensus_traces(first, second, SCORE, union=union, iupac=iupac, device=device)
    check_all(got, e["want"])
    assert fixups(ctx) == e["count"] > 0
    return e


@pytest.mark.parametrize("iupac", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_host_and_device_buffers(ctx, cc, device, iupac):
    """every family in one batch, both strands, ops_len 63 .. 129 and longer: the host patch and cons_patch_kernel"""
    run_mix(ctx, cc, iupac=iupac, device=device)


def test_iupac_adds_exactly_the_tenth_columns(ctx, cc):
    a, b = run_mix(ctx, cc, iupac=False), run_mix(ctx, cc, iupac=True)
    tenth = sum(f == "tenth" for c in b["cols"] for f in c[2])
    assert b["count"] - a["count"] == tenth > 0


@pytest.mark.parametrize("device", [False, True])
def test_union_against_intersect(ctx, cc, device):
    """flagged columns in the overhangs: the union counts and patches them, the intersection emits none of them"""
    u = run_mix(ctx, cc, union=True, iupac=True, device=device)
    x = run_mix(ctx, cc, union=False, iupac=True, device=device)
    over = sum(f and s != "aligned" for c, fl in zip(u["cols"], u["flags"]) for f, s in zip(fl, c[3]))
    assert u["count"] - x["count"] == over > 0


def test_pairs_that_emit_nothing(ctx, cc):
    """NO_OVERLAP pairs of flagged-family columns (by min_overlap, by the match fraction) between pairs that are fixed up"""
    lo = fc.SHORT_PAIR - 1
    pairs = fc.mix()[lo:]
    e = fc.expectation(cc, fc.mix(), True, True, key="mix")
    got = ctx.consensus_traces(fc.firsts(pairs), fc.seconds(pairs), SCORE, iupac=True)
    check_all(got, e["want"][lo:])
    for i in (fc.SHORT_PAIR, fc.MISMATCH_PAIR):
        assert int(got["status"][i - lo]) == 1 and int(got["cons_len"][i - lo]) == 0 and e["per_pair"][i] == 0
    assert fixups(ctx) == sum(e["per_pair"][lo:]) > 0
    # alone, they reach no fix-up at all
    only = [fc.mix()[i] for i in (fc.SHORT_PAIR, fc.MISMATCH_PAIR)]
    got = ctx.consensus_traces(fc.firsts(only), fc.seconds(only), SCORE, iupac=True, device=True)
    check_all(got, [e["want"][fc.SHORT_PAIR], e["want"][fc.MISMATCH_PAIR]])
    assert fixups(ctx) == 0


@pytest.mark.parametrize("device", [False, True])
def test_chunks(ctx, cc, device):
    """a workspace limit of a few pairs: the list and its slots span the chunks"""
    ctx.set_workspace_limit(fc.MIX_LIMIT)
    try:
        run_mix(ctx, cc, iupac=True, device=device)
        assert ctx.last_call_stats()["cons_chunks"] > 1
    finally:
        ctx.set_workspace_limit(0)
    run_mix(ctx, cc, iupac=True, device=device)
    assert ctx.last_call_stats()["cons_chunks"] == 1


def run_overflow(ctx, cc, device):
    p = fc.overflow_pair()
    e = fc.expectation(cc, [p], True, True, key="overflow")
    got = ctx.consensus_traces([p["first"]] * fc.OVERFLOW_COPIES, [p["second"]] * fc.OVERFLOW_COPIES, SCORE, iupac=True, device=device)
    check_all(got, e["want"] * fc.OVERFLOW_COPIES)
    assert fixups(ctx) == fc.OVERFLOW_COUNT == fc.OVERFLOW_COPIES * e["count"] > fc.FIX_CAP


@pytest.mark.parametrize("device", [False, True])
def test_list_overflow(ctx, cc, device):
    """more flagged columns than the list holds: the consensus stage runs again with a list that does"""
    run_overflow(ctx, cc, device)


def test_no_stale_counter_or_list(ctx, cc):
    """a call without flagged columns directly after the overflow, then the mixed batch again: each call its own count"""
    run_overflow(ctx, cc, False)
    pairs = fc.clean_batch()
    e = fc.expectation(cc, pairs, True, True, key="clean")
    for device in (False, True):
        got = ctx.consensus_traces(fc.firsts(pairs), fc.seconds(pairs), SCORE, iupac=True, device=device)
        check_all(got, e["want"])
        assert e["count"] == 0 and fixups(ctx) == 0
    run_mix(ctx, cc, iupac=True)
    run_mix(ctx, cc, iupac=True, device=True)


def test_repeat_on_int32_counts_once(ctx, cc):
    """every profile x 4.0: the call runs twice (16-bit refused at the end of the first run), the flagged columns are counted once"""
    plain = run_mix(ctx, cc, iupac=True)
    syncs = ctx.last_call_stats()["host_syncs"]
    wide = run_mix(ctx, cc, iupac=True, scale=fc.WIDE)
    syncs_wide = ctx.last_call_stats()["host_syncs"]
    assert wide["count"] == plain["count"]
    assert (syncs, syncs_wide) == (2, 4)
    run_mix(ctx, cc, iupac=True, scale=fc.WIDE, device=True)


def test_queued_calls(ctx, cc):
    """two calls with different fix-up counts queued on one context"""
    from tracy_amd import capi
    pairs = fc.mix()
    a, b = pairs[:6], pairs[6:]
    ea = fc.expectation(cc, pairs, True, False, key="mix")
    eb = fc.expectation(cc, pairs, False, True, key="mix")
    na, nb = sum(ea["per_pair"][:6]), sum(eb["per_pair"][6:])
    assert na > 0 and nb > 0 and na != nb
    p = capi.PreparedConsensus(fc.firsts(a), fc.seconds(a), SCORE)
    q = capi.PreparedConsensus(fc.firsts(b), fc.seconds(b), SCORE, union=False, iupac=True)
    ctx.consensus_traces_async(p.job, p.prm, p.out)
    ctx.consensus_traces_async(q.job, q.prm, q.out)
    ctx.synchronize()
    check_all(p.results(), ea["want"][:6])
    check_all(q.results(), eb["want"][6:])
    assert fixups(ctx) == nb  # (the statistics are the last call's)


@pytest.mark.parametrize("iupac", [False, True])
@pytest.mark.parametrize("device", [False, True])
def test_device_log10_over_many_columns(ctx, cc, device, iupac):
    """32 768 aligned columns, a crafted one at every eighth position: ocml's log10 plus the screen against the host gtLetter of the
    float32 column sums.  A mismatch at an unflagged column would be a finding against the 4 ulp assumed for the device."""
    pairs = fc.log10_batch()
    got = ctx.consensus_traces(fc.firsts(pairs), fc.seconds(pairs), SCORE, iupac=iupac, device=device)
    sample = fc.expectation(cc, [pairs[i] for i in fc.LOG10_SAMPLE], True, iupac, key="log10_sample")
    for i, w in zip(fc.LOG10_SAMPLE, sample["want"]):
        check_pair(got, i, w)
    count = 0
    for i, p in enumerate(pairs):
        # the precondition of the expectation: the diagonal
        assert int(got["status"][i]) == 0 and int(got["forward"][i]) == 1
        assert int(got["ops_len"][i]) == p["first"].shape[1] == p["second"].shape[1] == int(got["cons_len"][i]), i
        assert b"-" not in got["rows"][i][0] + got["rows"][i][1], i
        cl = fc.diagonal_columns(p)
        letter, qual = host_gt(cc, cl, iupac)
        flag = fc.stable_flags(cc, cl, iupac)
        bad = np.flatnonzero((np.frombuffer(got["cons"][i], np.uint8) != letter) | (got["qual"][i].astype(np.uint32) != qual))
        assert bad.size == 0, (i, bad[:8], flag[bad[:8]], cl[bad[:8]])
        count += int(flag.sum())
    assert fixups(ctx) == count > 1000
