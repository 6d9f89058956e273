"""What the kernel timers are credited (launches, cells, bytes: integers that depend on the inputs alone) on both paths of
`tracy align` and `tracy decompose`: the stream-ordered pass (tracy_amd/csrc/stream.hip, credits summed on the device) and the
host-planned pipeline (pipeline.hip, option no_stream).  Every rule behind them is stated once in tracy_amd/csrc/launch_rules.h;
the figures in tests/golden/launch_credit.json were recorded before the rules moved there (tests/golden/make_launch_credit_golden.py)
and are compared with margin zero.  The results of both paths are compared too, so that a wrong order or fit cannot hide behind
equal credit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SC = (3, -5, -10, -4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_credit.json")
TIMERS = ("SCORE", "TRACE", "WALK", "BAND", "PREFIX", "ORIGIN", "DECOMP", "AFRAC", "MISC", "FRONT")  # TRACYHIP_TIMER_*
MUST_RUN = ("SCORE", "FRONT", "TRACE", "ORIGIN")
CALLS = (("align_stream", "align", 0), ("align_host", "align", 1), ("decompose_stream", "decompose", 0), ("decompose_host", "decompose", 1))


def align_batch():
    """the first 24 of test_gpu_front's cases (both tiers of the pruned sweep, strip heights 8 to 16, certificates that fail) and
    16 traces too short for a pruned sweep (class 1: both strands in full)"""
    from test_gpu_early_tail import short_traces
    from test_gpu_front import cases
    cs = cases(np.random.default_rng(77))[:24]
    sh = short_traces(np.random.default_rng(78), 16)
    return [c[0] for c in cs] + [s[0] for s in sh], [c[1] for c in cs] + [s[1] for s in sh]


def decompose_batch():
    from tracy_amd import hostlib
    nd = 8
    d = hostlib.synth_decompose_batch(4711, nd, 3000, 1000, 0, mix=1)
    return d, [d["refs"][i].tobytes() for i in range(nd)], nd


def all_timers(ctx):
    from tracy_amd import capi
    out = {}
    for which, name in enumerate(TIMERS):
        kt = capi.KernelTiming()
        capi._check(capi.lib().tracyhip_timing_get(ctx._h, which, C.byref(kt)))
        out[name] = {"launches": int(kt.launches), "cells": int(kt.cells), "bytes": int(kt.bytes)}
    return out


def timed(ctx, fn, no_stream):
    """fn() on one path with the timers on: (result, what the call says of itself, every timer)"""
    from tracy_amd import capi
    ctx.set_option("no_stream", no_stream)
    capi._check(capi.lib().tracyhip_timing_enable(ctx._h, 1))
    capi._check(capi.lib().tracyhip_timing_reset(ctx._h))
    try:
        res = fn()
        return res, ctx.last_call_stats(), all_timers(ctx)
    finally:
        capi.lib().tracyhip_timing_enable(ctx._h, 0)
        ctx.set_option("no_stream", 0)


def measure(ctx):
    """the four calls: {name: (result, stats, timers)}"""
    from tracy_amd import capi
    profs, wins = align_batch()
    d, refs, nd = decompose_batch()

    def align():
        return ctx.align_traces(profs, wins, SC, 50, 50)

    def decompose():
        hbc = capi.HostBaseCalls([d["signal"][i] for i in range(nd)], [d["bcpos"][i] for i in range(nd)],
                                 [d["primary"][i].tobytes() for i in range(nd)], [d["secondary"][i].tobytes() for i in range(nd)])
        return ctx.decompose_traces([d["profiles"][i] for i in range(nd)], hbc, refs, SC)

    return {name: timed(ctx, {"align": align, "decompose": decompose}[what], no_stream) for name, what, no_stream in CALLS}


@pytest.fixture(scope="module")
def measured():
    import tracy_amd
    c = tracy_amd.Context(0)
    try:
        yield measure(c)
    finally:
        c.close()


@pytest.mark.parametrize("name,what,no_stream", CALLS)
def test_timer_credit_is_what_it_was_before_the_rules_had_one_copy(measured, name, what, no_stream):
    golden = json.load(open(GOLDEN))
    res, stats, timers = measured[name]
    assert stats["stream_ordered"] == 1 - no_stream, stats
    for t in MUST_RUN:
        assert timers[t]["cells"] > 0, (name, t, timers)
    fields = ("launches", "cells", "bytes") if golden["compare_launches"] else ("cells", "bytes")
    for t in TIMERS:
        for f in fields:
            assert timers[t][f] == golden["calls"][name][t][f], (name, t, f, timers[t], golden["calls"][name][t])


def test_both_paths_give_the_same_results(measured):
    from test_gpu_stream import same_align, same_decompose
    same_align(measured["align_stream"][0], measured["align_host"][0], True, "stream vs host-planned")
    same_decompose(measured["decompose_stream"][0], measured["decompose_host"][0], "stream vs host-planned")
    st = measured["align_stream"][1]
    assert st["pruned"] >= 16 and st["pruned_uncertified"] >= 1 and st["fallback_traces"] >= 1, st  # tiers run, and some fail
