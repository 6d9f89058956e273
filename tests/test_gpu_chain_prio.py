"""Wave priority for the voted strand's chain beside the other strand's full sweeps (tracy_amd/csrc/stream.hip queue_orientation,
queued_prio; option chain_prio = 0 / 1 / 2; band16_launch.h wave_prio).

The option changes nothing a kernel computes: priority decides which wave of a SIMD issues next.  Every case therefore runs with
chain_prio 0, 1 and 2 and once on the host-planned pipeline (no_stream); every ALIGN_KEYS array and every `btr` must be the same in all
four, and the stage counters of the call the same under the three priority settings."""
import os

import numpy as np
import pytest

from test_gpu_early_tail import SC, against_oracle, mixed_batch, same_align  # (same_align compares every ALIGN_KEYS array and btr)

COMP = bytes.maketrans(b"ACGT", b"TGCA")
DEFAULT_PRIO = "1"  # CtxKnobs::chain_prio as the library is built (what the measurement chose)
STAT_KEYS = ("fallback_traces", "host_syncs", "pruned", "pruned_uncertified", "prelim_banded", "final_banded", "final_repeated")  # test_gpu_early_tail.three_ways


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def every_way(ctx, fn, exact=True):
    """fn() under the three priority settings and on the host-planned pipeline; returns the result under the default and its statistics"""
    assert ctx.describe()["chain_prio"] == DEFAULT_PRIO
    got = {}
    try:
        for prio in (0, 1, 2):
            ctx.set_option("chain_prio", prio)
            assert ctx.describe()["chain_prio"] == str(prio)
            got[prio] = (fn(), ctx.last_call_stats())
    finally:
        ctx.set_option("chain_prio", DEFAULT_PRIO)
    ctx.set_option("no_stream", 1)
    try:
        host, s_host = fn(), ctx.last_call_stats()
    finally:
        ctx.set_option("no_stream", 0)
    assert s_host["stream_ordered"] == 0, s_host
    base, s_base = got[0]
    for prio, (r, s) in got.items():
        assert s["stream_ordered"] == 1, (prio, s)
        same_align(r, base, exact, "chain_prio %d vs 0" % prio)
        for k in STAT_KEYS:
            assert s[k] == s_base[k], (prio, k, s, s_base)
    same_align(base, host, exact, "stream-ordered vs host-planned")
    return got[int(DEFAULT_PRIO)]


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False])
def test_headline_shape_in_miniature(ctx, exact):
    """every trace is early with both exact scores (tiers and early tail under priority); none is with the strand by certificate"""
    from tracy_amd import hostlib
    refs, profs, rev = hostlib.synth_align(311, 128, 4000, 1000, 2)
    refl = [r.tobytes() for r in refs]
    got, s = every_way(ctx, lambda: ctx.align_traces(list(profs), refl, SC, 50, 50, exact_scores=exact), exact)
    assert s["fallback_traces"] == 0 and s["pruned"] == 128 and s["prelim_banded"] == 128 and s["final_banded"] == 128, s
    assert [int(x) for x in got["forward"]] == [1 - int(r) for r in rev]


@pytest.fixture(scope="module")
def mixed():
    return mixed_batch(77)


@pytest.mark.gpu
def test_mixed_batch_of_every_kind(ctx, mixed):
    """early, short, uncertified, chimeric and refuted traces: both passes of the stages run, the early one raised"""
    profs, wins, kinds = mixed
    got, s = every_way(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50))
    assert s["pruned"] >= 48 and s["pruned_uncertified"] >= 8 and s["fallback_traces"] >= 4 + kinds.count("refuted"), s
    against_oracle(got, profs, wins, range(len(kinds)))


@pytest.mark.gpu
def test_two_lanes(ctx, mixed):
    """each lane has its own side streams and its own queue priority; the lanes inherit the options"""
    profs, wins, kinds = mixed
    ctx.set_lanes(2)
    try:
        every_way(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50, device=True))
    finally:
        ctx.set_lanes(1)


def n_run_batch(seed, count):
    """traces of 600 to 950 bases in windows that hold runs of N: in a flank, and (every other trace) inside the target below the 128
    prefix rows -- the prefixes of the voted strand take the six-code form and the tiers sweep six-code windows"""
    from test_gpu_front import noisy, profile_of, rand_seq
    rng = np.random.default_rng(seed)
    profs, wins = [], []
    for it in range(count):
        mf = int(rng.integers(600, 950))
        seq = rand_seq(rng, mf)
        target = bytearray(noisy(rng, seq, float(rng.choice([0.0, 0.02]))))
        if it % 2:
            at = int(rng.integers(250, len(target) - 80))
            run = int(rng.integers(2, 7))
            target[at:at + run] = b"N" * run
        left = rand_seq(rng, int(rng.integers(50, 1200))) + b"N" * int(rng.integers(8, 40)) + rand_seq(rng, int(rng.integers(30, 300)))
        right = rand_seq(rng, int(rng.integers(30, 300))) + (b"N" * int(rng.integers(8, 40)) if it % 3 else b"") + rand_seq(rng, int(rng.integers(50, 1200)))
        win = left + bytes(target) + right
        if it % 4 >= 2:
            win = win.translate(COMP)[::-1]
        profs.append(profile_of(rng, seq))
        wins.append(win)
    return profs, wins


@pytest.mark.gpu
def test_windows_with_runs_of_n(ctx):
    profs, wins = n_run_batch(5150, 32)
    assert all(b"NNNNNNNN" in w for w in wins)
    got, s = every_way(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50))
    assert s["pruned"] >= 24, s  # (the tiers did run over these windows)
    against_oracle(got, profs, wins, range(len(profs)))


def same_decompose(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if k in ("dcp_indel", "dcp_err"):  # raw tables: rows past dstatus[t].dcp_n are unspecified ("dcp" holds the rows written)
            continue
        if k == "bp":
            assert [(v.indelshift, v.traceleft, v.breakpoint, v.best_diff) for v in x] == [(v.indelshift, v.traceleft, v.breakpoint, v.best_diff) for v in y], what
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y), (what, k)
        elif isinstance(x, (list, tuple, dict, int, float, str, bytes)):
            assert x == y, (what, k)
        else:  # ctypes arrays of result records
            assert bytes(x) == bytes(y), (what, k)


@pytest.mark.gpu
def test_decompose_batch(ctx):
    """`tracy decompose` shares the orientation stage: its tiers run under the same rule (it has no early tail, so 2 is 1 there)"""
    from tracy_amd import capi, hostlib
    nd = 64
    d = hostlib.synth_decompose_batch(4242, nd, 1500, 520, 0)

    def run():
        hbc = capi.HostBaseCalls([d["signal"][i] for i in range(nd)], [d["bcpos"][i] for i in range(nd)],
                                 [d["primary"][i].tobytes() for i in range(nd)], [d["secondary"][i].tobytes() for i in range(nd)])
        return ctx.decompose_traces([d["profiles"][i] for i in range(nd)], hbc, [d["refs"][i].tobytes() for i in range(nd)], SC)
    ctx.set_option("chain_prio", 0)
    try:
        base = run()
        s_base = ctx.last_call_stats()
        ctx.set_option("chain_prio", 2)
        raised = run()
        s_raised = ctx.last_call_stats()
    finally:
        ctx.set_option("chain_prio", DEFAULT_PRIO)
    assert s_base["stream_ordered"] == 1 and int((np.asarray(base["status"]) == 0).sum()) > nd // 2, s_base
    ctx.set_option("no_stream", 1)
    try:
        host = run()
    finally:
        ctx.set_option("no_stream", 0)
    assert s_raised["stream_ordered"] == 1 and s_raised["pruned"] == s_base["pruned"] > 0, (s_raised, s_base)
    same_decompose(raised, base, "chain_prio 2 vs 0")
    same_decompose(host, base, "host-planned vs stream-ordered")


def test_options_without_a_device(monkeypatch):
    """CPU: the option is described, TRACYHIP_CHAIN_PRIO is read when a context's options are made, and chain_prio takes 0, 1 and 2 only"""
    from tracy_amd import capi
    monkeypatch.delenv("TRACYHIP_CHAIN_PRIO", raising=False)
    d = capi.describe_options()
    assert d["chain_prio"] == DEFAULT_PRIO and "chain_first" not in d, d  # (the order of queueing got no option: DESIGN.md section 9)
    for v in (0, 1, 2):
        assert capi.describe_options("chain_prio", v)["chain_prio"] == str(v)
    assert capi.describe_options("CHAIN_PRIO", 2)["chain_prio"] == "2"  # (names in any case)
    for bad in ("3", "7", "-1", "10", "1x", "", "two"):
        with pytest.raises(capi.TracyHipError):
            capi.describe_options("chain_prio", bad)
    monkeypatch.setenv("TRACYHIP_CHAIN_PRIO", "2")
    assert capi.describe_options()["chain_prio"] == "2"
    assert capi.describe_options("chain_prio", 1)["chain_prio"] == "1"  # (set on top of the environment)
    monkeypatch.setenv("TRACYHIP_CHAIN_PRIO", "3")  # a value the option refuses leaves the default
    assert capi.describe_options()["chain_prio"] == DEFAULT_PRIO
    assert os.environ["TRACYHIP_CHAIN_PRIO"] == "3"


@pytest.mark.gpu
def test_environment_is_read_at_context_creation(ctx, monkeypatch):
    import tracy_amd
    monkeypatch.setenv("TRACYHIP_CHAIN_PRIO", "2")
    c2 = tracy_amd.Context(0)
    try:
        assert c2.describe()["chain_prio"] == "2" and ctx.describe()["chain_prio"] == DEFAULT_PRIO
        with pytest.raises(tracy_amd.capi.TracyHipError):
            c2.set_option("chain_prio", 3)
        assert c2.describe()["chain_prio"] == "2"
    finally:
        c2.close()
