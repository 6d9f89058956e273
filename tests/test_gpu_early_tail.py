"""The early tail of the stream-ordered `tracy align` call (tracy_amd/csrc/stream.hip: s_orient_early_kernel, AlignStream::queue_stages).
A trace whose clear k-mer vote was certified by a tier of its pruned sweep gets its preliminary and final alignment queued for the
voted strand on the side stream, beside the other strand's full sweep; the decision with both exact scores then confirms it or
gives it the verdict a wrong clear vote has always had (the host-planned tiers redo it).  Every other trace takes the same stages
behind the decision.  Option no_early_tail sends every trace that way: the order before the early tail.

Every case runs with the option off, on, and on the host-planned pipeline (no_stream), and every ALIGN_KEYS array and `btr` of every
trace must be the same in all three."""
import numpy as np
import pytest

SC = (3, -5, -10, -4)
COMP = bytes.maketrans(b"ACGT", b"TGCA")
ALIGN_KEYS = ("forward", "score_fwd", "score_rev", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final")
ORACLE_KEYS = ("forward", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final")
VOTE_K = 11  # pipe_kernels.h kVoteK


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def same_align(a, b, exact, what=""):
    keys = ALIGN_KEYS if exact else tuple(k for k in ALIGN_KEYS if k not in ("score_fwd", "score_rev"))
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k, np.nonzero(np.asarray(a[k]) != np.asarray(b[k]))[0][:8])
    assert len(a["btr"]) == len(b["btr"]) and a["btr"] == b["btr"], what


def three_ways(ctx, fn, exact=True):
    """fn() with the early tail, without it (no_early_tail) and on the host-planned pipeline (no_stream): the three results are
    compared in full; returns (result, stats with the early tail, stats without it, the host-planned result)"""
    assert ctx.describe()["no_early_tail"] == "0"
    early = fn()
    s_early = ctx.last_call_stats()
    ctx.set_option("no_early_tail", 1)
    try:
        assert ctx.describe()["no_early_tail"] == "1"
        late = fn()
        s_late = ctx.last_call_stats()
    finally:
        ctx.set_option("no_early_tail", 0)
    ctx.set_option("no_stream", 1)
    try:
        host = fn()
        s_host = ctx.last_call_stats()
    finally:
        ctx.set_option("no_stream", 0)
    assert s_early["stream_ordered"] == 1 and s_late["stream_ordered"] == 1 and s_host["stream_ordered"] == 0, (s_early, s_late, s_host)
    same_align(early, late, exact, "early tail vs no_early_tail")
    same_align(early, host, exact, "early tail vs host-planned")
    same_align(late, host, exact, "no_early_tail vs host-planned")
    # what the call reports of its stages does not depend on the pass a trace took
    for k in ("fallback_traces", "host_syncs", "pruned", "pruned_uncertified", "prelim_banded", "final_banded", "final_repeated"):
        assert s_early[k] == s_late[k], (k, s_early, s_late)
    return early, s_early, s_late, host


def against_oracle(got, profs, wins, which, keys=ORACLE_KEYS + ("score_fwd", "score_rev")):
    import sage_oracle as so
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(16) as pool:
        want = list(pool.map(lambda i: so.align_trace(profs[i], wins[i], SC, 50, 50), which))
    for i, w in zip(which, want):
        for k in keys:
            assert int(got[k][i]) == int(w[k]), (i, k)
        assert got["btr"][i] == w["btr"], i
    return want


def short_traces(rng, count):
    """deferred by geometry: 200 bases, trims 50 / 50 leave 100 rows -- no more than the 128 prefix rows of a pruned sweep, so
    s_orient_class puts the trace in class 1 (both strands in full) whatever its vote"""
    from test_gpu_front import noisy, profile_of, rand_seq
    out = []
    for it in range(count):
        seq = rand_seq(rng, 200)
        win = rand_seq(rng, int(rng.integers(100, 1200))) + noisy(rng, seq, float(rng.choice([0.0, 0.02]))) + rand_seq(rng, int(rng.integers(100, 1200)))
        if it % 2:
            win = win.translate(COMP)[::-1]
        out.append((profile_of(rng, seq), win))
    return out


def refuted_trace(rng, voted_reverse):
    """A clear vote for the strand that loses.  Voted strand: the trimmed trace without its first 100 rows, exact -- about 690 shared
    11-mers, and nothing lost below the 128 prefix rows; the 28 prefix rows that do match put the maximum of the kept row in the
    right column (the 100 rows without a partner cost about 2 a row against the random flank, as the whole prefix does in every
    other column), so the first tier of the pruned sweep certifies it.  Those 100 rows are what it loses: about 440.  Other strand:
    the whole trace with a substitution every 18 bases -- 7 positions in 18 keep their 11-mer (about 310 votes, less than half), and
    the substitutions cost about 310 over the trimmed trace: the un-voted strand wins by about 100 to 140 (oracle: 1070-1103 against
    1192-1221).  Any positive margin refutes the vote; a larger one needs more rows without a partner, and then the kept row's
    maximum is no longer the trace's column."""
    from test_gpu_front import profile_of, rand_seq
    mf = 900
    seq = rand_seq(rng, mf)
    spaced = bytearray(seq)
    for j in range(7, mf, 18):
        spaced[j] = b"ACGT"[(b"ACGT".index(spaced[j]) + 1 + int(rng.integers(0, 3))) % 4]
    voted = seq[50 + 100:mf - 50]
    other = bytes(spaced).translate(COMP)[::-1]
    win = rand_seq(rng, int(rng.integers(200, 600))) + voted + rand_seq(rng, int(rng.integers(300, 500))) + other + rand_seq(rng, int(rng.integers(200, 600)))
    if voted_reverse:
        win = win.translate(COMP)[::-1]
    return profile_of(rng, seq), win, seq


def votes_of(seq, win):
    """window positions whose 11-mer occurs in the trimmed trace, read forward / as the reverse complement (kmer_vote_kernel without
    its hash collisions)"""
    t = seq[50:len(seq) - 50]
    fw = {t[i:i + VOTE_K] for i in range(len(t) - VOTE_K + 1)}
    rc = {k.translate(COMP)[::-1] for k in fw}
    vf = sum(win[i:i + VOTE_K] in fw for i in range(len(win) - VOTE_K + 1))
    vr = sum(win[i:i + VOTE_K] in rc for i in range(len(win) - VOTE_K + 1))
    return vf, vr


def refuted_batch(rng, count):
    return [refuted_trace(rng, bool(i % 2)) for i in range(count)]


def test_refuted_construction_votes_for_the_strand_that_loses():
    """CPU only: by the oracle, `forward` of every constructed trace is the strand its clear vote (s_orient_class's rule) does not name"""
    import sage_oracle as so
    rng = np.random.default_rng(2024)
    for i, (prof, win, seq) in enumerate(refuted_batch(rng, 4)):
        vf, vr = votes_of(seq, win)
        hi, lo = max(vf, vr), min(vf, vr)
        assert hi >= 32 and hi >= 2 * lo + 40, (i, vf, vr)  # clear, with room for the bitmap's hash collisions
        voted_forward = vf >= vr
        assert voted_forward == (i % 2 == 0), (i, vf, vr)
        w = so.align_trace(prof, win, SC, 50, 50)
        assert bool(w["forward"]) != voted_forward, (i, w["score_fwd"], w["score_rev"])
        assert abs(int(w["score_fwd"]) - int(w["score_rev"])) >= 60, (i, w["score_fwd"], w["score_rev"])


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False])
def test_headline_shape_in_miniature(ctx, exact):
    """every trace is early (a clear vote, certified in the first tier): nothing is left for the pass behind the decision, nothing
    falls back, and the call synchronises as often as without the early tail.  exact = False: strand_by_certificate, where no trace is
    early (there is no full sweep to run beside) and the option changes nothing"""
    from tracy_amd import hostlib
    refs, profs, rev = hostlib.synth_align(311, 128, 4000, 1000, 2)
    refl = [r.tobytes() for r in refs]
    assert 0 < int(rev.sum()) < len(rev)  # both strands
    got, s_early, s_late, _ = three_ways(ctx, lambda: ctx.align_traces(list(profs), refl, SC, 50, 50, exact_scores=exact), exact)
    assert s_early["fallback_traces"] == 0 and s_late["fallback_traces"] == 0, (s_early, s_late)
    assert s_early["host_syncs"] == s_late["host_syncs"], (s_early, s_late)
    assert s_early["pruned"] == 128 and s_early["prelim_banded"] == 128 and s_early["final_banded"] == 128, s_early
    assert [int(x) for x in got["forward"]] == [1 - int(r) for r in rev]


def mixed_batch(seed):
    """early traces (plain ones among test_gpu_front's cases), traces deferred by geometry (short: class 1), traces deferred because
    no tier certified them, chimeras and the like (the rest of the cases) and refuted ones"""
    from test_gpu_front import cases
    cs = cases(np.random.default_rng(77))  # (the generator is written for this seed: others draw an empty range)
    rng = np.random.default_rng(seed)
    profs, wins = [c[0] for c in cs], [c[1] for c in cs]
    short = short_traces(rng, 32)
    ref = refuted_batch(rng, 8)
    kinds = [c[2] for c in cs] + ["short"] * len(short) + ["refuted"] * len(ref)
    profs += [s[0] for s in short] + [r[0] for r in ref]
    wins += [s[1] for s in short] + [r[1] for r in ref]
    order = rng.permutation(len(profs))  # the kinds interleaved: the passes' lists are not runs of the batch
    return [profs[i] for i in order], [wins[i] for i in order], [kinds[i] for i in order]


@pytest.mark.gpu
def test_mixed_batch_of_every_kind(ctx):
    profs, wins, kinds = mixed_batch(77)
    nshort = kinds.count("short")
    assert 4 * nshort >= len(kinds)  # at least a quarter deferred by geometry
    got, s_early, s_late, _ = three_ways(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50))
    assert 48 + kinds.count("refuted") <= s_early["pruned"] <= len(kinds) - nshort, s_early  # (the short ones are class 1 whatever their vote)
    assert 8 <= s_early["pruned_uncertified"] <= s_early["pruned"] - 24, s_early  # deferred because the tiers failed, and early ones
    assert s_early["fallback_traces"] >= 4 + kinds.count("refuted"), s_early
    against_oracle(got, profs, wins, range(len(kinds)))


@pytest.mark.gpu
def test_refuted_traces_take_the_host_planned_tiers(ctx):
    """Clear votes for the strand that loses, certified by a front tier (pruned_uncertified == 0: every trace of the batch is early,
    so the refuted ones have had their alignments queued -- and written -- for the wrong strand).  The confirming decision gives each
    SD_LOSER_WON; they are counted in fallback_traces and not in prelim_banded / final_banded, and every array is the oracle's."""
    from tracy_amd import hostlib
    rng = np.random.default_rng(2024)
    ref = refuted_batch(rng, 12)
    refs, sprofs, rev = hostlib.synth_align(99, 36, 3000, 900, 2)
    profs = [r[0] for r in ref] + list(sprofs)
    wins = [r[1] for r in ref] + [r.tobytes() for r in refs]
    got, s_early, s_late, _ = three_ways(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50))
    assert s_early["pruned"] == len(profs) and s_early["pruned_uncertified"] == 0, s_early
    assert s_early["fallback_traces"] == len(ref) and s_late["fallback_traces"] == len(ref), (s_early, s_late)
    assert s_early["prelim_banded"] == len(sprofs) and s_early["final_banded"] == len(sprofs), s_early
    want = against_oracle(got, profs, wins, range(len(profs)))
    for i in range(len(ref)):
        assert int(want[i]["forward"]) == i % 2, i  # even: voted forward, so the reverse strand wins


@pytest.mark.gpu
def test_nothing_of_a_call_survives_it(ctx):
    """mixed, uniform, mixed on one context: no early mark, list or counter of a call is seen by the next (the uniform batch is as long
    as the mixed one, so every slot is visited with a different verdict) -- each equals a fresh context's and the host-planned result"""
    import tracy_amd
    from tracy_amd import hostlib
    profs, wins, kinds = mixed_batch(78)
    refs, uprofs, rev = hostlib.synth_align(132, len(kinds), 3500, 900, 2)
    mixed = (profs, wins)
    uniform = (list(uprofs), [r.tobytes() for r in refs])
    got = [ctx.align_traces(p_, w_, SC, 50, 50) for p_, w_ in (mixed, uniform, mixed)]
    stats_again = ctx.last_call_stats()
    fresh = tracy_amd.Context(0)
    try:
        first = fresh.align_traces(mixed[0], mixed[1], SC, 50, 50)
        stats_first = fresh.last_call_stats()
    finally:
        fresh.close()
    fresh = tracy_amd.Context(0)
    try:
        second = fresh.align_traces(uniform[0], uniform[1], SC, 50, 50)
    finally:
        fresh.close()
    same_align(got[0], first, True, "mixed")
    same_align(got[1], second, True, "uniform after mixed")
    same_align(got[2], first, True, "mixed after uniform")
    for k in ("fallback_traces", "pruned", "pruned_uncertified", "prelim_banded", "final_banded"):
        assert stats_again[k] == stats_first[k], (k, stats_again, stats_first)
    ctx.set_option("no_stream", 1)
    try:
        want = [ctx.align_traces(p_, w_, SC, 50, 50) for p_, w_ in (mixed, uniform)]
    finally:
        ctx.set_option("no_stream", 0)
    same_align(got[0], want[0], True, "mixed vs host-planned")
    same_align(got[1], want[1], True, "uniform vs host-planned")


@pytest.mark.gpu
def test_two_lanes(ctx):
    """set_lanes(2): each lane has side streams of its own, and the early tails of two calls run side by side"""
    profs, wins, kinds = mixed_batch(79)
    ctx.set_lanes(2)
    try:
        three_ways(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50, device=True))
    finally:
        ctx.set_lanes(1)


@pytest.mark.gpu
def test_strand_by_certificate(ctx):
    """exact_scores = False on the mixed batch: no trace is early, every one takes the pass behind the decision"""
    profs, wins, kinds = mixed_batch(80)
    got, s_early, s_late, _ = three_ways(ctx, lambda: ctx.align_traces(profs, wins, SC, 50, 50, exact_scores=False), exact=False)
    against_oracle(got, profs, wins, range(len(kinds)), ORACLE_KEYS)
