"""tracyhip_gotoh_banded (band kernels, tracy_amd/csrc/band16.h) on the GPU against the oracle: strings and profile rows, free
and paid end gaps, both strands of the origin-tracking sweep, bands chosen as the pipelines choose them."""
import random

import numpy as np
import pytest

import pyoracle as orc

pytestmark = pytest.mark.gpu
SC = (3, -5, -10, -4)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate(s, rate, rng):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(rng.choice(b"ACGT")); out.append(ch)
        elif x < rate:
            out.append(rng.choice(b"ACGTN"))
        else:
            out.append(ch)
    return bytes(out) or b"A"


def ends_of(btr, n):
    fwd = btr[::-1]
    return len(fwd) - len(fwd.lstrip(b"h")), n - (len(fwd) - len(fwd.rstrip(b"h")))


@pytest.mark.parametrize("hfree", [1, 0])
def test_banded_strings_equal_the_whole_matrix_when_the_band_holds_the_path(ctx, hfree):
    rng = random.Random(100 + hfree)
    a1, a2, lo, hi, wants = [], [], [], [], []
    for it in range(600):
        m = rng.randint(1, 1100 if it % 7 == 0 else 300)
        a = rand_seq(rng, m)
        core = mutate(a, rng.choice([0.0, 0.02, 0.08]), rng)
        b = (rand_seq(rng, rng.randint(0, 60)) + core + rand_seq(rng, rng.randint(0, 60))) if hfree else core
        ws, wb = orc.gotoh_str(a, b, hfree, 0, SC)
        n = len(b)
        if hfree:  # the band the decompose pipeline uses: around the end of the alignment, as wide as the score allows gap steps
            lead, ce = ends_of(wb, n)
            g = (SC[0] * m - ws) // 4
            d1 = ce - m
            dl, dh = d1 - g - 1, d1 + g + 1
        else:
            g = (SC[0] * m - ws) // 11 + 2
            dl, dh = -g - max(0, m - n), g + max(0, n - m)
        if dh - dl > 170:
            continue
        a1.append(a); a2.append(b); lo.append(dl); hi.append(dh); wants.append((ws, wb))
    prm = SC + (hfree, 0)
    sc, btr = ctx.align_banded(a1, a2, prm, lo, hi)
    assert len(wants) > 400
    for i, (ws, wb) in enumerate(wants):
        assert (int(sc[i]), btr[i]) == (ws, wb), (i, len(a1[i]), len(a2[i]), lo[i], hi[i])


def test_banded_origin_sweep(ctx):
    rng = random.Random(7)
    a1, a2, lo, hi, wants = [], [], [], [], []
    for it in range(500):
        m = rng.randint(5, 1000 if it % 5 == 0 else 250)
        a = rand_seq(rng, m)
        b = rand_seq(rng, rng.randint(0, 300)) + mutate(a, rng.choice([0.0, 0.05]), rng) + rand_seq(rng, rng.randint(0, 300))
        ws, wb = orc.gotoh_str(a, b, 1, 0, SC)
        lead, ce = ends_of(wb, len(b))
        g = (SC[0] * m - ws) // 4
        d1 = ce - m
        if ce == 0 or 2 * g + 2 > 170:
            continue
        a1.append(a); a2.append(b); lo.append(d1 - g - 1); hi.append(d1 + g + 1); wants.append((ws, (lead, ce)))
    sc, ends = ctx.align_banded(a1, a2, SC + (1, 0), lo, hi, origin=True)
    assert len(wants) > 300
    for i, (ws, we) in enumerate(wants):
        assert (int(sc[i]), ends[i]) == (ws, we), (i, len(a1[i]), len(a2[i]))


def test_banded_profile_rows(ctx):
    """gotoh(trace profile, _createProfile(slice)) on a band, as the final alignments of `tracy align` (sage.h:260)"""
    from tracy_amd import hostlib
    refs, profs, rev = hostlib.synth_align(4321, 40, 1400, 1000, 0)
    a1, a2, lo, hi, wants = [], [], [], [], []
    for i in range(40):
        ref = refs[i].tobytes()
        view = ref[::-1].translate(COMP) if rev[i] else ref
        p = np.ascontiguousarray(profs[i][:, :600 + 10 * i])
        m = p.shape[1]
        ws, wb = orc.gotoh_prof(p, orc.create_profile_str(view), 1, 0, SC)
        lead, ce = ends_of(wb, len(view))
        sl = view[max(0, lead - 50):min(len(view), ce + 50)]
        ws, wb = orc.gotoh_prof(p, orc.create_profile_str(sl), 1, 0, SC)
        W = 35  # (the synthetic traces lose < 4 * 35 against their row maxima)
        a1.append(p); a2.append(sl); lo.append(-W - max(0, m - len(sl))); hi.append(W + max(0, len(sl) - m)); wants.append((ws, wb))
    sc, btr = ctx.align_banded(a1, a2, SC + (1, 0), lo, hi)
    for i, (ws, wb) in enumerate(wants):
        assert (int(sc[i]), btr[i]) == (ws, wb), i


def test_banded_string_rows_outside_the_five_letters_are_refused(ctx):
    """the string tables of the band kernels know A C G T N: a row with any other byte (lower case, IUPAC, '-') is refused with
    TRACYHIP_ERR_ARG instead of being scored as a mismatch against an identical column byte (gotoh.h compares bytes, align.h:96-101);
    columns may hold anything, and the same rows in upper case go through"""
    from tracy_amd import capi
    good = b"ACGTNACGTTGCA" * 8
    col = b"ACGTRYacgt-NACGTTGCA" * 6  # columns: any byte (they mismatch every row letter they are not)
    lo, hi = [-(len(good))], [len(col)]
    band = (max(lo[0], -60), min(hi[0], 60))
    sc, btr = ctx.align_banded([good], [col], SC + (1, 0), [band[0]], [band[1]])
    assert len(btr[0]) > 0 or int(sc[0]) <= 0
    for bad in (good[:5] + b"a" + good[6:], good[:9] + b"R" + good[10:], good[:3] + b"-" + good[4:]):
        with pytest.raises(capi.TracyHipError) as e:
            ctx.align_banded([bad], [col], SC + (1, 0), [band[0]], [band[1]])
        assert e.value.code == capi.ERR_ARG and "A C G T N" in str(e.value)


# ---- band launches under a workspace limit (capi.hip run_band16 through the plan of dp_plan.h) ----------------------------------
WORD_BYTES = {4: 2, 8: 4, 12: 8}


def band_height(lo, hi):
    """b16_pick_k: the smallest strip height whose window holds the band"""
    for K in (4, 8, 12):
        if (K + hi - lo + K) // (K + 1) * (K + 1) <= 15 * (K + 1):
            return K
    return 0


def band_bytes(m, n, K, dmin, dmax):
    """bytes of traceback words of one pair: b16_store_words (band16.h) x the word size of its height, rounded up to 16"""
    KP = K + 1
    S = (K + dmax - dmin + K) // KP * KP
    NS, NB = (m + K - 1) // K, S // KP
    ext = n - ((NS - 1) * K + 1 + dmin) + 1
    NBl = max(((ext if ext > S else S) + K) // KP, NB)
    return (((NS - 1 + NB) * NB * KP + (NBl - NB) * KP) * WORD_BYTES[K] + 15) // 16 * 16


def chunks_of(job, limit):
    """the plan's cut restated: launch order is height 12, 8, 4 and the caller's order within one; a chunk closes before the pair
    that would pass the limit.  Returns the chunks as lists of heights."""
    out, cur, used = [], [], 0
    for K in (12, 8, 4):
        for a, b, lo, hi in zip(job["a1"], job["a2"], job["lo"], job["hi"]):
            if band_height(lo, hi) != K:
                continue
            need = band_bytes(len(a), len(b), K, lo, hi)
            assert need <= limit
            if cur and used + need > limit:
                out.append(cur)
                cur, used = [], 0
            cur.append(K)
            used += need
    return out + [cur]


def limit_job(hfree):
    """48 pairs, m in 40 .. 400, bands that hold the path and are widened so that every strip height occurs; the largest pair of
    height 12 (400 rows, the widest band, the longest reference) comes first"""
    rng = random.Random(4242 + hfree)
    job = dict(a1=[], a2=[], lo=[], hi=[], wants=[], ends=[])
    for it in range(48):
        m = 400 if it == 0 else rng.randint(40, 360)
        a = rand_seq(rng, m)
        core = mutate(a, 0.0 if it == 0 else rng.choice([0.0, 0.01, 0.02]), rng)
        b = (rand_seq(rng, 60 if it == 0 else rng.randint(0, 50)) + core + rand_seq(rng, 60 if it == 0 else rng.randint(0, 50))) if hfree else core
        ws, wb = orc.gotoh_str(a, b, hfree, 0, SC)
        n = len(b)
        if hfree:
            lead, ce = ends_of(wb, n)
            g = (SC[0] * m - ws) // 4
            dl, dh = ce - m - g - 1, ce - m + g + 1
        else:
            lead, ce = 0, n
            g = (SC[0] * m - ws) // 11 + 2
            dl, dh = -g - max(0, m - n), g + max(0, n - m)
        width = (183, 100, 60)[0 if it == 0 else it % 3]  # heights 12, 8, 4 (a path that needs more takes the next height up)
        while width < dh - dl:
            width = {60: 100, 100: 183}[width]
        extra = width - (dh - dl)
        dl, dh = dl - extra // 2, dh + (extra - extra // 2)
        job["a1"].append(a); job["a2"].append(b); job["lo"].append(dl); job["hi"].append(dh); job["wants"].append((ws, wb)); job["ends"].append((lead, ce))
    return job


@pytest.fixture(scope="module")
def limit_jobs():
    return {hfree: limit_job(hfree) for hfree in (1, 0)}


def reordered(job, order):
    return {key: [val[i] for i in order] for key, val in job.items()}


def trace_timer(ctx):
    from tracy_amd import capi
    import ctypes as C
    kt = capi.KernelTiming()
    capi.lib().tracyhip_timing_get(ctx._h, 1, C.byref(kt))  # TRACYHIP_TIMER_TRACE
    return int(kt.launches), int(kt.cells), int(kt.bytes)


def banded_under_limit(ctx, job, prm, limit, origin=False):
    from tracy_amd import capi
    capi.lib().tracyhip_timing_enable(ctx._h, 1)
    capi.lib().tracyhip_timing_reset(ctx._h)
    ctx.set_workspace_limit(limit)
    try:
        res = ctx.align_banded(job["a1"], job["a2"], prm, job["lo"], job["hi"], origin=origin)
        return res, trace_timer(ctx)
    finally:
        ctx.set_workspace_limit(0)
        capi.lib().tracyhip_timing_enable(ctx._h, 0)


def needed_by_pair_0(ctx, job, prm):
    from tracy_amd import capi
    ctx.set_workspace_limit(1024)
    try:
        with pytest.raises(capi.TracyHipError) as e:
            ctx.align_banded(job["a1"], job["a2"], prm, job["lo"], job["hi"])
    finally:
        ctx.set_workspace_limit(0)
    assert e.value.code == capi.ERR_OOM and "workspace limit is 1024" in str(e.value)
    return int(str(e.value).split("one pair needs ")[1].split(" bytes")[0])


@pytest.mark.parametrize("hfree", [1, 0])
def test_banded_chunks_under_a_workspace_limit(ctx, limit_jobs, hfree):
    """A limit of 1 KB holds no pair: out of memory, naming the N bytes of pair 0 (the first of height 12, so the first in launch
    order).  Under a limit of N -- pair 0 is the largest, the 48 pairs need many times N -- the call runs chunk after chunk, one launch
    each, and gives the scores and op strings of the unlimited call (one launch for the three heights) and of the whole matrix; the
    timers are credited the same cells and bytes either way.  The origin form keeps no words: one launch under any limit."""
    job = limit_jobs[hfree]
    prm = SC + (hfree, 0)
    assert {band_height(lo, hi) for lo, hi in zip(job["lo"], job["hi"])} == {4, 8, 12} and band_height(job["lo"][0], job["hi"][0]) == 12
    N = needed_by_pair_0(ctx, job, prm)
    assert N == band_bytes(len(job["a1"][0]), len(job["a2"][0]), 12, job["lo"][0], job["hi"][0])
    chunks = chunks_of(job, N)
    assert len(chunks) >= 4
    (sc0, btr0), whole = banded_under_limit(ctx, job, prm, 0)
    (sc1, btr1), cut = banded_under_limit(ctx, job, prm, N)
    assert whole[0] == 1 and cut[0] == len(chunks) and cut[1:] == whole[1:]
    for i, (ws, wb) in enumerate(job["wants"]):
        assert (int(sc0[i]), btr0[i]) == (ws, wb) and (int(sc1[i]), btr1[i]) == (ws, wb), (i, len(job["a1"][i]), len(job["a2"][i]), job["lo"][i], job["hi"][i])
    if hfree:
        (so0, e0), _ = banded_under_limit(ctx, job, prm, 0, origin=True)
        (so1, e1), _ = banded_under_limit(ctx, job, prm, 1024, origin=True)
        for i, (ws, _) in enumerate(job["wants"]):
            assert (int(so0[i]), e0[i]) == (ws, job["ends"][i]) and (int(so1[i]), e1[i]) == (ws, job["ends"][i]), i


def test_banded_chunks_of_one_height_and_across_heights(ctx, limit_jobs):
    """The same pairs reordered so that, under the limit N of pair 0, one chunk certainly holds one height and one certainly spans
    two.  Launch order is height 12, 8, 4 and the caller's order within one.  Pair 0 alone fills the first chunk (N bytes: any pair
    more passes the limit): one height.  The last two pairs of height 12 are the one with the most rows after pair 0 (z bytes) and the
    one with the fewest (x bytes), the first of height 8 is the one with the fewest rows (y bytes): z + x > N, so x opens a chunk, and
    x + y <= N, so the first pair of height 8 joins it -- a chunk of heights 12 and 8, launched at once.  (With 183 diagonals a pair of
    m rows keeps (m / 12 + 14) x 15 x 13 words of 8 bytes, about 75 KB at m = 400 and above 60 KB from m = 310 on; the smallest pairs
    keep about 30 KB at height 12 and under 10 KB at height 8.  The test restates the sizes and asserts all three inequalities.)"""
    job = limit_jobs[1]
    prm = SC + (1, 0)
    hs = [band_height(lo, hi) for lo, hi in zip(job["lo"], job["hi"])]
    rows = lambda i: len(job["a1"][i])
    h12 = sorted((i for i in range(1, 48) if hs[i] == 12), key=rows)
    h8 = sorted((i for i in range(48) if hs[i] == 8), key=rows)
    h4 = [i for i in range(48) if hs[i] == 4]
    order = [0] + h12[1:-1] + [h12[-1], h12[0]] + h8 + h4
    job = reordered(job, order)
    size = lambda i: band_bytes(len(job["a1"][i]), len(job["a2"][i]), band_height(job["lo"][i], job["hi"][i]), job["lo"][i], job["hi"][i])
    N, last12 = size(0), len(h12)
    z, x, y = size(last12 - 1), size(last12), size(last12 + 1)
    assert max(size(i) for i in range(48)) == N and z + x > N and x + y <= N
    chunks = chunks_of(job, N)
    assert chunks[0] == [12] and any(len(set(c)) > 1 for c in chunks) and any(len(set(c)) == 1 for c in chunks)
    assert needed_by_pair_0(ctx, job, prm) == N
    (sc, btr), cut = banded_under_limit(ctx, job, prm, N)
    assert cut[0] == len(chunks)
    for i, (ws, wb) in enumerate(job["wants"]):
        assert (int(sc[i]), btr[i]) == (ws, wb), (i, len(job["a1"][i]), len(job["a2"][i]), job["lo"][i], job["hi"][i])


def test_banded_reference_longer_than_the_staging_area(ctx):
    """the code rows of four pairs and the tables of the height share 64 KB of LDS: at height 12 (9216 bytes of tables) a reference
    of up to 14076 columns fits -- (n + 7) & ~3 <= 14080 -- and equals the whole matrix; one column more is TRACYHIP_ERR_RANGE"""
    from tracy_amd import capi
    n_fit = max(n for n in range(14000, 14200) if 4 * ((n + 7) & ~3) + 6 * 12 * 64 * 2 <= 64 * 1024)
    assert n_fit == 14076
    rng = random.Random(77)
    a = rand_seq(rng, 64)
    lead = 100
    for n in (n_fit, n_fit + 1):
        b = rand_seq(rng, lead) + a + rand_seq(rng, n - lead - 64)
        lo, hi = lead - 70, lead + 70
        assert band_height(lo, hi) == 12
        if n == n_fit:
            sc, btr = ctx.align_banded([a], [b], SC + (1, 0), [lo], [hi])
            assert (int(sc[0]), btr[0]) == orc.gotoh_str(a, b, 1, 0, SC)
        else:
            with pytest.raises(capi.TracyHipError) as e:
                ctx.align_banded([a], [b], SC + (1, 0), [lo], [hi])
            assert e.value.code == capi.ERR_RANGE and "reference of %d columns does not fit the staging area" % n in str(e.value)
