"""Inputs and expectations for the screened consensus columns and their fix-up (consensus.h, consensus.hip), shared by
tests/test_consensus_fixup_cases.py (no GPU) and tests/test_gpu_consensus_fixup.py.

A chosen class-weight vector x is placed into a pair's consensus by building both profiles over the same base string and writing x / 2
into both at one position: halving is exact, the alignment is the diagonal, and the aligned column is fadd(x / 2, x / 2) = x.  Unaligned
columns (a leading overhang of `first`, a trailing one of `second`; end gaps are free) carry x itself.  Rows, scores and status come
from oracle_pair, letters and qualities from consensus_oracle.pairwise_consensus (the large cases: the host gtLetter on numpy float32
sums), the expected fix-up count from the host build of cons_column -- never from a device result.  test_consensus_fixup_cases.py
asserts that the inputs hold the cases they are named for and that every flag is the same under a log10 moved by 0, 1 and 4 ulp."""
import numpy as np

import pyoracle as orc
from test_consensus_host import screen
from test_gpu_consensus_batch import SCORE, column_profile, oracle_pair, passes

ULPS = (0, 1, 4)
WIDE = 4.0
F32 = np.float32


# ---- the column families: (dominant weight, second weight) as float32 -----------------------------------------------------------

def float_steps(r, k):
    """the positive float32 r moved by k representable values"""
    return (np.array([r], F32).view(np.int32) + np.int32(k)).view(F32)[0]


def half_ratio(p):
    """the float32 nearest to 10^(-(p + 0.5) / 10): -10 (gl2 - gl1) lands on p + 0.5 to within a float step"""
    return F32(10.0 ** (-(p + 0.5) / 10))


HALF_P = tuple(range(40))
HALF = tuple((F32(1), float_steps(half_ratio(p), s)) for p in HALF_P for s in (-1, 0, 1))
NOT_HALF = tuple((F32(1), float_steps(half_ratio(p), s)) for p in HALF_P for s in (-64, 64))
TENTH_A = (0.0625, 0.125, 0.25, 1.0, 2.0, 3.0, 5.0, 7.0)
TENTH = tuple((F32(9 * a), F32(a)) for a in TENTH_A)
TENTH_SMALL = TENTH[:3]  # per-trace column mass up to 1.25: a batch that holds these stays on the 16-bit score kernels
NEGATIVE = ((F32(1.25), F32(-0.25)), (F32(1.5), F32(-0.5)), (F32(1.125), F32(-0.125)))
FAMILIES = dict(half=HALF, not_half=NOT_HALF, tenth=TENTH, negative=NEGATIVE)
FLAGGED = {False: {"half", "negative"}, True: {"half", "negative", "tenth"}}  # by iupac


def weights(entry, base):
    """the six class weights (A C G T N -) of a family entry whose dominant class is `base` and whose second class is the next base"""
    x = np.zeros(6, F32)
    x[base] = entry[0]
    x[(base + 1) % 4] = entry[1]
    return x


def family_columns(name):
    """every entry of a family over the four bases in turn, float32 [n][6]"""
    return np.array([weights(e, i % 4) for i, e in enumerate(FAMILIES[name])], F32)


# ---- pairs ----------------------------------------------------------------------------------------------------------------------

def bases(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).tolist())


def revcomp(p):
    return np.ascontiguousarray(orc.revcomp_profile(p))


def crafted_pair(rng, L, aligned=(), lead=0, trail=0, over=(), delete=None, reverse=False, seq=None):
    """both profiles over one base string g of lead + L + trail columns: `first` holds g[:lead + L], `second` g[lead:] (without column
    `delete`).  aligned: (position in g, family, entry) -> x / 2 in both; over: the same inside an overhang -> x in the one profile.
    Returns dict(first, second (as handed to the library: the reverse complement where `reverse`), crafted (the strand the construction
    is on), fam1 / fam2 (family name per column of first / crafted, None for a clean column))."""
    g = seq if seq is not None else bases(rng, lead + L + trail)
    idx = [b"ACGT".index(c) for c in g]
    p1 = column_profile(rng, g[:lead + L])
    p2 = column_profile(rng, g[lead:])
    fam1, fam2 = [None] * (lead + L), [None] * (L + trail)
    for j, fam, e in aligned:
        assert lead <= j < lead + L and j != delete
        x = weights(e, idx[j])
        p1[:, j] = p2[:, j - lead] = x * F32(0.5)
        fam1[j] = fam2[j - lead] = fam
    for j, fam, e in over:
        x = weights(e, idx[j])
        if j < lead:
            p1[:, j], fam1[j] = x, fam
        else:
            assert j >= lead + L
            p2[:, j - lead], fam2[j - lead] = x, fam
    if delete is not None:
        keep = [c for c in range(L + trail) if c != delete - lead]
        p2 = np.ascontiguousarray(p2[:, keep])
        fam2 = [fam2[c] for c in keep]
    p1, p2 = np.ascontiguousarray(p1), np.ascontiguousarray(p2)
    return dict(first=p1, second=revcomp(p2) if reverse else p2, crafted=p2, fam1=fam1, fam2=fam2, reverse=reverse, lead=lead, trail=trail,
                delete=delete)


def mismatch_pair(rng, L):
    """a pair on the diagonal whose rows differ in three columns of five: there `first` holds half of a p = 0 half-family column
    (1, r) and `second` half of (r, 1) over the same two bases -- another called letter, a substitution score near zero -- and the
    other columns are negative-family ones.  Every column of both profiles is a flagged-family column."""
    t = [(j, "negative", NEGATIVE[j % 3]) if j % 5 in (0, 2) else (j, "half", HALF[j % 3]) for j in range(L)]
    p = crafted_pair(rng, L, t)
    q = p["second"].copy()
    for j in range(L):
        if p["fam2"][j] == "half":
            b = int(np.argmax(q[:, j]))
            q[b, j], q[(b + 1) % 4, j] = q[(b + 1) % 4, j], q[b, j]
    return dict(p, second=q, crafted=q)


def cycle(entries, start=0):
    k = start
    while True:
        yield entries[k % len(entries)]
        k += 1


MIX_ENTRIES = ([("half", e) for e in HALF] + [("not_half", e) for e in NOT_HALF] + [("tenth", e) for e in TENTH_SMALL]
               + [("negative", e) for e in NEGATIVE])
# overhang columns carry x itself: the entries whose column mass stays near 1 (p >= 10: r < 0.09; the negative entries: |x| sums to 2 at most)
OVER_ENTRIES = [("half", e) for e in HALF[30:]] + [("negative", e) for e in NEGATIVE]
ROUND_LENGTHS = (63, 64, 65, 128, 129)  # ops_len on both sides of a round of 64 columns of consensus_kernel
GAP_PAIR, OVER_PAIRS, SHORT_PAIR, MISMATCH_PAIR, CLEAN_PAIR, LONG_PAIR, ALL_PAIR = 6, (7, 8), 9, 11, 10, 12, 5
MIX_LIMIT = 2 << 20  # workspace limit of the chunked run (bytes)


def _lane_targets(L, it):
    """crafted columns at lanes 0 and 63 of every round of 64 the pair has, and a few between"""
    pos = sorted({j for j in list(range(0, L, 64)) + list(range(63, L, 64)) + [L - 1] + list(range(7, L, 13))})
    return [(j,) + next(it) for j in pos]


_cache = {}


def mix():
    """thirteen pairs that hold every family: five short ones around the round of 64, the 600-column pair with all 206 entries, a pair
    with a gap column, two with flagged columns in their overhangs, two that emit nothing, a clean one and a 1000-column one"""
    if "mix" in _cache:
        return _cache["mix"]
    rng = np.random.default_rng(4711)
    it = cycle(MIX_ENTRIES)
    flagged_first = cycle([("negative", NEGATIVE[0]), ("half", HALF[61]), ("negative", NEGATIVE[1]), ("half", HALF[3])])
    pairs = []
    for i, L in enumerate(ROUND_LENGTHS):
        t = _lane_targets(L, it)
        # lanes 0 and 63 and the last column carry a flagged family whatever the cycle has reached
        t = [(j,) + (next(flagged_first) if j % 64 in (0, 63) or j == L - 1 else (f, e)) for j, f, e in t]
        pairs.append(crafted_pair(rng, L, t, reverse=bool(i % 2)))
    pairs.append(crafted_pair(rng, 600, [(k * 597 // len(MIX_ENTRIES) + 1, f, e) for k, (f, e) in enumerate(MIX_ENTRIES)]))          # ALL_PAIR
    g = bases(rng, 400)
    d = next(k for k in range(200, 390) if g[k] not in (g[k - 1], g[k + 1]) and g[k + 1] != g[k + 2])
    t = [(d + 1, "negative", NEGATIVE[0]), (d - 1, "tenth", TENTH_SMALL[2])] + [(j, f, e) for j, f, e in _lane_targets(400, it) if abs(j - d) > 2]
    pairs.append(crafted_pair(rng, 400, t, delete=d, reverse=True, seq=g))                                                        # GAP_PAIR
    ov = cycle(OVER_ENTRIES)
    pairs.append(crafted_pair(rng, 300, [(40 + j, f, e) for j, f, e in _lane_targets(300, it)], lead=40, trail=30,
                              over=[(j,) + next(ov) for j in list(range(0, 40, 3)) + list(range(340, 370, 2))]))
    pairs.append(crafted_pair(rng, 350, [(70 + j, f, e) for j, f, e in _lane_targets(350, it)], lead=70, trail=64, reverse=True,
                              over=[(j,) + next(ov) for j in [0, 63, 64, 69] + list(range(5, 60, 4)) + [447, 448] + list(range(425, 445, 5)) + list(range(455, 484, 5))]))
    neg = cycle([("negative", e) for e in NEGATIVE] + [("half", e) for e in HALF[3:30:5]])
    pairs.append(crafted_pair(rng, 20, [(j,) + next(neg) for j in range(20)]))                                                    # SHORT_PAIR
    pairs.append(crafted_pair(rng, 500))                                                                                          # CLEAN_PAIR
    pairs.append(mismatch_pair(rng, 300))                                                                                         # MISMATCH_PAIR
    pairs.append(crafted_pair(rng, 1000, _lane_targets(1000, it)))                                                                # LONG_PAIR
    _cache["mix"] = pairs
    return pairs


def clean_batch():
    """six pairs of trace-like columns only: no column reaches the screen"""
    if "clean" not in _cache:
        rng = np.random.default_rng(99)
        _cache["clean"] = [crafted_pair(rng, L, lead=ld, trail=tr, reverse=rv)
                           for L, ld, tr, rv in ((300, 0, 0, False), (333, 20, 0, True), (450, 0, 31, False), (512, 5, 5, True), (600, 0, 0, False), (64, 0, 0, False))]
    return _cache["clean"]


# the list overflow: one 1000-column pair whose every column is flagged with IUPAC (negative and tenth entries in turn), OVERFLOW_COPIES
# times in one batch.  fix_cap = max(65536, 4 npairs) = max(65536, 288) = 65536 entries; the batch flags 72 x 1000 = 72000 > 65536, so
# the first pass counts 72000, writes 65536, and the consensus stage runs again with a list of 72000.
OVERFLOW_LEN = 1000
OVERFLOW_COPIES = 72
OVERFLOW_COUNT = OVERFLOW_COPIES * OVERFLOW_LEN
FIX_CAP = 65536


def overflow_pair():
    if "overflow" not in _cache:
        rng = np.random.default_rng(65536)
        it = cycle([("negative", e) for e in NEGATIVE] + [("tenth", e) for e in TENTH_SMALL])
        _cache["overflow"] = crafted_pair(rng, OVERFLOW_LEN, [(j,) + next(it) for j in range(OVERFLOW_LEN)])
    return _cache["overflow"]


# the device's log10 over many columns: LOG10_PAIRS pairs of LOG10_LEN columns, a crafted column of every family at every eighth position
LOG10_PAIRS, LOG10_LEN, LOG10_EVERY = 64, 512, 8
LOG10_SAMPLE = (0, 21, 42, 63)
LOG10_ENTRIES = ([("half", e) for e in HALF] + [("not_half", e) for e in NOT_HALF] + [("tenth", e) for e in TENTH] + [("negative", e) for e in NEGATIVE])


def log10_batch():
    if "log10" not in _cache:
        rng = np.random.default_rng(1010)
        it = cycle(LOG10_ENTRIES)
        _cache["log10"] = [crafted_pair(rng, LOG10_LEN, [(j,) + next(it) for j in range(3, LOG10_LEN, LOG10_EVERY)]) for _ in range(LOG10_PAIRS)]
    return _cache["log10"]


def diagonal_columns(pair):
    """the aligned columns of a pair on the diagonal: numpy's float32 sum IS __fadd_rn.  float32 [n][6]"""
    return np.ascontiguousarray((pair["first"] + pair["crafted"]).T)


def firsts(pairs):
    return [p["first"] for p in pairs]


def seconds(pairs):
    return [p["second"] for p in pairs]


def scaled(profiles):
    return [np.ascontiguousarray(p * F32(WIDE)) for p in profiles]


# ---- expectations ---------------------------------------------------------------------------------------------------------------

def emitted(want, pair, union, scale=1.0):
    """the columns a pair's consensus emits, from the oracle's rows: (weights float32 [n][6], alignment column of each, family of each,
    'aligned' / 'first' / 'second' of each).  A column that pairs a crafted position with another one has the family 'broken'."""
    if want["status"] != 0:
        return np.zeros((0, 6), F32), [], [], []
    p1 = pair["first"] * F32(scale)
    p2 = pair["crafted"] * F32(scale)
    assert want["forward"] == (0 if pair["reverse"] else 1)
    cl, col, fam, side = [], [], [], []
    s1 = s2 = 0
    for j, (a, b) in enumerate(zip(*want["rows"])):
        g0, g1 = a == ord("-"), b == ord("-")
        if not g0 and not g1:
            cl.append(p1[:, s1] + p2[:, s2])
            f1, f2 = pair["fam1"][s1], pair["fam2"][s2]
            fam.append(f1 if f1 == f2 else "broken")
            col.append(j)
            side.append("aligned")
        else:
            if not g0 and union:
                cl.append(p1[:, s1]); fam.append(pair["fam1"][s1]); col.append(j); side.append("first")
            if not g1 and union:
                cl.append(p2[:, s2]); fam.append(pair["fam2"][s2]); col.append(j); side.append("second")
        s1 += not g0
        s2 += not g1
    return np.array(cl, F32).reshape(-1, 6), col, fam, side


def expectation(cc, pairs, union=True, iupac=False, scale=1.0, key=None):
    """per pair: the oracle's result (`want`), the emitted columns and the flag of each under the host build of cons_column with
    glibc's log10; `count` is the number of flagged emitted columns of the batch"""
    k = (key, union, iupac, scale)
    if key is not None and k in _cache:
        return _cache[k]
    out = dict(want=[], cols=[], flags=[], per_pair=[])
    for p in pairs:
        first, second = p["first"] * F32(scale), p["second"] * F32(scale)
        w = oracle_pair(np.ascontiguousarray(first), np.ascontiguousarray(second), SCORE, union, iupac, 25, 0.5)
        e = emitted(w, p, union, scale)
        f = screen(cc, e[0], iupac, 0)[2] if len(e[0]) else np.zeros(0, bool)
        out["want"].append(w)
        out["cols"].append(e)
        out["flags"].append(f)
        out["per_pair"].append(int(f.sum()))
    out["count"] = sum(out["per_pair"])
    if key is not None:
        _cache[k] = out
    return out


def stable_flags(cc, cl, iupac):
    """the flags of cons_column under a log10 moved by 0, 1 and 4 ulp, asserted identical"""
    f = [screen(cc, cl, iupac, u)[2] for u in ULPS]
    assert np.array_equal(f[0], f[1]) and np.array_equal(f[0], f[2]), np.flatnonzero((f[0] != f[1]) | (f[0] != f[2]))[:10]
    return f[0]


def pair_need(m, n):
    """bytes of traceback planes and boundary rows of one pair (consensus_run's chunk planning)"""
    P = passes(m)
    return 8 * (P * (n + 63) * 64 + (2 * (n + 2) if P > 1 else 0))


def mass_bound(profiles):
    """the largest column mass (sum of |entries| of rows 0 .. 4) the score kernels report for a profile set, at least 1.001"""
    return max(1.001, max(float(np.abs(p[:5]).sum(0).max()) for p in profiles))


def largest_sub(first, second):
    """range_verdict's bound of a substitution score for scoring 3/-5: masses x 5 x 1.0001 + 1, rounded up"""
    return max(5, int(mass_bound(first) * mass_bound(second) * 5 * 1.0001 + 1.0) + 1)
