"""Cases for Needleman-Wunsch on the device (tracyhip_needle_score / tracyhip_needle_align: needle_body, needle_walk_one, needle_step,
SubProfD): string and profile pairs at every strip height the host may choose and on both sides of every pass edge, the scorings and
AlignConfigs they run under, and restatements of the two host rules that decide which kernel a pair reaches.  Shared by
tests/test_emu_needle.py (CPU, the wave emulator) and tests/test_gpu_needle.py."""
import functools

import numpy as np

# (match, mismatch, go, ge); needle.h reads match, mismatch and ge only
SCORINGS = [(5, -4, -10, -1),
            (5, -4, -10, -2),  # mismatch = 2 ge: a diagonal step and a pair of gaps tie
            (0, 0, 0, 0),      # every cell ties three ways: the tie order hor > ver > diag decides all of them
            (1, -1, 0, -1)]
CONFIGS = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (hfree, vfree)
TALL = 513  # scorings 2 and 3 run on the cases of at most this many rows, and on one case of every (strip height, passes) class

STRING_ROWS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 769, 1023, 1024, 1025, 1281, 1793, 2048, 2049)
STRING_COLS = (0, 1, 2, 63, 64, 65, 130)
PROFILE_ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 512, 513, 768, 769, 1024, 1025, 1281)
PROFILE_COLS = (1, 64, 65, 97)
KINDS = ("random", "onehot", "dyadic", "x37.5", "minus0.3", "row5")
MAX_CELLS = 2049 * 130


# ---- the host's rules (capi.hip choose_k, dp_lane.h num_passes, dp_plan.h sweep_words), restated ----
def passes(m, K):
    return (m + 64 * K - 1) // (64 * K)


def strip_height(m, prof):
    """smallest passes x K over the strip heights compiled for needle; the first of (16, 8, 4) / (8, 4) wins a tie"""
    best, cost = None, None
    for K in ((8, 4) if prof else (16, 8, 4)):
        c = passes(max(m, 1), K) * K
        if cost is None or c < cost:
            best, cost = K, c
    return best


def lanes_used(m, prof):
    K = strip_height(m, prof)
    return (min(m, 64 * K) + K - 1) // K


def trace_bytes(m, n, prof):
    """bytes of traceback words a pair needs (4-byte words, one per lane and step; none for an empty side)"""
    return passes(m, strip_height(m, prof)) * (n + 63) * 64 * 4 if m and n else 0


def planned_chunks(cases, limit):
    """dp_plan.h sweep_plan + chunk_cut.h for a traceback call under a workspace limit, restated: the pairs ordered by strip height, then
    by cells, both descending and stably; a chunk of consecutive pairs closes before the pair whose words would pass the limit"""
    prof = is_prof(cases[0])
    key = lambda c: (-strip_height(shape(c)[0], prof), -shape(c)[0] * shape(c)[1])
    chunks, used = [[]], 0
    for c in sorted(cases, key=key):
        need = trace_bytes(*shape(c), prof)
        assert need <= limit
        if chunks[-1] and used + need > limit:
            chunks.append([])
            used = 0
        chunks[-1].append(c)
        used += need
    return chunks


def shape(case):
    """(m, n) of a case"""
    _, a, b = case
    return (len(a), len(b)) if isinstance(a, bytes) else (a.shape[1], b.shape[1])


def is_prof(case):
    return not isinstance(case[1], bytes)


def klass(case):
    """(strip height, more than one pass) of a case whose kernel sweeps cells, else None"""
    m, n = shape(case)
    if m == 0 or n == 0:
        return None
    K = strip_height(m, is_prof(case))
    return K, passes(m, K) > 1


STRING_CLASSES = {(K, s) for K in (4, 8, 16) for s in (False, True)}
PROFILE_CLASSES = {(K, s) for K in (4, 8) for s in (False, True)}
# (strip height, passes) by rows, derived by hand from the rule
STRING_BY_HAND = {256: (4, 1), 257: (8, 1), 512: (8, 1), 513: (4, 3), 769: (16, 1), 1024: (16, 1), 1281: (8, 3), 1793: (16, 2),
                  2048: (16, 2), 2049: (4, 9)}
PROFILE_BY_HAND = {257: (8, 1), 513: (4, 3), 769: (8, 2), 1024: (8, 2)}


def classes(cases):
    return {klass(c) for c in cases} - {None}


def representatives(cases):
    """per class the case of the fewest cells among those of 63 columns and more: where every config x scoring runs"""
    rep = {}
    for c in cases:
        k = klass(c)
        if k is not None and shape(c)[1] >= 63 and (k not in rep or np.prod(shape(c)) < np.prod(shape(rep[k]))):
            rep[k] = c
    return [rep[k] for k in sorted(rep)]


def cases_of_scoring(cases, si):
    """the cases scoring SCORINGS[si] runs on"""
    if si < 2:
        return list(cases)
    reps = {c[0] for c in representatives(cases)}
    return [c for c in cases if shape(c)[0] <= TALL or c[0] in reps]


def interleaved(cases):
    """the cases in an order where neighbours have different strip heights as long as more than one height has cases left"""
    buckets = {}
    for c in cases:
        buckets.setdefault(strip_height(shape(c)[0], is_prof(c)), []).append(c)
    out = []
    while any(buckets.values()):
        for K in sorted(buckets):
            if buckets[K]:
                out.append(buckets[K].pop(0))
    return out


# ---- strings ----
def rand_bytes(rng, n, alpha):
    return bytes(rng.choice(list(alpha), size=n).tolist()) if n else b""


def noisy_copy(rng, s, m, alpha, rate=0.06):
    """m bytes copied from s (repeated to length) with substitutions, insertions and deletions: long diagonals, short gaps"""
    src = (s * (m // max(len(s), 1) + 2))[:m + 16] if s else rand_bytes(rng, m + 16, alpha)
    out = bytearray()
    for ch in src:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(rng.choice(list(alpha))))
        out.append(int(rng.choice(list(alpha))) if u > 1 - rate / 3 else ch)
    return (bytes(out) + rand_bytes(rng, m, alpha))[:m]


def string_shapes():
    """every m with n = 1, with the largest n below its lanes in use (the last step is then set by the lanes, not by n), with n = 65
    and with one more n in rotation; and the empty sides"""
    out = [(0, 0), (0, 7), (9, 0)]
    for i, m in enumerate(STRING_ROWS):
        ns = [1, 65, STRING_COLS[i % len(STRING_COLS)]]
        if m:
            ns.insert(1, max(n for n in (0, 1, 2, 63) if n < lanes_used(m, False)))
        for n in dict.fromkeys(ns):
            if (m, n) not in out:
                out.append((m, n))
    return out


@functools.lru_cache(maxsize=None)
def string_cases():
    """[(name, s1, s2)]: alphabets A (every cell ties), AC and ACGTN in rotation, every other pair a noisy copy, the rest unrelated; and one
    pair of arbitrary bytes (0x00, 0xff, lower case: the kernels compare bytes, and the row sentinel is -1)"""
    rng = np.random.default_rng(20261)
    out = []
    for j, (m, n) in enumerate(string_shapes()):
        alpha = (b"A", b"AC", b"ACGTN")[j % 3]
        noisy = (j // 3) % 2 == 1
        s2 = rand_bytes(rng, n, alpha)
        s1 = noisy_copy(rng, s2, m, alpha) if noisy else rand_bytes(rng, m, alpha)
        out.append(("%dx%d-%s-%s" % (m, n, alpha.decode(), "copy" if noisy else "apart"), s1, s2))
    odd = bytes([0x00, 0xff, 0x80, 0x7f]) + b"aAcCgN-"
    s2 = rand_bytes(rng, 130, odd)
    out.append(("600x130-bytes-copy", noisy_copy(rng, s2, 600, odd), s2))
    assert len({c[0] for c in out}) == len(out)
    assert all(len(a) * len(b) <= MAX_CELLS for _, a, b in out)
    return tuple(out)


# ---- profiles ----
def profile_of_kind(rng, n, kind):
    p = np.zeros((6, n), dtype=np.float32)
    x = rng.random((5, n)).astype(np.float32) ** 4  # a called base stands out; row 4 ('N') carries weight
    norm = x / x.sum(axis=0, keepdims=True)
    if kind == "onehot":
        p[rng.choice(5, size=n, p=[0.24, 0.24, 0.24, 0.24, 0.04]), np.arange(n)] = 1.0
    elif kind == "dyadic":  # two halves per column (in one row or two): every product and partial sum is exact
        for _ in range(2):
            np.add.at(p, (rng.integers(0, 5, n), np.arange(n)), np.float32(0.5))
    elif kind == "x37.5":
        p[:5] = norm * np.float32(37.5)
    elif kind == "minus0.3":  # negative entries: negative accumulators, truncation toward zero
        p[:5] = norm - np.float32(0.3)
    else:
        p[:5] = norm
        if kind == "row5":  # the 5 x 5 sum must not read the gap row
            p[5] = (40.0 * rng.random(n) + 1.0).astype(np.float32)
    return p


def resampled(rng, p, n):
    """n columns of p in order, a few skipped and a few doubled"""
    idx, pos = [], 0
    for _ in range(n):
        u = rng.random()
        pos += u < 0.03
        idx.append(pos % p.shape[1])
        pos += u < 0.97
    return np.ascontiguousarray(p[:, idx])


@functools.lru_cache(maxsize=None)
def profile_cases():
    """[(name, p1, p2)] float32 [6][len]: every m with three of the four n, the kinds in rotation (both profiles of a pair of one kind),
    every other pair with p2 resampled from p1"""
    rng = np.random.default_rng(20262)
    out = []
    j = 0
    for i, m in enumerate(PROFILE_ROWS):
        for n in PROFILE_COLS[:i % 4] + PROFILE_COLS[i % 4 + 1:]:
            kind = KINDS[j % len(KINDS)]
            copy = (j // len(KINDS)) % 2 == 1
            p1 = profile_of_kind(rng, m, kind)
            p2 = resampled(rng, p1, n) if copy else profile_of_kind(rng, n, kind)
            for p in (p1, p2):
                p.setflags(write=False)
            out.append(("%dx%d-%s-%s" % (m, n, kind, "copy" if copy else "apart"), p1, p2))
            j += 1
    return tuple(out)


def kind_of(case):
    return case[0].split("-", 1)[1].rsplit("-", 1)[0]


def assert_every_kernel_is_reached():
    """the ten needle kernels, in trace form and in score form (both forms run on every case): strings at strip heights 4, 8 and 16,
    profiles at 4 and 8, each in one pass and in several.  The hand derivation pins the restated rule; where the two disagreed the rule
    would be right and the sizes would have to move."""
    for m, want in STRING_BY_HAND.items():
        assert (strip_height(m, False), passes(m, strip_height(m, False))) == want, m
    for m, want in PROFILE_BY_HAND.items():
        assert (strip_height(m, True), passes(m, strip_height(m, True))) == want, m
    assert classes(string_cases()) == STRING_CLASSES
    assert classes(profile_cases()) == PROFILE_CLASSES
    # every kind of profile in several passes, every alphabet too
    several = {kind_of(c) for c in profile_cases() if (klass(c) or (0, False))[1]}
    assert several == set(KINDS), several
    assert {c[0].split("-")[1] for c in string_cases() if (klass(c) or (0, False))[1]} >= {"A", "AC", "ACGTN", "bytes"}
    for m in STRING_ROWS:
        ns = {shape(c)[1] for c in string_cases() if shape(c)[0] == m}
        assert {1, 65} <= ns and (m == 0 or any(n < lanes_used(m, False) for n in ns)), m
    assert {(0, 0), (0, 7), (9, 0)} <= {shape(c) for c in string_cases()}
