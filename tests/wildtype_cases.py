"""Inputs and oracle results for the edges of the two wildtype-trace paths (tracyhip_align_traces with refs of kind PROFILE,
tracyhip_decompose_traces with ref_profiles and no `oriented`), shared by tests/test_wildtype_cases.py (no GPU: the inputs hold every
case they are named for) and tests/test_gpu_wildtype_edges.py.  The oracle is tests/wildtype_oracle.py over pyoracle; every batch is
seeded and computed once per process.  The align batches are dicts of traces / wild / ridx / tl / tr / want (tl, tr: ints or per-trace
arrays); the decompose batches are dicts of traces / wild / ridx / tl / tr / want with the traces and wildtypes of
tests/test_gpu_wildtype_decompose.py."""
import functools

import numpy as np

import pyoracle as orc
import wildtype_oracle as wo
from decomp_cases import SC
from test_gpu_consensus_batch import column_profile, mutate, with_gap_row, with_n_row

SCORE = (3, -5, -10, -4)
assert tuple(SC) == SCORE
TRIM = 50


def genome(rng, n):
    return bytes(rng.choice(list(b"ACGT"), size=n).tolist())


def revcomp(p):
    return np.ascontiguousarray(orc.revcomp_profile(p))


def without_rows_4_5(w):
    w = w.copy()
    w[4:] = 0
    return w


def oracle_align(traces, wild, ridx, tl=TRIM, tr=TRIM):
    tl = np.broadcast_to(tl, len(traces))
    tr = np.broadcast_to(tr, len(traces))
    return [wo.align_trace(t, wild[int(ridx[i])], SCORE, int(tl[i]), int(tr[i])) for i, t in enumerate(traces)]


def _align(traces, wild, ridx, tl=TRIM, tr=TRIM):
    ridx = np.array(ridx, np.uint32)
    return dict(traces=traces, wild=wild, ridx=ridx, tl=tl, tr=tr, want=oracle_align(traces, wild, ridx, tl, tr))


# ---- A1: wildtypes with an N row and a gap row, read on both strands ------------------------------------------------------------
A1_LENGTHS = (300, 612, 869)  # trimmed 200 / 512 / 769: 4 rows one pass, 8 rows one pass, 8 rows two passes; full 8 x 1, 4 x 3, 8 x 2
A1_N_EVERY, A1_GAP_EVERY, A1_PERIOD = 7, 11, 5


def tandem(rng, n, period):
    """a tandem repeat of one random unit.  A read with substitutions only has ONE sensible alignment to a random genome, and rows 4
    and 5 of the wildtype then move the scores and the rows but never the path; along a repeat the end gaps of the trace may sit at any
    multiple of the period, and which one wins hangs on the weight of every column"""
    return (genome(rng, period) * (n // period + 1))[:n]


@functools.lru_cache(maxsize=None)
def a1():
    """per length one wildtype within L / 8 of L with rows 4 and 5 set, a forward trace and a reverse trace of it (ridx 0 0 1 1 2 2)"""
    rng = np.random.default_rng(4101)
    traces, wild, ridx = [], [], []
    for L in A1_LENGTHS:
        g = tandem(rng, 2 * L, A1_PERIOD)
        n = L - int(rng.integers(0, L // 8 + 1))
        s = int(rng.integers(0, L // 8 + 1))
        w = with_gap_row(rng, with_n_row(rng, column_profile(rng, g[s:s + n]), A1_N_EVERY), A1_GAP_EVERY)
        traces.append(column_profile(rng, mutate(rng, g[:L], 0.02)))
        traces.append(revcomp(column_profile(rng, mutate(rng, g[:L], 0.02))))
        ridx += [len(wild)] * 2
        wild.append(w)
    return _align(traces, wild, ridx)


@functools.lru_cache(maxsize=None)
def a1_plain_rows():
    """the A1 traces against the same wildtypes with rows 4 and 5 zeroed: what the rows must bear on"""
    b = a1()
    return oracle_align(b["traces"], [without_rows_4_5(w) for w in b["wild"]], b["ridx"])


# ---- A2: wildtype lengths ----------------------------------------------------------------------------------------------------------
A2_SHORT = (1, 2, 63, 64, 65, 127, 129)                 # columns of the wildtypes of the 140-column traces (40 rows trimmed)
A2_PAIRS = tuple((140, n) for n in A2_SHORT) + ((300, 1500), (869, 64), (869, 1500))  # (trace columns, wildtype columns)


@functools.lru_cache(maxsize=None)
def a2():
    """per (L, n) one wildtype and two traces of it, forward and reverse.  n <= L: the wildtype is cut from the trace's genome inside
    the middle of the trace's genome; n > L: the trace is cut from the middle of the wildtype's genome"""
    rng = np.random.default_rng(4102)
    traces, wild, ridx = [], [], []
    for L, n in A2_PAIRS:
        if n <= L:
            g = genome(rng, L)
            s = (L - n) // 2  # (centred: inside the trimmed view where it is shorter, around it where it is longer)
            w, tg = g[s:s + n], g
        else:
            g = genome(rng, n)
            s = (n - L) // 2
            w, tg = g, g[s:s + L]
        traces.append(column_profile(rng, mutate(rng, tg, 0.02)))
        traces.append(revcomp(column_profile(rng, mutate(rng, tg, 0.02))))
        ridx += [len(wild)] * 2
        wild.append(column_profile(rng, w))
    return _align(traces, wild, ridx)


# ---- A3: trimmed heights at the strip edges, per-trace trims ------------------------------------------------------------------------
A3_HEIGHTS = ((140, (1, 2, 63, 64, 65)), (356, (255, 256, 257)), (869, (512, 513, 768, 769)))  # (full columns, trimmed heights)
A3_CLAMPED = ((140, 0), (356, 7))                       # (full columns, l + r - mf): both clamp to 0 / 0


@functools.lru_cache(maxsize=None)
def a3():
    """every trace with a wildtype of its own of about mf columns, strands alternating, l != r"""
    rng = np.random.default_rng(4103)
    shapes = [(mf, mf - mt) for mf, hs in A3_HEIGHTS for mt in hs] + [(mf, mf + over) for mf, over in A3_CLAMPED]
    traces, wild, tl, tr = [], [], [], []
    for i, (mf, cut) in enumerate(shapes):
        g = genome(rng, 2 * mf)
        n = mf - int(rng.integers(0, mf // 8 + 1))
        s = int(rng.integers(0, mf // 8 + 1))
        t = column_profile(rng, mutate(rng, g[:mf], 0.02))
        traces.append(revcomp(t) if i % 2 else t)
        wild.append(column_profile(rng, g[s:s + n]))
        l = cut // 2 - 1 - int(rng.integers(0, max(cut // 4, 1)))
        tl.append(l)
        tr.append(cut - l)
    tl, tr = np.array(tl, np.uint32), np.array(tr, np.uint32)
    return _align(traces, wild, np.arange(len(traces)), tl, tr)


# ---- A4: more than 256 traces in one chunk ------------------------------------------------------------------------------------------
A4_TRACES, A4_COLUMNS, A4_WILD = 300, 120, (24, 27, 30, 33, 36, 38, 40)


@functools.lru_cache(maxsize=None)
def a4():
    """300 traces of 120 columns (20 trimmed) against seven shared wildtypes cut around the trimmed view, strands alternating"""
    rng = np.random.default_rng(4104)
    gs = [genome(rng, A4_COLUMNS) for _ in A4_WILD]
    wild = [column_profile(rng, g[60 - n // 2:60 - n // 2 + n]) for g, n in zip(gs, A4_WILD)]
    traces, ridx = [], []
    for i in range(A4_TRACES):
        w = i % len(wild)
        t = column_profile(rng, mutate(rng, gs[w], 0.02))
        traces.append(revcomp(t) if (i // len(wild)) % 2 else t)
        ridx.append(w)
    return _align(traces, wild, ridx)


# ---- A5: the A1 wildtypes and one nobody refers to, laid out by hand ------------------------------------------------------------
A5_ORDER = (4, 0, 2, 1, 5, 3)        # the A1 traces in this order: ref_index 2 0 1 0 2 1
A5_PADDING = (5, 0, 131)             # floats between the profiles as they lie in memory (index 3, 2, 1, 0)
A5_SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def a5():
    b = a1()
    rng = np.random.default_rng(4105)
    extra = with_gap_row(rng, with_n_row(rng, column_profile(rng, genome(rng, 77))))
    traces = [b["traces"][i] for i in A5_ORDER]
    ridx = np.array([b["ridx"][i] for i in A5_ORDER], np.uint32)
    return dict(traces=traces, wild=list(b["wild"]) + [extra], ridx=ridx, tl=TRIM, tr=TRIM, want=[b["want"][i] for i in A5_ORDER])


def a5_layout(wild):
    """(data, offset) of the wildtype set stored in reverse index order with A5_PADDING between the profiles, padding = sentinel"""
    parts, offset, pos = [], np.zeros(len(wild), np.uint64), 0
    pads = list(A5_PADDING) + [0] * len(wild)
    for k, i in enumerate(reversed(range(len(wild)))):
        offset[i] = pos
        parts.append(np.ascontiguousarray(wild[i], dtype=np.float32).reshape(-1))
        pos += parts[-1].size
        if k + 1 < len(wild):
            parts.append(np.full(pads[k], A5_SENTINEL, np.float32))
            pos += pads[k]
    return np.concatenate(parts), offset


# ---- decompose: synthetic chromatograms against basecalled wildtype chromatograms ---------------------------------------------------
# (seed, basecalls asked for, trimmed height, kind of tracyhost_synth_decompose: 0 heterozygous indel / 3 no variant, the wildtype
# holds the reverse strand).  The window is the basecalls + 300; the last entry shares the window -- and the wildtype -- of the first
D1_CASES = ((51, 300, 200, 0, False), (52, 300, 200, 3, True), (53, 356, 256, 0, False), (54, 356, 256, 3, True), (55, 357, 257, 3, False),
            (56, 357, 257, 0, True), (57, 560, 520, 0, False), (58, 560, 520, 0, True), (59, 840, 780, 0, False), (60, 840, 780, 3, True),
            (51, 280, 200, 0, False))
D1_WINDOW = {10: 600}


def _trace(seed, window, mf, kind):
    from tracy_amd import hostlib
    ref, sig, pos, indel = hostlib.synth_decompose(seed, window, mf, 25, kind, 0.6)
    pri, sec, con, bcpos = hostlib.basecall(sig, pos, 0.33)
    return ref, indel, dict(sig=sig, pos=pos, bcpos=bcpos, pri=pri, sec=sec, prof=hostlib.create_profile(sig, bcpos, pri, sec, 0, 0))


def _wildtype(ref, reverse):
    """basecalled like any trace: its profile and its primary calls are the reference"""
    from sage_oracle import revcomp as revcomp_str
    from test_gpu_wildtype_decompose import wildtype_chromatogram
    from tracy_amd import hostlib
    wsig, wpos = wildtype_chromatogram(revcomp_str(ref) if reverse else ref)
    gpri, gsec, _, gpos = hostlib.basecall(wsig, wpos, 0.33)
    return dict(primary=gpri, prof=hostlib.create_profile(wsig, gpos, gpri, gsec, 0, 0), ref=ref, reverse=reverse)


def oracle_decompose(traces, wild, ridx, tl, tr):
    return [wo.decompose_trace(t, wild[int(ridx[i])]["prof"], wild[int(ridx[i])]["primary"], SCORE, int(tl[i]), int(tr[i]))
            for i, t in enumerate(traces)]


@functools.lru_cache(maxsize=None)
def d1():
    """per trimmed height one trace against a forward and one against a reverse wildtype; the trims follow the basecalls the host chain
    made of the chromatogram (left (mf - mt) // 2, the rest right), so that the trimmed height is the one asked for"""
    traces, wild, ridx, indels, tl, tr, seen = [], [], [], [], [], [], {}
    for i, (seed, mf, mt, kind, reverse) in enumerate(D1_CASES):
        window = D1_WINDOW.get(i, mf + 300)
        ref, indel, t = _trace(seed, window, mf, kind)
        if (seed, window) not in seen:
            seen[(seed, window)] = len(wild)
            wild.append(_wildtype(ref, reverse))
        assert wild[seen[(seed, window)]]["ref"] == ref
        cut = len(t["pri"]) - mt
        traces.append(t); indels.append(indel); ridx.append(seen[(seed, window)]); tl.append(cut // 2); tr.append(cut - cut // 2)
    ridx, tl, tr = np.array(ridx, np.uint32), np.array(tl, np.uint32), np.array(tr, np.uint32)
    return dict(traces=traces, wild=wild, ridx=ridx, tl=tl, tr=tr, indels=indels, want=oracle_decompose(traces, wild, ridx, tl, tr))


D3_UNIT, D3_REPEATS = b"ACGT", 175


@functools.lru_cache(maxsize=None)
def d3():
    """a wildtype that is its own reverse complement against the first two D1 traces: both strand scores are equal, a tie is reverse.
    The oracle's chain runs on this input, so `want` holds every field; `strand` restates the strand fields from the two scores"""
    b = d1()
    s = D3_UNIT * D3_REPEATS
    w = dict(primary=s, prof=np.ascontiguousarray(orc.create_profile_str(s), dtype=np.float32), ref=s, reverse=False)
    traces, tl, tr = b["traces"][:2], b["tl"][:2], b["tr"][:2]
    ridx = np.zeros(2, np.uint32)
    want = oracle_decompose(traces, [w], ridx, tl, tr)
    strand = []
    for t, l, r in zip(traces, tl, tr):
        view = wo.trimmed_view(t["prof"], l, r)
        gf, gr, rev = wo.strand_scores(view, w["prof"], SCORE)
        strand.append(dict(score_fwd=gf, score_rev=gr, forward=int(gf > gr), score_trim=orc.gotoh_prof(view, w["prof"] if gf > gr else rev, 1, 0, SCORE)[0]))
    return dict(traces=traces, wild=[w], ridx=ridx, tl=tl, tr=tr, want=want, strand=strand)


D4_N_WILD, D4_STRANGER = 0, (4, 3)     # the D1 wildtype that gets an N row; (D1 trace, the other seed's wildtype it is paired with)


@functools.lru_cache(maxsize=None)
def d4():
    """the D1 traces of wildtype D4_N_WILD against that wildtype with an N row, and one trace against the wildtype of another seed"""
    b = d1()
    rng = np.random.default_rng(4204)
    wild = [dict(w) for w in b["wild"]]
    wild[D4_N_WILD]["prof"] = with_n_row(rng, wild[D4_N_WILD]["prof"])
    keep = [i for i in range(len(b["traces"])) if b["ridx"][i] == D4_N_WILD] + [D4_STRANGER[0]]
    traces = [b["traces"][i] for i in keep]
    ridx = np.array([D4_N_WILD] * (len(keep) - 1) + [D4_STRANGER[1]], np.uint32)
    tl, tr = b["tl"][keep], b["tr"][keep]
    return dict(traces=traces, wild=wild, ridx=ridx, tl=tl, tr=tr, keep=keep, want=oracle_decompose(traces, wild, ridx, tl, tr))
