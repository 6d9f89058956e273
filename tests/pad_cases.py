"""Cases for the trace padding stage (tracyhip_pad_traces: hard trim trim.h:77-99, reverseComplementTrace trim.h:125-150,
alignmentTracePadding json.h:383-472) and what the Python restatements of tests/assemble_oracle.py and tests/sage_oracle.py give for
them -- tests only.  A case is a dict: sig int [4][ns], bcpos, pri / sec / con (bytes), q (list), row (bytes), l, r, reverse."""
import numpy as np

import assemble_oracle as ao
import sage_oracle as so

OK, DEFERRED, TOO_SMALL = 0, 1, 2
MAX_CALLS = 131071
COMPLEMENT_FROM = b"ACGTNHVMYDBKRUSW"
FIELDS = ("bcPos", "primary", "secondary", "consensus", "estQual")


def make(bcpos, row, ns=None, l=0, r=0, reverse=False, seed=0, letters=None):
    rng = np.random.default_rng(1000 + seed)
    n = len(bcpos)
    if ns is None:
        ns = (max(bcpos) if n else 0) + 1 + int(rng.integers(0, 6))
    sig = rng.integers(-200, 3000, size=(4, ns)).astype(np.int32)
    alphabet = np.frombuffer(b"ACGTNRYKMSWBDHVU", np.uint8)
    pick = lambda: (bytes(rng.choice(alphabet, n)) if letters is None else bytes(letters[:n]))
    return dict(sig=sig, bcpos=[int(x) for x in bcpos], pri=pick(), sec=pick() if letters is None else bytes(letters[:n])[::-1],
                con=pick(), q=[int(x) for x in rng.integers(0, 61, n)], row=bytes(row), l=int(l), r=int(r), reverse=bool(reverse))


def expected(c):
    """the gapped trace of assemble_oracle.gapped_trace before it is printed: trim, then reverse, then pad"""
    t = dict(sig=np.asarray(c["sig"]), bcpos=list(c["bcpos"]), pri=c["pri"], sec=c["sec"], con=c["con"], q=list(c["q"]), tl=c["l"], tr=c["r"])
    nbc = ao.hard_trim(t)
    sig = t["sig"]
    if c["reverse"]:
        sig, nbc = ao.revcomp_trace(sig, nbc)
    p = so.alignment_trace_padding(c["row"], sig, nbc["bcPos"], bytes(nbc["primary"]), bytes(nbc["secondary"]), bytes(nbc["consensus"]),
                                   nbc["estQual"])
    m = len(nbc["bcPos"])
    step = (nbc["bcPos"][-1] - nbc["bcPos"][0]) // (m - 1) if m > 1 else 6
    return dict(signal=np.asarray(p["signal"], np.int64).reshape(4, -1), bcPos=np.asarray(p["bcPos"], np.int64), primary=bytes(p["primary"]),
                secondary=bytes(p["secondary"]), consensus=bytes(p["consensus"]), estQual=np.asarray(p["estQual"], np.int64),
                leadingGaps=p["leadingGaps"], trailingGaps=p["trailingGaps"], step=step)


def compare(got, want, name):
    """got: dict(status, signal [4][ns'], bcPos, primary, secondary, consensus, estQual, leadingGaps, trailingGaps, step)"""
    assert got["status"] == OK, name
    assert np.asarray(got["signal"]).shape == want["signal"].shape, (name, np.asarray(got["signal"]).shape, want["signal"].shape)
    assert (np.asarray(got["signal"], np.int64) == want["signal"]).all(), name
    assert len(got["bcPos"]) == len(want["bcPos"]) and (np.asarray(got["bcPos"], np.int64) == want["bcPos"]).all(), (name, got["bcPos"], want["bcPos"])
    for f in ("primary", "secondary", "consensus"):
        assert bytes(got[f]) == want[f], (name, f, bytes(got[f]), want[f])
    assert (np.asarray(got["estQual"], np.int64) == want["estQual"]).all(), name
    for f in ("leadingGaps", "trailingGaps", "step"):
        assert int(got[f]) == int(want[f]), (name, f, got[f], want[f])


def _spaced(n, spacing=12, start=4):
    return [start + spacing * i for i in range(n)]


def _row(letters, gaps):
    """letters letters; gaps: {letter index p: run before letter p} (p == letters: behind the last letter)"""
    out = bytearray()
    for p in range(letters):
        out += b"-" * gaps.get(p, 0) + b"ACGT"[p % 4:p % 4 + 1]
    return bytes(out + b"-" * gaps.get(letters, 0))


def crafted(insert_tile=256, sample_tile=256):
    """(name, case): answerable, status OK"""
    cs = []
    add = lambda name, *a, **k: cs.append((name, make(*a, seed=len(cs), **k)))
    add("adjacent", [5, 6], b"A--C", ns=9)               # bcPos' [5, 6, 7, 8], primary' "--AC"
    add("apart", [5, 8], b"A--C", ns=11)                 # bcPos' [5, 7, 10, 14], primary' "A--C"
    add("lead_trail", [5, 9], b"--A-C--", ns=20)         # leading and trailing 2, ns' 24
    add("one_call", [7], b"-A--", ns=12)                 # step 6, no insert
    add("one_call_bare", [0], b"A", ns=1)
    add("two_calls", [2, 9], b"G---T")
    add("mean_not_integer", [3, 7, 12, 20], b"A-CG--T")  # 17 / 3
    add("no_gaps", _spaced(10), _row(10, {}))
    add("all_gaps_row", _spaced(3), b"----")
    add("empty_row", _spaced(3), b"")
    for cols in (63, 64, 65, 128):
        add("cols_%d" % cols, _spaced(cols - 4, 7), _row(cols - 4, {0: 1, 9: 2, cols - 4: 1}))
    add("run_straddles_63_64", _spaced(100, 5), _row(100, {62: 4}))         # letters 0 .. 61 in columns 0 .. 61, gaps 62 .. 65
    add("run_ends_at_63", _spaced(100, 5), _row(100, {62: 2}))              # gaps 62, 63; the letter opens the next step
    add("run_fills_a_step", _spaced(40, 9), _row(40, {10: 150, 20: 64}))    # runs longer than a step of columns
    add("leading_run_over_a_step", _spaced(8), _row(8, {0: 70, 3: 1, 8: 130}))
    st = sample_tile
    add("insert_ends_sample_tile", [10, st - 2, st + 1, st + 40], b"AC-GT")   # q = st - 1
    add("insert_opens_sample_tile", [10, st - 1, st + 2, st + 40], b"AC-GT")  # q = st
    add("inserts_across_sample_tiles", _spaced(120, 11), _row(120, {p: 1 + p % 3 for p in range(1, 120, 2)}))
    ni = insert_tile + 44
    add("more_inserts_than_a_tile", _spaced(2 * ni + 1, 3), _row(2 * ni + 1, {p: 1 for p in range(1, 2 * ni + 1, 2)}))
    add("every_letter_gapped_adjacent", list(range(2, 2 + 90)), _row(90, {p: 1 + p % 2 for p in range(0, 91)}))  # spacing 1: q == b[p - 1]
    add("last_possible_insert", [3, 18, 19], b"AC-G", ns=20)                  # q = ns - 2: (b[p-1] + b[p]) >> 1 cannot reach ns - 1
    add("trims_zero", _spaced(12), _row(12, {3: 2}), l=0, r=0)
    add("trims_leave_one", _spaced(12), b"-A-", l=4, r=7)
    add("trims_asymmetric", _spaced(30), _row(22, {0: 3, 5: 1, 17: 2, 22: 4}), l=1, r=7)
    add("reverse", _spaced(25, 10), _row(25, {4: 2, 20: 1}), reverse=True)
    add("reverse_trims", _spaced(25, 10), _row(19, {1: 1, 18: 3}), l=2, r=4, reverse=True)
    tab = COMPLEMENT_FROM + b"Xa"  # every byte of the complement table and two outside it
    add("reverse_table", _spaced(len(tab), 6), _row(len(tab), {7: 1}), reverse=True, letters=tab)
    add("row_shorter_than_calls", _spaced(20), _row(12, {2: 2, 11: 1}))
    add("row_shorter_reverse", _spaced(20), _row(9, {0: 1, 8: 2}), l=3, r=1, reverse=True)
    return cs


def deferred():
    """(name, case): outside the answered domain, one case each"""
    cs = []
    add = lambda name, *a, **k: cs.append((name, make(*a, seed=100 + len(cs), **k)))
    add("equal_neighbours", [4, 9, 9, 15], b"AC-GT", ns=20)
    add("position_at_ns", [4, 9, 20], b"AC-G", ns=20)
    add("negative_position", [-1, 9, 15], b"AC-G", ns=20)
    add("decreasing", [4, 12, 9, 15], b"AC-GT", ns=20)
    add("letters_over_calls", [4, 9, 15], b"AC-GT", ns=20)
    add("letters_over_kept_calls", _spaced(10), _row(8, {2: 1}), l=2, r=1)
    add("trims_take_all", _spaced(10), b"A", l=4, r=6)
    add("right_trim_over_n", _spaced(10), b"A", l=0, r=11)
    add("no_calls", [], b"A-", ns=20)
    add("too_many_calls", list(range(MAX_CALLS + 1)), b"A-C", ns=MAX_CALLS + 2)
    return cs


def random_small(seed):
    """one answerable trace: 1 .. 40 calls, spacings 1 .. 3, ns <= 200, gap runs of 1 .. 3 with probability 0.3 per letter"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 41))
    pos = [int(rng.integers(0, 6))]
    for _ in range(n - 1):
        pos.append(pos[-1] + int(rng.integers(1, 4)))
    l = r = 0
    if rng.random() < 0.4 and n > 1:
        l = int(rng.integers(0, n))
        r = int(rng.integers(0, n - l))
    m = n - l - r
    letters = m if rng.random() < 0.7 else int(rng.integers(1, m + 1))
    gaps = {p: int(rng.integers(1, 4)) for p in range(letters + 1) if rng.random() < 0.3}
    c = make(pos, _row(letters, gaps), ns=pos[-1] + 1 + int(rng.integers(0, 80)), l=l, r=r, reverse=rng.random() < 0.4, seed=seed)
    assert c["sig"].shape[1] <= 200
    return c


def mixed_batch():
    """deferred and answered traces interleaved (the oversized one left out: a batch stays small)"""
    a, d = crafted(), [x for x in deferred() if x[0] != "too_many_calls"]
    out = []
    for i in range(max(len(a), len(d))):
        if i < len(d):
            out.append(d[i] + (False,))
        if i < len(a):
            out.append(a[i] + (True,))
    return out
