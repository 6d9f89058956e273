"""The inputs of the consensus fix-up tests (tests/consensus_fixup_cases.py) hold every case they are named for -- asserted on the
oracle's own results and on the host build of consensus.h (tests/cpp/consensus_column.cpp), so that the GPU test cannot pass on easy
inputs and so that every expected fix-up count is the same whatever the device's log10 does in its last 4 ulp.  No GPU."""
import numpy as np
import pytest

import consensus_fixup_cases as fc
from test_consensus_host import cc, host_gt, screen  # noqa: F401  (cc: the g++ build of the column body, a fixture)
from test_gpu_consensus_batch import arith16_holds

VARIANTS = [(True, False), (True, True), (False, False), (False, True)]  # (union, iupac)


def test_families(cc):
    """per-family flag membership, with and without IUPAC, stable under 0, 1 and 4 ulp"""
    assert [len(fc.FAMILIES[k]) for k in ("half", "not_half", "tenth", "negative")] == [120, 80, 8, 3]
    for name in fc.FAMILIES:
        cl = fc.family_columns(name)
        assert cl.dtype == np.float32
        for iupac in (False, True):
            flag = fc.stable_flags(cc, cl, iupac)
            assert flag.all() if name in fc.FLAGGED[iupac] else not flag.any(), (name, iupac)
    # half: -10 (gl2 - gl1) of a double log10 lies within the screen (2^-20) of p + 0.5, its float neighbours too; not-half: 64 steps away
    for entries, near in ((fc.HALF, True), (fc.NOT_HALF, False)):
        for one, r in entries:
            x = -10 * np.log10(np.float64(r) / np.float64(one))
            assert (abs(x - np.floor(x) - 0.5) < 2.0 ** -20) == near, (r, x)
    # tenth: a / (9 a + a) is the double 0.1 and gl[second] is -1 on the host
    for big, a in fc.TENTH:
        assert np.float64(a) / (np.float64(big) + np.float64(a)) == 0.1 and np.log10(0.1) == -1.0
    # negative: the device body alone gives another quality than gtLetter (secondPL 10001 is outside the gq table), so a fix-up that is
    # lost, or patched into the wrong slot, shows in the result
    cl = fc.family_columns("negative")
    for iupac in (False, True):
        _, q, _ = screen(cc, cl, iupac)
        _, hq = host_gt(cc, cl, iupac)
        assert (q.astype(np.uint32) != hq).all() and (hq == 10000).all()


def lanes_of(e, i, which=None):
    """alignment column mod 64 of the flagged emitted columns of pair i"""
    cols, flags = e["cols"][i], e["flags"][i]
    return {c % 64 for c, f, s in zip(cols[1], flags, cols[3]) if f and (which is None or s == which)}


@pytest.mark.parametrize("union,iupac", VARIANTS)
def test_mix_holds_every_case(cc, union, iupac):
    pairs = fc.mix()
    e = fc.expectation(cc, pairs, union, iupac, key="mix")
    want = e["want"]
    assert len(pairs) == 13
    # status, strands, the diagonal
    nothing = (fc.SHORT_PAIR, fc.MISMATCH_PAIR)
    assert [w["status"] for w in want] == [1 if i in nothing else 0 for i in range(13)]
    assert [w["forward"] for i, w in enumerate(want) if i not in nothing] == [0 if p["reverse"] else 1 for i, p in enumerate(pairs) if i not in nothing]
    assert {w["forward"] for w in want} == {0, 1}
    for i, (p, w) in enumerate(zip(pairs, want)):
        if i in nothing or i == fc.GAP_PAIR:
            continue
        m, n = p["first"].shape[1], p["crafted"].shape[1]
        assert w["rows"][0].count(b"-") == p["trail"] and w["rows"][1].count(b"-") == p["lead"], i
        assert w["rows"][1][:p["lead"]] == b"-" * p["lead"] and w["rows"][0][m:] == b"-" * p["trail"], i  # the overhangs, nothing else
        assert len(w["rows"][0]) == p["lead"] + n and w["num_aligned"] == m - p["lead"] == w["num_match"], i
    assert [len(w["rows"][0]) for w in want[:5]] == list(fc.ROUND_LENGTHS)
    # every emitted column is the crafted one or a clean one, is flagged iff its family is a flagged one, and its flag is stable
    for i, (cols, flags) in enumerate(zip(e["cols"], e["flags"])):
        assert "broken" not in cols[2], i
        assert [f in fc.FLAGGED[iupac] for f in cols[2]] == flags.tolist(), i
        if len(cols[0]):
            assert np.array_equal(fc.stable_flags(cc, cols[0], iupac), flags), i
    fams = [f for cols in e["cols"] for f in cols[2]]
    assert {f for f in fams if f} == set(fc.FAMILIES)
    assert e["count"] == sum(f in fc.FLAGGED[iupac] for f in fams) > 0
    # the all-families pair: 600 columns, every entry once
    assert e["cols"][fc.ALL_PAIR][2].count("half") == 120 and e["cols"][fc.ALL_PAIR][2].count("not_half") == 80
    assert want[fc.ALL_PAIR]["rows"][0] == want[fc.ALL_PAIR]["rows"][1] and len(want[fc.ALL_PAIR]["rows"][0]) == 600
    # flagged columns at lanes 0 and 63 of a round, in the first round and in a later one, and in the last (partial) round
    for i in range(5):
        assert {0, 63} & lanes_of(e, i) == ({0} if fc.ROUND_LENGTHS[i] == 63 else {0, 63}), i
        assert e["flags"][i][0] and e["flags"][i][-1], i                      # the first and the last column of the pair
    assert any(f and c >= 64 and c % 64 == 0 for c, f in zip(e["cols"][4][1], e["flags"][4]))
    assert any(f and c == 127 for c, f in zip(e["cols"][4][1], e["flags"][4]))
    # a flagged column directly after a gap column, an aligned flagged column directly before it
    g = pairs[fc.GAP_PAIR]
    w = want[fc.GAP_PAIR]
    d = g["delete"]
    assert w["rows"][1].count(b"-") == 1 and w["rows"][1][d] == ord("-") and b"-" not in w["rows"][0]
    cols = e["cols"][fc.GAP_PAIR]
    at = {(c, s): (f, fl) for c, s, f, fl in zip(cols[1], cols[3], cols[2], e["flags"][fc.GAP_PAIR])}
    assert at[(d + 1, "aligned")] == ("negative", True)
    assert at[(d - 1, "aligned")] == ("tenth", iupac)
    assert ((d, "first") in at) == union
    # the pairs that emit nothing are made of flagged-family columns only: one fails by min_overlap, one by the match fraction
    for i in nothing:
        assert all(f in ("half", "negative") for f in pairs[i]["fam1"] + pairs[i]["fam2"]) and want[i]["cons"] == b"" and e["per_pair"][i] == 0
    assert want[fc.SHORT_PAIR]["num_aligned"] == 20 < 25
    u = want[fc.MISMATCH_PAIR]
    assert u["num_aligned"] >= 250 and 0.3 < u["num_match"] / u["num_aligned"] < 0.5
    assert e["per_pair"][fc.CLEAN_PAIR] == 0 and e["per_pair"][fc.LONG_PAIR] > 0


def test_mix_counts_differ_as_stated(cc):
    e = {v: fc.expectation(cc, fc.mix(), v[0], v[1], key="mix") for v in VARIANTS}
    fam = lambda v, name: sum(f == name for c in e[v]["cols"] for f in c[2])
    # IUPAC adds exactly the tenth columns
    for union in (True, False):
        tenth = fam((union, True), "tenth")
        assert tenth > 0 and e[(union, True)]["count"] - e[(union, False)]["count"] == tenth
    # the intersection drops exactly the flagged overhang columns; only the overhang pairs hold any
    for iupac in (False, True):
        over = sum(f and s != "aligned" for c, fl in zip(e[(True, iupac)]["cols"], e[(True, iupac)]["flags"]) for f, s in zip(fl, c[3]))
        assert over >= 40 and e[(True, iupac)]["count"] - e[(False, iupac)]["count"] == over
        assert all(s == "aligned" for c in e[(False, iupac)]["cols"] for s in c[3])
        diff = [a - b for a, b in zip(e[(True, iupac)]["per_pair"], e[(False, iupac)]["per_pair"])]
        assert [i for i, x in enumerate(diff) if x] == list(fc.OVER_PAIRS)
    # flagged overhang columns on both sides, at lanes 0 and 63 of a round
    ev = e[(True, False)]
    for i in fc.OVER_PAIRS:
        assert lanes_of(ev, i, "first") and lanes_of(ev, i, "second"), i
    assert {0, 63} <= lanes_of(ev, fc.OVER_PAIRS[1], "first") and {0, 63} & lanes_of(ev, fc.OVER_PAIRS[1], "second")


def test_mix_runs_in_chunks_under_the_limit():
    """consensus_run's planning restated: a chunk closes when the next pair's planes no longer fit, so cons_chunks > 1 iff the pairs
    together need more than the limit (and every single pair fits)"""
    need = [fc.pair_need(p["first"].shape[1], p["second"].shape[1]) for p in fc.mix()]
    assert max(need) <= fc.MIX_LIMIT < sum(need)
    chunks, held = 1, 0
    for x in need:  # (the library orders pairs by strip height first; in any order a sum beyond the limit closes a chunk)
        if held and held + x > fc.MIX_LIMIT:
            chunks, held = chunks + 1, 0
        held += x
    assert chunks > 1


def test_mix_scaled_repeats_on_int32_with_the_same_flags(cc):
    """every profile x 4.0: exact, every cl / total unchanged, so the same columns are flagged; the 16-bit score launches are refused
    at the end of the first run (test_gpu_consensus_batch.test_runs_repeat_on_int32)"""
    pairs = fc.mix()
    plain = fc.expectation(cc, pairs, True, True, key="mix")
    wide = fc.expectation(cc, pairs, True, True, scale=fc.WIDE, key="mix")
    assert wide["per_pair"] == plain["per_pair"] and wide["count"] == plain["count"] > 0
    for a, b, fa, fb in zip(plain["cols"], wide["cols"], plain["flags"], wide["flags"]):
        assert np.array_equal(a[0] * np.float32(fc.WIDE), b[0]) and a[1:] == b[1:] and np.array_equal(fa, fb)
        if len(b[0]):
            assert np.array_equal(fc.stable_flags(cc, b[0], True), fb)
    assert [w["status"] for w in plain["want"]] == [w["status"] for w in wide["want"]]
    ok = [i for i, w in enumerate(plain["want"]) if w["status"] == 0]  # (the scores of a pair without overlap round differently x 16)
    assert [plain["want"][i]["rows"] for i in ok] == [wide["want"][i]["rows"] for i in ok]
    assert [w["cons"] for w in plain["want"]] == [w["cons"] for w in wide["want"]] and [w["qual"] for w in plain["want"]] == [w["qual"] for w in wide["want"]]
    mn = [p["first"].shape[1] + p["second"].shape[1] for p in pairs]
    q_plain = fc.largest_sub(fc.firsts(pairs), fc.seconds(pairs))
    q_wide = fc.largest_sub(fc.scaled(fc.firsts(pairs)), fc.scaled(fc.seconds(pairs)))
    assert all(arith16_holds(x, 5) for x in mn)                    # a priori every score launch is a 16-bit one
    assert all(arith16_holds(x, q_plain) for x in mn)              # ... and stays one with the masses of the crafted columns
    assert max(mn) >= 730 and q_wide >= 82 and not arith16_holds(730, 82) and not arith16_holds(max(mn), q_wide)
    assert (max(mn) + 2) * (14 + q_wide) + 1000000 < 1 << 26       # the int32 kernels hold the values


def test_clean_batch_flags_nothing(cc):
    for union, iupac in VARIANTS[:2]:
        e = fc.expectation(cc, fc.clean_batch(), union, iupac, key="clean")
        assert e["count"] == 0 and all(w["status"] == 0 for w in e["want"]) and {w["forward"] for w in e["want"]} == {0, 1}
        for cols in e["cols"]:
            assert not fc.stable_flags(cc, cols[0], iupac).any()


def test_overflow_pair_flags_every_column(cc):
    p = fc.overflow_pair()
    e = fc.expectation(cc, [p], True, True, key="overflow")
    w = e["want"][0]
    assert w["status"] == 0 and w["rows"][0] == w["rows"][1] and len(w["rows"][0]) == fc.OVERFLOW_LEN and b"-" not in w["rows"][0]
    assert set(e["cols"][0][2]) == {"negative", "tenth"} and e["cols"][0][3] == ["aligned"] * fc.OVERFLOW_LEN
    assert fc.stable_flags(cc, e["cols"][0][0], True).all() and e["count"] == fc.OVERFLOW_LEN
    assert fc.OVERFLOW_COUNT == fc.OVERFLOW_COPIES * e["count"] == 72000 > fc.FIX_CAP == max(65536, 4 * fc.OVERFLOW_COPIES)
    assert w["qual"].count(10000) > 400  # the negative columns: a result only the host gtLetter gives
    mn = 2 * fc.OVERFLOW_LEN
    assert arith16_holds(mn, fc.largest_sub([p["first"]], [p["second"]]))


@pytest.mark.parametrize("iupac", [False, True])
def test_log10_batch(cc, iupac):
    pairs = fc.log10_batch()
    assert len(pairs) == fc.LOG10_PAIRS and all(p["first"].shape == p["second"].shape == (6, fc.LOG10_LEN) for p in pairs)
    assert fc.LOG10_PAIRS * fc.LOG10_LEN == 32768
    fams = [f for p in pairs for f in p["fam1"]]
    per = len(range(3, fc.LOG10_LEN, fc.LOG10_EVERY))
    assert per == 64 and all([f is not None for f in p["fam1"]] == [j % 8 == 3 for j in range(fc.LOG10_LEN)] for p in pairs)
    n_all = len(fc.LOG10_ENTRIES)
    assert n_all == 211 and all(fams.count(k) >= (per * fc.LOG10_PAIRS // n_all) * len(v) for k, v in fc.FAMILIES.items())  # every entry, many times
    count = 0
    for i, p in enumerate(pairs):
        cl = fc.diagonal_columns(p)
        flag = fc.stable_flags(cc, cl, iupac)
        assert [f in fc.FLAGGED[iupac] for f in p["fam1"]] == flag.tolist(), i
        count += int(flag.sum())
    assert count == sum(f in fc.FLAGGED[iupac] for f in fams) > 1000
    # the sampled pairs: the oracle aligns them on the diagonal, and its consensus is gtLetter of the float32 column sums
    sample = [pairs[i] for i in fc.LOG10_SAMPLE]
    e = fc.expectation(cc, sample, True, iupac, key="log10_sample")
    for p, w, cols in zip(sample, e["want"], e["cols"]):
        assert w["status"] == 0 and len(w["rows"][0]) == fc.LOG10_LEN and b"-" not in w["rows"][0] + w["rows"][1]
        assert np.array_equal(cols[0], fc.diagonal_columns(p))
        letter, qual = host_gt(cc, cols[0], iupac)
        assert letter.tobytes() == w["cons"] and qual.tolist() == w["qual"]
