"""The inputs of the wildtype edge tests (tests/wildtype_cases.py) hold every case they are named for -- asserted on the inputs and on
the oracle's own results, so that tests/test_gpu_wildtype_edges.py cannot pass on easy inputs.  No GPU.  The strip-height rule of
capi.hip is restated in tests/test_gpu_consensus_batch.py: 4 rows per lane up to 256 rows, 8 up to 512, 4 again (three passes) up to
768, 8 (two passes) from 769 on."""
import numpy as np

import pyoracle as orc
import wildtype_cases as wc
import wildtype_oracle as wo
from test_gpu_consensus_batch import arith16_holds, passes, strip_height


def heights(b):
    """(mf, mt, n) of every pair of an align batch, createProfile's clamp applied"""
    tl, tr = np.broadcast_to(b["tl"], len(b["traces"])), np.broadcast_to(b["tr"], len(b["traces"]))
    out = []
    for t, l, r, w in zip(b["traces"], tl, tr, b["ridx"]):
        mf = t.shape[1]
        out.append((mf, wo.trimmed_view(t, l, r).shape[1], b["wild"][int(w)].shape[1]))
    return out


def test_every_16_bit_launch_stays_in_range():
    """profiles are normalised (Q = 5): every pair but the long wildtypes of A2 must hold the 16-bit arithmetic"""
    for b in (wc.a1(), wc.a3(), wc.a4(), wc.a5()):
        assert all(arith16_holds(mt + n, 5) for _, mt, n in heights(b))
        assert all(np.allclose(p[:, j].sum(), 1.0, atol=1e-5) for p in b["traces"] + b["wild"] for j in (0, p.shape[1] // 2, p.shape[1] - 1))
    assert all(arith16_holds(mt + n, 5) for _, mt, n in heights(wc.a2()) if n < 1500)
    d = wc.d1()
    for t, l, r, w in zip(d["traces"], d["tl"], d["tr"], d["ridx"]):
        assert arith16_holds(len(t["pri"]) - int(l) - int(r) + d["wild"][int(w)]["prof"].shape[1], 5)


def test_a1_wildtype_rows_4_and_5_bear_on_the_reverse_alignment():
    b, plain = wc.a1(), wc.a1_plain_rows()
    hs = heights(b)
    assert [h[0] for h in hs] == [300, 300, 612, 612, 869, 869] and list(b["ridx"]) == [0, 0, 1, 1, 2, 2]
    assert [(strip_height(mt), passes(mt)) for _, mt, _ in hs[::2]] == [(4, 1), (8, 1), (8, 2)]   # the scores: trimmed heights 200, 512, 769
    assert [(strip_height(mf), passes(mf)) for mf, _, _ in hs[::2]] == [(8, 1), (4, 3), (8, 2)]   # the traceback: full heights
    assert all(abs(mf - n) <= mf // 8 for mf, _, n in hs)
    for w in range(3):
        p = b["wild"][w]
        assert p[4].any() and p[5].any()
        assert np.array_equal(wc.revcomp(p)[4:], p[4:, ::-1])                   # what the reverse copy must hold in rows 4 and 5
        assert not np.array_equal(p[4], p[4, ::-1]) and not np.array_equal(p[5], p[5, ::-1])  # ... and a forward row would not pass for it
        assert [b["want"][2 * w]["forward"], b["want"][2 * w + 1]["forward"]] == [1, 0]
        # the rows decide the path of the reverse trace, not only its score: with rows 4 and 5 zeroed the oracle walks another way
        assert b["want"][2 * w + 1]["btr"] != plain[2 * w + 1]["btr"]
        assert plain[2 * w + 1]["forward"] == 0


def test_a2_wildtype_lengths():
    b = wc.a2()
    hs = heights(b)
    assert [(mf, n) for mf, _, n in hs[::2]] == [(140, 1), (140, 2), (140, 63), (140, 64), (140, 65), (140, 127), (140, 129),
                                                 (300, 1500), (869, 64), (869, 1500)]
    assert hs[::2] == hs[1::2] and all(mt == mf - 100 for mf, mt, _ in hs)
    for n in sorted({n for _, _, n in hs if n >= 63}):
        assert {w["forward"] for w, h in zip(b["want"], hs) if h[2] == n} == {0, 1}, n
    assert passes(769) > 1 and passes(40) == passes(200) == 1  # 869 columns: the n + 2 boundary rows per strand, for n = 64 and n = 1500
    assert not any(p[4].any() for p in b["traces"] + b["wild"])


def test_a3_trimmed_heights():
    b = wc.a3()
    hs = heights(b)
    tl, tr = b["tl"].astype(np.int64), b["tr"].astype(np.int64)
    assert (tl != tr).all()
    mf = np.array([h[0] for h in hs])
    free = tl + tr < mf
    assert sorted(h[1] for h, f in zip(hs, free) if f) == [1, 2, 63, 64, 65, 255, 256, 257, 512, 513, 768, 769]
    assert sorted(mf[free].tolist()) == [140] * 5 + [356] * 3 + [869] * 4
    assert sorted((tl + tr - mf)[~free].tolist()) == [0, 7] and [h[1] for h, f in zip(hs, free) if not f] == [140, 356]  # clamped to 0 / 0
    assert {(strip_height(h[1]), passes(h[1]) > 1) for h in hs} == {(4, False), (4, True), (8, False), (8, True)}
    assert all(abs(h[0] - h[2]) <= h[0] // 8 for h in hs) and list(b["ridx"]) == list(range(len(hs)))
    one = [i for i, h in enumerate(hs) if h[1] == 1]
    assert len(one) == 1
    i = one[0]
    col = np.ascontiguousarray(b["traces"][i][:, int(tl[i]):int(tl[i]) + 1])
    assert int(tl[i]) + 1 + int(tr[i]) == hs[i][0]
    assert b["want"][i]["score_fwd"] == orc.gotoh_score_prof(col, b["wild"][i], 1, 0, wc.SCORE)
    fwd = [w["forward"] for h, w in zip(hs, b["want"]) if h[1] >= 63]
    assert fwd == [(k + 1) % 2 for k in range(len(fwd))] or fwd == [k % 2 for k in range(len(fwd))]  # the strands alternate


def test_a4_more_traces_than_one_block_of_the_decision_kernel():
    b = wc.a4()
    hs = heights(b)
    assert len(hs) == 300 > 256 and {h[:2] for h in hs} == {(120, 20)}
    assert sorted({h[2] for h in hs}) == list(wc.A4_WILD) and len(b["wild"]) == 7 and min(wc.A4_WILD) == 24 and max(wc.A4_WILD) == 40
    fwd = np.array([w["forward"] for w in b["want"]])
    assert 100 <= fwd.sum() <= 200 and {int(f) for f in fwd[256:]} == {0, 1}      # both strands behind the first 256 traces as well
    assert all(np.bincount(b["ridx"], minlength=7) >= 42)


def test_a5_layout():
    b = wc.a5()
    assert list(b["ridx"]) == [2, 0, 1, 0, 2, 1] and len(b["wild"]) == 4 and 3 not in b["ridx"]
    data, off = wc.a5_layout(b["wild"])
    assert list(np.argsort(off)) == [3, 2, 1, 0]                                  # index 0 lies last in memory
    ends = {int(off[i]) + b["wild"][i].size for i in range(4)}
    assert [int(off[2]) - (int(off[3]) + b["wild"][3].size), int(off[1]) - (int(off[2]) + b["wild"][2].size),
            int(off[0]) - (int(off[1]) + b["wild"][1].size)] == list(wc.A5_PADDING)
    assert data.size == max(ends) and (data == wc.A5_SENTINEL).sum() == sum(wc.A5_PADDING)
    for i in range(4):
        assert np.array_equal(data[int(off[i]):int(off[i]) + b["wild"][i].size].reshape(6, -1), b["wild"][i])
    assert {w["forward"] for w in b["want"]} == {0, 1}
    assert b["wild"][3][4].any() and b["wild"][3][5].any()


def test_d1_strip_heights():
    d = wc.d1()
    mf = np.array([len(t["pri"]) for t in d["traces"]])
    mt = mf - d["tl"] - d["tr"]
    assert sorted(set(mt.tolist())) == [200, 256, 257, 520, 780] and (d["tl"] + d["tr"] < mf).all()
    assert {(strip_height(m), passes(m)) for m in mt.tolist()} == {(4, 1), (8, 1), (4, 3), (8, 2)}
    assert [(strip_height(m), passes(m)) for m in (200, 256, 257, 520, 780)] == [(4, 1), (4, 1), (8, 1), (4, 3), (8, 2)]
    assert len(set(zip(d["tl"].tolist(), d["tr"].tolist()))) >= 3                                    # per-trace trims
    for m in (200, 256, 257, 520, 780):                                                              # a forward and a reverse wildtype per height
        assert {d["wild"][int(w)]["reverse"] for w, x in zip(d["ridx"], mt) if x == m} == {False, True}, m
    fwd = [w["forward"] for w in d["want"]]
    assert fwd == [int(not d["wild"][int(w)]["reverse"]) for w in d["ridx"]]
    assert {f for f, m in zip(fwd, mt) if passes(int(m)) > 1} == {0, 1}
    assert sorted(np.bincount(d["ridx"]).tolist())[-1] == 2                                          # two traces share a wildtype
    assert sum(c[3] == 0 for c in wc.D1_CASES) >= 3 and {c[3] for c in wc.D1_CASES} == {0, 3}
    assert sum(w["status"] == 0 and w["bp"].indelshift != 0 for w in d["want"]) >= 3
    assert all(w["prof"].shape[1] == len(w["primary"]) for w in d["wild"])


def test_d3_tie():
    d = wc.d3()
    w = d["wild"][0]["prof"]
    assert w.shape == (6, 700) and np.array_equal(wc.revcomp(w).view(np.uint32), w.view(np.uint32))  # bit-equal to its reverse complement
    for s, full in zip(d["strand"], d["want"]):
        assert s["score_fwd"] == s["score_rev"] and s["forward"] == 0
        assert all(full[k] == s[k] for k in s)


def test_d4_n_row_and_a_stranger():
    d, base = wc.d4(), wc.d1()
    w = d["wild"][wc.D4_N_WILD]["prof"]
    assert w[4].any() and not base["wild"][wc.D4_N_WILD]["prof"][4].any()
    twins = [(d["want"][k], base["want"][i]) for k, i in enumerate(d["keep"][:-1])]
    assert len(twins) == 2
    keys = ("status", "score_fwd", "score_rev", "forward", "score_trim", "primary", "secondary", "dcp", "btr0", "btr1", "btr2")
    assert any(a[k] != b[k] for a, b in twins for k in keys)                                         # the N row changes what the oracle answers
    t, other = wc.D4_STRANGER
    assert int(d["ridx"][-1]) == other != int(base["ridx"][t]) and d["wild"][other]["ref"] != base["wild"][int(base["ridx"][t])]["ref"]
    assert d["want"][-1]["score_trim"] < 0 < base["want"][t]["score_trim"]
