"""The inputs of the de novo batch tests (tests/denovo_cases.py) hold every case they are named for -- asserted on the oracle's own
results, so that the GPU test cannot pass on easy inputs.  No GPU."""
import numpy as np

import denovo_cases as dc
import msa_oracle as mo
from test_gpu_assemble_batch import passes, strip_height


def kind(want, name):
    return want[dc.KINDS.index(name)]


def group(name):
    return dc.groups()[dc.KINDS.index(name)]


def internal(tree, v):
    return v >= tree["num"]


def node_rows(tree, v):
    return mo.palign(tree["sps"], tree["p"], v, dc.SCORE)[0]


def test_shapes():
    assert [len(g) for g in dc.groups()] == [5, 7, 4, 4, 2, 3, 2 + 1, 2, 3, 5, 3, 0, 1, 2]
    assert [p.shape[1] for p in group("short")] == [40, 40, 26]
    assert {p.shape[1] for p in group("tiled5")} == {180} and {p.shape[1] for p in group("tiled7")} == {200}
    assert all(200 <= p.shape[1] <= 260 for p in group("longleft"))
    n = group("ncols")
    assert n[1][4, 3::9].all() and not n[1][4, 4::9].any() and not n[0][4].any() and not n[2][4].any()


def test_the_inputs_hold_every_case_at_one_half():
    want = dc.oracle(0.5)
    w = kind(want, "tiled5")
    assert w["forward"] == [1, 0, 1, 1, 0] and w["nrows"] == 5                      # the strand stage flips exactly the two reversed reads
    w = kind(want, "tiled7")
    t = w["tree"]
    assert w["nrows"] == 7 and any(internal(t, t["p"][v][1]) and internal(t, t["p"][v][2]) for v in range(t["num"], t["root"]))
    w = kind(want, "pairs4")
    t = w["tree"]
    left, right = t["p"][t["root"]][1], t["p"][t["root"]][2]
    assert internal(t, left) and internal(t, right) and len(node_rows(t, left)) == 2 and len(node_rows(t, right)) == 2
    w = kind(want, "stranger")
    assert w["partner"][1] == dc.NONE and w["tries"][1] == 3 and w["rounds"] == 3 and w["nrows"] == 3 and w["row"][1] == dc.NONE
    w = kind(want, "lonely")
    assert w["nrows"] == 0 and w["partner"] == [dc.NONE] * 2 and w["rows"] == []
    w = kind(want, "dup")
    t = w["tree"]
    assert w["nrows"] == 3 and t["dist"][0][1] == t["dist"][0][2] == t["dist"][1][2] and t["p"][3][1:] == [0, 1]  # equal distances: the first pair
    T = dc.strand_table(group("dup"))
    assert T[0, 1, 0, 1] == T[0, 2, 0, 1]                                              # ... and equal sums in the flip test
    w = kind(want, "short")
    assert w["partner"] == [dc.NONE, 2, 1] and w["nrows"] == 2 and w["tries"] == [2, 2, 2]
    import pyoracle as orc
    na = [orc.gotoh_prof(w["profs"][i], w["profs"][j], 1, 1, dc.SCORE)[1].count(b"s") for i, j in ((0, 1), (1, 2))]
    assert na == [20, 26]                                                              # numAligned > 25 decides
    assert kind(want, "cross64")["ncol"] > 64 and kind(want, "cross64")["nrows"] == 2
    assert kind(want, "cross256")["ncol"] > 256 and kind(want, "cross256")["nrows"] == 3 and kind(want, "cross256")["forward"] == [1, 0, 1]
    w = kind(want, "longleft")
    t = w["tree"]
    left = t["p"][t["root"]][1]
    cols = len(node_rows(t, left)[0])
    assert w["nrows"] == 5 and internal(t, left) and cols > 512                        # a1 of the root's DP is a node profile ...
    assert passes(cols) > 1 and strip_height(cols) * 64 < cols                         # ... swept in several strip passes
    w = kind(want, "ncols")
    t = w["tree"]
    below = [v for v in range(t["num"], t["root"])]
    assert w["nrows"] == 3 and any(b"N" in r.encode() for v in below for r in node_rows(t, v))  # 'N' rows in a node profile
    assert kind(want, "empty")["nrows"] == 0 and kind(want, "one")["nrows"] == 0 and kind(want, "one")["forward"] == [0]
    assert kind(want, "long2")["nrows"] == 2
    # more than one round and more than one height somewhere; rows in another order than the input somewhere
    assert max(w["rounds"] for w in want) == 5 and max(w["heights"] for w in want) == 3
    assert any(w["nrows"] and [r for r in w["row"] if r != dc.NONE] != sorted(r for r in w["row"] if r != dc.NONE) for w in want)


def test_the_score_term_decides_at_three_quarters():
    want = dc.oracle(0.75)
    for name in ("tiled5", "tiled7"):
        w = kind(want, name)
        first = [0 if i else 1 for i in range(len(w["partner"]))]
        assert any(p != dc.NONE and p != f for p, f in zip(w["partner"], first)), name   # a partner that is not the first candidate
        assert dc.NONE in w["partner"] and w["nrows"] >= 2, name                          # a tiled trace is excluded
    assert any(a["nrows"] != b["nrows"] for a, b in zip(want, dc.oracle(0.5)))


def test_the_table_restatement_is_the_oracle():
    """strands_from_table (what the planning header is compared with) gives msa_oracle.rev_seq_based_on_dist's flags on every group"""
    for name, g, w in zip(dc.KINDS, dc.groups(), dc.oracle(0.5)):
        rev, _ = dc.strands_from_table(dc.strand_table(g))
        assert [1 - r for r in rev] == w["forward"], name


def test_the_wide_groups():
    groups, want = dc.wide()
    assert [w["nrows"] for w in want] == [5, 3, 2]
    assert all(np.float32(3.5) < p.sum(0).max() <= np.float32(4.001) for g in groups for p in g)
