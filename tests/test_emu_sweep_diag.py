"""The 16-bit query-profile sweeps in their offset form (dp_kernels.h gotoh_narrow_qp_body / gotoh_prefix_body, DIAG: every value
carries (row + column) |ge| minus a running base, six operations per cell) on the 64-lane host emulator: scores against the oracle,
and everything the sweeps leave in memory -- row m, the wavefront checkpoints, the kept prefix row, the reported bound -- against
the form on values as they are, bit for bit.

Checkpoint records are compared in the lanes that hold rows of the pair.  A lane beyond the last row holds no DP value: it runs
the steady-state steps unguarded on whatever its registers held, in either form, nothing reads it, and the two forms' leftovers
there are not images of each other."""
import os
import sys

import numpy as np
import pytest

import pyoracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu_sweep_diag as sd  # noqa: E402

SC = (3, -5, -10, -4)
MS = [1, 14, 15, 16, 31, 130, 899, 900, 960]   # padding rows, one lane, the last lane full or nearly empty
NS = [1, 3, 4, 5, 63, 64, 65, 200, 700]        # the ramps only, a re-base inside the ramp-down, several re-bases
B = 32


def rand_seq(rng, n, alpha):
    return bytes(rng.choice(list(alpha), size=n).tolist())


def rand_profile(rng, n, sharp):
    p = np.zeros((6, n), dtype=np.float32)
    x = rng.random((4, n)).astype(np.float32)
    if sharp:
        x = x ** 6
    p[:4] = x / x.sum(axis=0, keepdims=True)
    if n > 2:  # weight in row 4 ('N'): the entries of N columns are not a constant of the scoring then
        j = rng.integers(0, n, size=max(1, n // 7))
        p[4, j] = p[0, j]
        p[0, j] = 0
    return p


def revcomp_str(s):
    return bytes(s[::-1]).translate(bytes.maketrans(b"ACGT", b"TGCA"))


_CASES = {}


def case(K, im, jn):
    """one pair per (K, m, n); view, alphabet (so: table form), profile kind and strings rotate over the grid.  The reference
    results -- the oracle's score and the sweep on values as they are -- are computed once."""
    key = (K, im, jn)
    if key not in _CASES:
        m, n = MS[im], NS[jn]
        rng = np.random.default_rng(1000 * K + 10 * im + jn)
        rc = (im + jn) % 2 == 1
        plain = (im + 2 * jn) % 3 != 0            # references over ACGT: the four-code table; over ACGTNn-x: the six-code one
        strings = (2 * im + jn) % 5 == 0          # MODE_CQ
        ref = rand_seq(rng, n, b"ACGT" if plain else b"ACGTNn-x")
        if strings:
            a1 = rand_seq(rng, m, b"ACGTN")
            want = orc.gotoh_score_str(a1, revcomp_str(ref) if rc else ref, 1, 0, SC)
        else:
            a1 = rand_profile(rng, m, sharp=jn % 2 == 0)
            p2 = orc.create_profile_str(ref)
            want = orc.gotoh_score_prof(a1, orc.revcomp_profile(p2) if rc else p2, 1, 0, SC)
        today = sd.sweep(a1, ref, SC, K, 0, ckpt=True, B=B, revcomp=rc)
        assert today[0] == want and today[1] == (0, 0), key
        _CASES[key] = (a1, ref, rc, want, today)
    return _CASES[key]


@pytest.mark.parametrize("period", [64, 128])
@pytest.mark.parametrize("K", [15, 16])
def test_full_sweep_offset_form(K, period):
    for im, m in enumerate(MS):
        for jn, n in enumerate(NS):
            a1, ref, rc, want, today = case(K, im, jn)
            score, err, rowm, rec = sd.sweep(a1, ref, SC, K, period, ckpt=True, B=B, revcomp=rc)
            assert score == want and err == (0, 0), (K, period, m, n)
            assert np.array_equal(rowm[1:n + 1], today[2][1:n + 1]), (K, period, m, n)
            lanes = (m + K - 1) // K
            nrec = (n + lanes - 1) // B
            assert np.array_equal(rec[:nrec, :, :lanes], today[3][:nrec, :, :lanes]), (K, period, m, n)
            assert np.array_equal(rec[nrec:], today[3][nrec:])  # (nothing written behind the last record)
            if (im + jn + period // 64) % 3 == 0:  # the sweep that keeps nothing (tracyhip_gotoh_score): a third of the grid per period
                assert sd.sweep(a1, ref, SC, K, period, ckpt=False, revcomp=rc)[0] == want, (K, period, m, n)


def test_sixteen_row_strips_with_every_lane_full():
    """K = 16 at the heights it is chosen for (961 to 1 024 rows): 61 lanes, one row in the last lane (1 009 = 63 x 16 + 1), all 64
    lanes full -- the grid above runs K = 16 on heights of at most 960 rows, so its last four lanes never hold a row.  References
    longer than the traces too (n = 1 100 > m).  Score, row m and the checkpoints of the lanes that hold rows, at both periods,
    against the form on values as they are and the oracle."""
    K = 16
    for im, m in enumerate((961, 1009, 1024)):
        for jn, n in enumerate((1, 64, 65, 700, 1100)):
            rng = np.random.default_rng(16000 + 10 * im + jn)
            rc = (im + jn) % 2 == 1
            a1 = rand_profile(rng, m, sharp=jn != 3 or im != 1)  # (one flat profile; the others sharp)
            ref = rand_seq(rng, n, b"ACGTNn-x" if (im + jn) % 4 else b"ACGT")
            p2 = orc.create_profile_str(ref)
            want = orc.gotoh_score_prof(a1, orc.revcomp_profile(p2) if rc else p2, 1, 0, SC)
            today = sd.sweep(a1, ref, SC, K, 0, ckpt=True, B=B, revcomp=rc)
            assert today[0] == want and today[1] == (0, 0), (m, n)
            lanes = (m + K - 1) // K
            nrec = (n + lanes - 1) // B
            for period in (64, 128):
                score, err, rowm, rec = sd.sweep(a1, ref, SC, K, period, ckpt=True, B=B, revcomp=rc)
                assert score == want and err == (0, 0), (period, m, n)
                assert np.array_equal(rowm[1:n + 1], today[2][1:n + 1]), (period, m, n)
                assert np.array_equal(rec[:nrec, :, :lanes], today[3][:nrec, :, :lanes]), (period, m, n)
                assert np.array_equal(rec[nrec:], today[3][nrec:]), (period, m, n)
            assert sd.sweep(a1, ref, SC, K, 64 << (jn % 2), ckpt=False, revcomp=rc)[0] == want, (m, n)  # the sweep that keeps nothing


@pytest.mark.parametrize("K,GL", [(8, 16), (8, 8)])
def test_prefix_rows_offset_form(K, GL):
    """four (eight) pairs per wave with references of different lengths, one group without a pair, both views: the reported bound
    and the kept row equal those of the form on values as they are"""
    rng = np.random.default_rng(70 + GL)
    per_wave = 64 // GL
    for npairs in (per_wave, per_wave - 1):
        for lengths in ([700, 5, 64, 65, 200, 3, 130, 63], [90, 90, 300, 1, 257, 4, 66, 128]):
            ns = lengths[:npairs]
            profs = [rand_profile(rng, K * GL + int(rng.integers(1, 60)), sharp=i % 2 == 0) for i in range(npairs)]
            refs = [rand_seq(rng, n, b"ACGT" if i % 2 else b"ACGTNn-x") for i, n in enumerate(ns)]
            rc = [i % 3 == 0 for i in range(npairs)]
            skip = [i == 1 for i in range(npairs)]
            b0, k0, e0 = sd.prefix(profs, refs, SC, K, GL, 0, rc, skip)
            assert e0 == (0, 0)
            for period in (64, 128):
                b1, k1, e1 = sd.prefix(profs, refs, SC, K, GL, period, rc, skip)
                assert e1 == (0, 0) and np.array_equal(b0, b1), (K, GL, npairs, period)
                for i in range(npairs):
                    assert np.array_equal(k0[i][1:], k1[i][1:]), (K, GL, npairs, period, i)
            assert b0[1] == 0x7f7f7f7f and all(b0[i] != 0x7f7f7f7f for i in range(npairs) if i != 1)  # the skipped group wrote nothing


def test_the_edge_of_the_range_rule_on_the_emulator():
    """3/-5/-10/-18 at 960 rows: narrow_ok admits it, and the rule's own period leaves the offsets just enough of int16.  A pair
    built to reach the bounds -- every cell a mismatch (the values fall as far as they can), every cell a match (they rise as far as
    they can) -- gives the oracle's score, the same row m and the same checkpoints at that period."""
    sc = (3, -5, -10, -18)
    K, m, n = 15, 960, 700
    assert sd.narrow_ok(sc, m, K)
    period = sd.diag_period(sc, K)
    assert period == 256  # (4 800 + 18 (898 + 256) = 25 572 stays under narrow_ok's ceiling of 30 000; with 512 it would be 30 180)
    for row_char, col_char in ((b"A", b"C"), (b"A", b"A")):
        p1 = orc.create_profile_str(row_char * m)
        ref = col_char * n
        want = orc.gotoh_score_prof(p1, orc.create_profile_str(ref), 1, 0, sc)
        today = sd.sweep(p1, ref, sc, K, 0, ckpt=True, B=B)
        got = sd.sweep(p1, ref, sc, K, period, ckpt=True, B=B)
        assert today[0] == want and got[0] == want and got[1] == (0, 0)
        assert np.array_equal(got[2][1:n + 1], today[2][1:n + 1]) and np.array_equal(got[3], today[3])
