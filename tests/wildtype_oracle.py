"""The wildtype-trace branches of `tracy align` (sage.h:261-300 + :311) and `tracy decompose` (indigo.h:252-291) composed from oracle
functions -- the expected behaviour of tracyhip_align_traces with wildtype profiles as its references and of tracyhip_decompose_traces
with ref_profiles and no `oriented` (tests only)."""
import numpy as np

import pyoracle as orc


def _bytes(x):
    return x if isinstance(x, (bytes, bytearray)) else x.encode()


def trimmed_view(profile_full, trim_left, trim_right):
    """createProfile's clamp (profile.h:24-27): l + r >= mf gives trims 0 / 0"""
    mf = profile_full.shape[1]
    tl, tr = int(trim_left), int(trim_right)
    if tl + tr >= mf:
        tl = tr = 0
    return np.ascontiguousarray(profile_full[:, tl:mf - tr])


def strand_scores(trimmed, wildtype, score):
    """(gsFwd, gsRev, revcomp profile): AlignConfig<true,false> as sage_oracle.align_trace"""
    rev = np.ascontiguousarray(orc.revcomp_profile(wildtype))
    return orc.gotoh_score_prof(trimmed, wildtype, 1, 0, score), orc.gotoh_score_prof(trimmed, rev, 1, 0, score), rev


def align_trace(profile_full, wildtype, score, trim_left=50, trim_right=50, oriented=None):
    """oriented: None = the strand by the two scores (a tie is reverse, sage.h:293); 0 / 1 = `wildtype` is already oriented and the
    flag is rs.forward: one score goes into both score fields"""
    trimmed = trimmed_view(profile_full, trim_left, trim_right)
    wildtype = np.ascontiguousarray(wildtype, dtype=np.float32)
    if oriented is None:
        gs_fwd, gs_rev, rev = strand_scores(trimmed, wildtype, score)
        forward = gs_fwd > gs_rev
        chosen = wildtype if forward else rev
    else:
        gs_fwd = gs_rev = orc.gotoh_score_prof(trimmed, wildtype, 1, 0, score)
        forward, chosen = bool(oriented), wildtype
    sc, btr = orc.gotoh_prof(profile_full, chosen, 1, 0, score)
    r0, r1 = orc.create_alignment_prof(btr, profile_full, chosen)[:2]
    return dict(score_fwd=gs_fwd, score_rev=gs_rev, forward=int(forward), score_prelim=gs_fwd if forward else gs_rev, slice_begin=0,
                slice_len=wildtype.shape[1], ref_pos=0, score_final=sc, btr=btr, rows0=_bytes(r0), rows1=_bytes(r1), chosen=chosen)


FIELDS = ("score_fwd", "score_rev", "forward", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final")


def check_trace(got, i, want):
    for k in FIELDS:
        assert int(got[k][i]) == int(want[k]), (i, k, int(got[k][i]), want[k])
    assert got["btr"][i] == want["btr"], i
    if "rows0" in got:
        assert got["rows0"][i] == want["rows0"], i
        assert got["rows1"][i] == want["rows1"], i


def decompose_trace(trace, wildtype_profile, wildtype_primary, score, tl=50, tr=50):
    """indigo.h:252-291 and on: `trace` holds sig / bcpos / pri / sec; the strand comes from the oracle's own two scores of the trimmed
    trace profile against the FORWARD wildtype profile and its reverse complement (oriented_forward=None)"""
    import indigo_oracle as io
    return io.decompose_trace(trace["sig"], trace["bcpos"], trace["pri"], trace["sec"], wildtype_primary, score, tl, tr,
                              oriented_forward=None, wildtype_profile=np.ascontiguousarray(wildtype_profile, dtype=np.float32))
