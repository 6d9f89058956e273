"""tracyhost_dcptext_batch (the tail of the JSON report and the record lines of the VCF, callable alone) against the files the whole-file
writers print for the same decompose results: the oracle chain on two small traces, one of them on the reverse strand.  No device."""
import numpy as np
import pytest

import dcptext_cases as dc
import dcptext_chain as ch
import indigo_oracle as io
from decomp_cases import SC
from sage_oracle import revcomp

TRIMS = (20, 20)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_the_batch_prints_what_the_files_hold(tmp_path, reverse):
    from tracy_amd import hostlib
    ref, sig, pos, _ = hostlib.synth_decompose(411 + int(reverse), 500, 250, 12, 0, 0.6)
    if reverse:
        ref = revcomp(ref)
    pri, sec, _, bcpos, estq = hostlib.basecall_qual(sig, pos, ch.PRATIO)
    w = io.decompose_trace(sig, bcpos, pri, sec, ref, SC, *TRIMS)
    assert w["status"] == 0 and bool(w["forward"]) != reverse and w["bp"].indelshift
    rows = ch.report_rows(w, ref, TRIMS)
    vrows = ch.variant_rows(w, ref, TRIMS, rows)
    slice_pos = 12345
    variants = ch.oracle_variants(w, vrows, slice_pos)
    assert variants
    files = ch.whole_file_texts(tmp_path, w, sig, pos, ref, rows, vrows, slice_pos, TRIMS)
    case = ch.trace_case(w, rows, bcpos, estq, variants, slice_pos, TRIMS)
    flat = hostlib.dcptext_pack([case], 64, 1024)
    for form in dc.FORMS:
        got = hostlib.dcptext_batch(flat, form, ch.QUAL_CUT, 1)[0]
        assert got["status"] == 0 and got["text"] == files[form], form
        assert got["text"] == dc.expected(dict(case, maxv=64, maxt=1024, qc=ch.QUAL_CUT), form), form
    assert files[dc.VCF].count(b"\n") == len(variants) and files[dc.JSON].endswith(b"]\n}\n}\n")
