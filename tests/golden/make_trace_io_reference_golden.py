"""Generate tests/golden/trace_io_reference.json from the REFERENCE's own abif.h (oracle/_ref/libref_abif.so): what readab(),
basecall()'s quality estimate and traceTxtOut return for the inputs tests/test_trace_io.py builds (abif_cases with seed 41,
estqual_cases with seed 77), so that those tests hold on machines where oracle/_ref cannot be built.  Large arrays are kept as
SHA-256 digests of their little-endian int32 / uint8 bytes.  Run where oracle/_ref exists; the JSON is committed (data, not source)."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as orc  # noqa: E402
from test_trace_io import (GOLD_REF, abif_cases, abif_refused_cases, estqual_cases, ref_read_trace, sha256, trace_digest,  # noqa: E402
                           TRACE_TXT_TRIMS)


def main():
    ref = orc.ref_lib()
    assert ref is not None, "build oracle/_ref first (make -C oracle ref)"
    out = {"readab": {"files": [], "refused": []}, "estqual": []}
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(41)
        for p in abif_cases(rng, tmp):
            t = ref_read_trace(p)
            out["readab"]["files"].append(dict(file_sha256=sha256(open(p, "rb").read()), **trace_digest(t)))
        for p in abif_refused_cases(rng, tmp):
            out["readab"]["refused"].append(dict(file_sha256=sha256(open(p, "rb").read()), refused=ref_read_trace(p) is None))
        ref.ref_basecall_qual.restype = C.c_size_t
        b = os.path.join(tmp, "b.txt")
        for tr, pos in estqual_cases(np.random.default_rng(77)):
            n = len(pos)
            pri, sec, con = (C.create_string_buffer(n + 1) for _ in range(3))
            bc = np.zeros(max(n, 1), np.int32)
            q = np.zeros(max(n, 1), np.uint8)
            k = ref.ref_basecall_qual(tr.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(tr.shape[1]), pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                      C.c_size_t(n), C.c_float(0.33), pri, sec, con, bc.ctypes.data_as(C.POINTER(C.c_int32)),
                                      q.ctypes.data_as(C.POINTER(C.c_uint8)))
            txt = []
            for lt, rt in TRACE_TXT_TRIMS:
                rc = ref.ref_trace_txt(os.fsencode(b), tr.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(tr.shape[1]),
                                       pos.ctypes.data_as(C.POINTER(C.c_int32)), C.c_size_t(n), C.c_float(0.33), C.c_uint32(lt), C.c_uint32(rt))
                txt.append(dict(rc=int(rc), sha256=sha256(open(b, "rb").read()) if rc == 0 else None))
            out["estqual"].append(dict(trace_sha256=sha256(tr), basecallpos_sha256=sha256(pos), primary=pri.raw[:k].decode(),
                                       secondary=sec.raw[:k].decode(), estQual=q[:k].tolist(), trace_txt=txt))
    json.dump(out, open(GOLD_REF, "w"))
    print("wrote", len(out["readab"]["files"]), "ABIF files,", len(out["readab"]["refused"]), "refused files and", len(out["estqual"]),
          "quality / traceTxtOut cases")


if __name__ == "__main__":
    main()
