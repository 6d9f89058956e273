"""The text printed from a batch of decompose results (tracyhip_render_decompositions), one JSON line.  Per form (the .decomp table, the
tail of the JSON report, the record lines of the VCF): ms of the call with every payload and the text resident on the device; the call
from host buffers end to end; the host writers (tracyhost_dcptext_batch: writeDecomposition / traceAlleleAlignJsonTail / vcfRecordLines
into a TextBuf per trace) on 16 threads on the same data in the same run; and the comparison that decides where a caller should print:
    results_back_then_host_print   rows, tables, basecall positions and qualities and the variant arrays copied device -> host, then the
                                   host writers on 16 threads
    device_print_then_text_back    the device call, then the text copied device -> host
Every trace's text is compared between the host writers and both device forms.

The data: heterozygous 1 kb traces against 3 kb windows (hostlib.synth_decompose, the shape of bench.py's decompose workload), odd ones
on the reverse strand, carried through decompose_traces -> alignment_rows -> decompose_variants once for `--distinct` traces; the batch
of `--traces` repeats their result arrays back to back, so that every trace of the batch reads payload bytes of its own.  One warm-up
round and `--reps` timed rounds, the forms interleaved; a timed device step ends in a device synchronisation.

    python tools/dcptext_device_line.py [--traces 20000] [--distinct 64] [--reps 3] [--out profiles/dcptext_device_line.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

SCORE = (3, -5, -10, -4)
HOST_THREADS = 16
TRIMS = (50, 50)
QUAL_CUT = 45
MAXV, MAXT = 64, 1024
FORM_NAMES = {0: "decomp", 1: "json", 2: "vcf"}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def distinct_cases(ctx, n):
    """n traces through the chain, from host buffers: the per-trace dicts of hostlib.dcptext_pack of those that decompose"""
    import dcptext_chain as ch
    import indigo_oracle as io
    from sage_oracle import revcomp
    from tracy_amd import capi, hostlib
    cases = []
    for i in range(n):
        ref, sig, pos, _ = hostlib.synth_decompose(5000 + i, 3000, 1000, 30, 0, (0.6, 0.55, 0.7)[i % 3])
        if i % 2:
            ref = revcomp(ref)
        pri, sec, _, bcpos, estq = hostlib.basecall_qual(sig, pos, ch.PRATIO)
        hbc = capi.HostBaseCalls([sig], [bcpos], [pri], [sec])
        prof = hostlib.create_profile(sig, bcpos, pri, sec, 0, 0)
        o = ctx.decompose_traces([prof], hbc, [ref], SCORE, *TRIMS)
        if int(o["status"][0]) != 0:
            continue
        var, flags = ctx.decompose_variants(o, [1000 * i], MAXV, MAXT)
        if int(flags[0]):
            continue
        w = dict(forward=int(o["forward"][0]), bp=o["bp"][0], af=tuple(float(x) for x in o["fractions"][:2]), dcp=o["dcp"][0], primary=o["primary"][0],
                 secdecomp=o["secdecomp_list"][0])
        for k in range(3):
            w["score%d" % k], w["btr%d" % k] = int(o["score%d" % k][0]), o["btr%d" % k][0]
        for k in range(2):
            for nm in ("slice_begin", "slice_len", "ref_pos"):
                w["%s%d" % (nm, k)] = int(o["%s%d" % (nm, k)][0])
        al, sl = ch.alleles(w, TRIMS), ch.slices(w, ref)
        pairs = [(al[0], sl[0], w["btr0"]), (al[1], sl[1], w["btr1"]), (al[0], al[1], w["btr2"])]
        rows = []
        for a, b, btr in pairs:  # tracyhip_alignment_rows, one pair a call
            pa, pb = capi.PackedSeqs([a], capi.SEQ_CHAR), capi.PackedSeqs([b], capi.SEQ_CHAR)
            pr = capi.Pairs()
            pr.npairs, pr.a1, pr.a2 = 1, pa.seqset(), pb.seqset()
            ops = np.frombuffer(btr + b"\0", np.uint8).copy()
            off, olen = np.zeros(1, np.uint64), np.array([len(btr)], np.uint32)
            r0, r1 = np.zeros_like(ops), np.zeros_like(ops)
            u8p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint8))
            capi._check(capi.lib().tracyhip_alignment_rows(ctx._h, C.byref(pr), capi.MEM_HOST, u8p(ops), capi._u64p(off), capi._u32p(olen), u8p(r0), u8p(r1)))
            rows.append((r0[:len(btr)].tobytes(), r1[:len(btr)].tobytes()))
        cases.append(ch.trace_case(w, rows, bcpos, estq, var[0], 1000 * i, TRIMS, b"chr%d" % (i % 22 + 1)))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=20000)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcptext_device_line.json"))
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi, hostlib
    ctx = tracy_amd.Context(0)
    base = distinct_cases(ctx, a.distinct)
    cases = [base[i % len(base)] for i in range(a.traces)]
    nt = len(cases)
    flat = hostlib.dcptext_pack(cases, MAXV, MAXT)
    out = {"traces": nt, "distinct_traces": len(base), "trace_len": 1000, "window_len": 3000, "max_variants": MAXV, "max_text": MAXT,
           "host_threads": HOST_THREADS, "reps": a.reps, "variants": int(flat["var_n"][:nt].sum()),
           "rows_bytes": int(2 * sum(int(flat["cols_%d" % k][:nt].sum()) for k in range(3))), "device": torch.cuda.get_device_name(0)}
    back_keys = {0: ("dcp_indel", "dcp_err"), 2: ("bcpos", "estqual", "var", "var_text", "var_n")}
    back_keys[1] = back_keys[0] + back_keys[2] + tuple("rows%d_%d" % (r, k) for k in range(3) for r in range(2))
    prepared, texts = {}, {}
    for form in FORM_NAMES:
        pd = capi.PreparedDcpText(form, flat, QUAL_CUT, device=True)
        sizes = pd.sizes(ctx)
        pd.with_capacity(sizes)
        ph = capi.PreparedDcpText(form, flat, QUAL_CUT).with_capacity(sizes)
        prepared[form] = (pd, ph, sizes)
    res = {f: {k: [] for k in ("resident_ms", "host_buffers_ms", "host_writers_ms", "results_back_then_host_print_ms", "device_print_then_text_back_ms")}
           for f in FORM_NAMES}
    for rep in range(a.reps + 1):
        for form in FORM_NAMES:
            pd, ph, sizes = prepared[form]
            t_res = timed(lambda: pd.run(ctx))
            t_hb = timed(lambda: ph.run(ctx))
            hout = hostlib.dcptext_alloc(nt, sizes)
            t0 = time.perf_counter()
            hostlib.dcptext_batch_raw(flat, form, hout, QUAL_CUT, HOST_THREADS)
            t_hw = time.perf_counter() - t0
            nbytes = int(pd.o["text_offset"][nt])
            pinned = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
            t_back = timed(lambda: pinned.copy_(pd.o["text"][:max(nbytes, 1)], non_blocking=True))
            dst = {k: torch.empty_like(pd.d[k], device="cpu").pin_memory() for k in back_keys[form]}
            t_copy = timed(lambda: [dst[k].copy_(pd.d[k], non_blocking=True) for k in back_keys[form]])
            if rep:
                r = res[form]
                r["resident_ms"].append(1e3 * t_res); r["host_buffers_ms"].append(1e3 * t_hb); r["host_writers_ms"].append(1e3 * t_hw)
                r["results_back_then_host_print_ms"].append(1e3 * (t_copy + t_hw)); r["device_print_then_text_back_ms"].append(1e3 * (t_res + t_back))
            texts[form] = (pd.results(fill_deferred=False), ph.results(fill_deferred=False), [hostlib.dcptext_unpack(hout, t) for t in range(nt)]) if rep == a.reps else None
    differing = 0
    for form, name in FORM_NAMES.items():
        pd, ph, sizes = prepared[form]
        d, h, w = texts[form]
        bad = [t for t in range(nt) if not (d[t]["status"] == h[t]["status"] == w[t]["status"] == 0 and d[t]["text"] == h[t]["text"] == w[t]["text"])]
        differing += len(bad)
        nbytes = int(sizes.astype(np.uint64).sum())
        med = {k: round(float(np.median(v)), 3) for k, v in res[form].items()}
        out[name] = dict(med, text_bytes=nbytes, result_bytes_back=int(sum(pd.d[k].numel() * pd.d[k].element_size() for k in back_keys[form])),
                         resident_gb_per_s=round(nbytes / med["resident_ms"] / 1e6, 2) if med["resident_ms"] else None,
                         host_writers_over_resident=round(med["host_writers_ms"] / med["resident_ms"], 2) if med["resident_ms"] else None,
                         back_then_print_over_print_then_back=round(med["results_back_then_host_print_ms"] / med["device_print_then_text_back_ms"], 2),
                         traces_differing=len(bad), first_differing=bad[:4])
    out["traces_compared"] = nt
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    ctx.close()
    return 0 if differing == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
