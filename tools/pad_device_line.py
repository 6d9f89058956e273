"""Gapped chromatograms of a plate of traces (tracyhip_pad_traces), one JSON line: traces/s of the call with chromatograms, basecalls,
rows and results resident on the device (int32 and int16 samples), of the call with host buffers, and of the host chain
(tracyhost_pad_batch: trimTrace, reverseComplementTrace, alignmentTracePadding per trace) on 16 threads in the same run; the kernel
time of the device-resident calls and achieved_GBps = sample_bytes * 4 * (ns + ns') summed over the traces / kernel time.  Every trace
is compared between the host chain and the device forms, every field.

The data: N synthetic 1 kb traces of 12 012 samples x 4 (hostlib.synth_decompose_batch, what bench.py's decompose workload renders) with
the rows of their final alignments from one align_traces call in the same process.  Workload "plain": no trims, forward.  Workload
"trim_reverse": trimTrace pairs at stringency 2 (the alignment run with them), every other trace reverse-complemented.  Each form is
timed `--reps` times, the forms interleaved; a timed step is the full call into buffers sized by one sizes-only call before the clock
starts, and ends in a device synchronisation.

    python tools/pad_device_line.py [--traces 10000] [--reps 3] [--out profiles/pad_device_line.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

SCORE = (3, -5, -10, -4)
HOST_THREADS = 16
TIMER_MISC = 8


class KernelTiming(C.Structure):
    _fields_ = [("ms", C.c_double), ("launches", C.c_uint64), ("cells", C.c_uint64), ("bytes", C.c_uint64)]


def rows_of(btr):
    """row 0 of the alignments from their op strings (push order): 'h' is a gap of the trace; only '-' against a letter is read"""
    out = []
    for b in btr:
        ops = np.frombuffer(b, np.uint8)[::-1]
        out.append(np.where(ops == ord("h"), ord("-"), ord("N")).astype(np.uint8).tobytes())
    return out


def same(a, b):
    if a["status"] != b["status"]:
        return False
    if a["status"] != 0:
        return True
    return (np.array_equal(a["signal"], b["signal"]) and np.array_equal(a["bcPos"], b["bcPos"]) and np.array_equal(a["estQual"], b["estQual"])
            and all(a[k] == b[k] for k in ("primary", "secondary", "consensus", "leadingGaps", "trailingGaps", "step")))


def workload(ctx, d, trims, reverse, reps):
    from tracy_amd import capi, hostlib
    nt, ns = d["signal"].shape[0], d["signal"].shape[2]
    lib = capi.lib()
    res = ctx.align_traces(list(d["profiles"]), [r.tobytes() for r in d["refs"]], SCORE, *(trims if trims else (50, 50)))
    rows = rows_of(res["btr"])  # (the final alignment is the untrimmed trace's, sage.h:300-321)
    if trims:  # the hard-trimmed trace keeps the columns from its first kept letter to its last
        for t, r in enumerate(rows):
            at = np.flatnonzero(np.frombuffer(r, np.uint8) != ord("-"))
            rows[t] = r[int(at[int(trims[0][t])]):int(at[len(at) - 1 - int(trims[1][t])]) + 1]
    bc = [dict(bcpos=d["bcpos"][t], primary=d["primary"][t], secondary=d["secondary"][t], consensus=d["primary"][t], estqual=d["estqual"][t])
          for t in range(nt)]
    tl, tr = trims if trims else (None, None)
    out = {"inserted_calls": 0}
    preps = {}
    for name, dt, device in (("device_int32", np.int32, True), ("device_int16", np.int16, True), ("host_int32", np.int32, False)):
        sigs = [d["signal"][t].astype(dt) if dt != np.int32 else d["signal"][t] for t in range(nt)]
        p = capi.PreparedPad(sigs, bc, rows, tl, tr, reverse, device=device, sample_dtype=dt)
        sizes = p.sizes(ctx)
        p.with_capacity(*sizes)
        preps[name] = p
    flat = preps["host_int32"].host_flat()
    hout = hostlib.pad_alloc(flat, *sizes)
    times = {k: [] for k in list(preps) + ["host_chain_16_threads"]}
    kernel_ms = {k: [] for k in preps if k.startswith("device")}
    capi._check(lib.tracyhip_timing_enable(ctx._h, 1))
    for rep in range(reps + 1):  # (the first round warms up and is not kept)
        for name, p in preps.items():
            capi._check(lib.tracyhip_timing_reset(ctx._h))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.run(ctx)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            kt = KernelTiming()
            capi._check(lib.tracyhip_timing_get(ctx._h, TIMER_MISC, C.byref(kt)))
            if rep:
                times[name].append(dt)
                if name in kernel_ms:
                    kernel_ms[name].append(kt.ms)
        t0 = time.perf_counter()
        hostlib.pad_batch_raw(flat, hout, HOST_THREADS)
        if rep:
            times["host_chain_16_threads"].append(time.perf_counter() - t0)
    capi._check(lib.tracyhip_timing_enable(ctx._h, 0))
    st = ctx.last_call_stats()
    moved = 4 * int((flat["nsamples"][:nt].astype(np.int64) + sizes[0].astype(np.int64)).sum())
    for name in times:
        best = min(times[name])
        out[name + "_traces_per_s"] = round(nt / best, 1)
        out[name + "_ms"] = [round(1e3 * x, 3) for x in times[name]]
    for name, sb in (("device_int32", 4), ("device_int16", 2)):
        ms = min(kernel_ms[name])
        out[name + "_kernel_ms"] = [round(x, 4) for x in kernel_ms[name]]
        out[name + "_achieved_GBps"] = round(sb * moved / (1e-3 * ms) / 1e9, 1)
    out["device_vs_host_chain"] = round(out["device_int32_traces_per_s"] / out["host_chain_16_threads_traces_per_s"], 2)
    out["host_syncs_host_buffers"], out["pad_chunks_host_buffers"] = st["host_syncs"], st["pad_chunks"]
    # every trace, every field, between the host chain and the three device forms
    want = [hostlib.pad_unpack(hout, t) for t in range(nt)]
    mism = deferred = 0
    for name, p in preps.items():
        got = p.results(fill_deferred=False)
        for t in range(nt):
            g = got[t]
            if name == "device_int16" and g["status"] == 0:
                g = dict(g, signal=g["signal"].astype(np.int32))
            mism += 0 if same(g, want[t]) else 1
            deferred += g["status"] != 0
    out["inserted_calls"] = int(sum(w["ncalls_out"] for w in want)) - int(sum(len(b["bcpos"]) - (int(tl[t]) + int(tr[t]) if trims else 0) for t, b in enumerate(bc)))
    out.update(compared=3 * nt, mismatches=mism, deferred=int(deferred), samples_in=ns, mean_samples_out=round(float(np.mean([w["nsamples_out"] for w in want])), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pad_device_line.json"))
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import hostlib
    nt, mf = a.traces, 1000
    d = hostlib.synth_decompose_batch(4711, nt, mf + 400, mf, 0, 1)  # (mix 1: a tenth of the traces carry a homozygous indel -- rows with gaps)
    # qualities as estimateQualities gives them travel with the calls; any bytes do here
    d["estqual"] = (np.arange(nt * mf, dtype=np.int64).reshape(nt, mf) % 61).astype(np.uint8)
    ctx = tracy_amd.Context(0)
    out = {"traces": nt, "bases": mf, "samples": int(d["signal"].shape[2]), "reps": a.reps, "host_threads": HOST_THREADS}
    out["plain"] = workload(ctx, d, None, None, a.reps)
    trims = [hostlib.trim_trace(d["signal"][t], d["bcpos"][t], 0.33, 2.0) for t in range(nt)]
    tl = np.array([x[0] for x in trims], np.uint32)
    tr = np.array([x[1] for x in trims], np.uint32)
    keep = tl.astype(np.int64) + tr < mf - 100  # (a trace trimmed to nothing aligns nothing: it keeps the default pair)
    tl, tr = np.where(keep, tl, 50).astype(np.uint32), np.where(keep, tr, 50).astype(np.uint32)
    out["trim_reverse"] = workload(ctx, d, (tl, tr), [t % 2 == 1 for t in range(nt)], a.reps)
    ctx.close()
    out["mismatches"] = out["plain"]["mismatches"] + out["trim_reverse"]["mismatches"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["mismatches"] == 0 and out["plain"]["deferred"] == 0 and out["trim_reverse"]["deferred"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
