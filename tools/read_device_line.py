"""Reading a plate of chromatogram files on the device (tracyhip_read_traces), one JSON line.  Per sample width: ms of the call with the
file images and the results resident on the device (capacities from tracyhip_read_bound: one call, one synchronisation); the kernel time
of its launches (scan from the sizes-only call, emit as the rest) and read_GBps = (file bytes read + result bytes written) / kernel time;
the call from host buffers end to end; the host readers (tracyhost_read_batch: readab into the flattened layout) on 16 threads on the same
images in the same run; the count of deferred traces, which must be 0; every trace compared between the host batch and both device forms.
Then the chain file bytes -> chromatograms -> basecalls -> .abif table with everything resident (read_traces, basecall_traces,
render_traces) against the host stages on 16 threads (tracyhost_read_batch, tracyhost_basecall_batch, tracyhost_render_batch), the text
of every trace compared with the host writers' and that of the first 50 with hostlib.trace_txt of the host-read trace.

The data: N synthetic 1 kb traces of 12 012 samples x 4 (hostlib.synth_decompose_batch, what bench.py's decompose workload reads) written
as ABIF images by hostlib.write_abif.  One warm-up round and `--reps` timed rounds; a timed device step ends in a device synchronisation.

    python tools/read_device_line.py [--traces 10000] [--reps 3] [--out profiles/read_device_line.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

HOST_THREADS = 16
TIMER_MISC = 8


class KernelTiming(C.Structure):
    _fields_ = [("ms", C.c_double), ("launches", C.c_uint64), ("cells", C.c_uint64), ("bytes", C.c_uint64)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_ms(ctx, fn):
    from tracy_amd import capi
    lib = capi.lib()
    capi._check(lib.tracyhip_timing_reset(ctx._h))
    dt = timed(fn)
    kt = KernelTiming()
    capi._check(lib.tracyhip_timing_get(ctx._h, TIMER_MISC, C.byref(kt)))
    return dt, 1e-3 * kt.ms


def images(nt, mf):
    from tracy_amd import hostlib
    d = hostlib.synth_decompose_batch(4711, nt, mf + 400, mf, 0, 1)
    qual = (np.arange(nt * mf, dtype=np.int64).reshape(nt, mf) % 61).astype(np.uint8)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "t.ab1")
        for t in range(nt):
            hostlib.write_abif(p, np.clip(d["signal"][t], -32768, 32767), d["bcpos"][t], d["primary"][t].tobytes(), qual[t], d["secondary"][t].tobytes(),
                               (b"GATC", b"ACGT", b"TCGA", b"CATG")[t % 4])
            with open(p, "rb") as f:
                out.append(f.read())
    return out


def width(ctx, flat, dt, reps):
    from tracy_amd import capi, hostlib
    nt = flat["nt"]
    dev = capi.PreparedRead(flat, dt, device=True)
    caps = dev.bounds()
    # host buffers: exact capacities from the sizes-only call, so the regions follow each other and come back as one copy per array
    exact = dev.sizes(ctx)
    dev.with_capacity(*caps)
    host = capi.PreparedRead(flat, dt, device=False).with_capacity(*exact)
    hout = hostlib.read_alloc(nt, np.dtype(dt), *exact)
    t = {k: [] for k in ("device_resident", "host_buffers", "host_readers_16_threads", "kernel_scan", "kernel_all")}
    for rep in range(reps + 1):  # (the first round warms up and is not kept)
        o = dev.o
        _, scan = kernel_ms(ctx, lambda: dev.sizes(ctx))
        dev._bind(o)
        res, every = kernel_ms(ctx, lambda: dev.run(ctx))
        hb = timed(lambda: host.run(ctx))
        t0 = time.perf_counter()
        hostlib.read_batch_raw(flat, hout, HOST_THREADS)
        rd = time.perf_counter() - t0
        if rep:
            for k, v in dict(device_resident=res, host_buffers=hb, host_readers_16_threads=rd, kernel_scan=scan, kernel_all=every).items():
                t[k].append(v)
    best = {k: min(v) for k, v in t.items()}
    out = {k + "_ms": [round(1e3 * x, 3) for x in v] for k, v in t.items()}
    file_bytes = int(flat["file_len"][:nt].astype(np.int64).sum())
    sb = np.dtype(dt).itemsize
    result_bytes = int((4 * sb * dev.meta["nsamples"][:nt].astype(np.int64) + 7 * dev.meta["ncalls"][:nt].astype(np.int64)).sum())
    out.update(file_bytes=file_bytes, result_bytes=result_bytes, kernel_emit_ms=round(1e3 * (best["kernel_all"] - best["kernel_scan"]), 3),
               read_GBps=round((file_bytes + result_bytes) / best["kernel_all"] / 1e9, 1))
    for k in ("device_resident", "host_buffers", "host_readers_16_threads"):
        out[k + "_files_per_s"] = round(nt / best[k], 1)
    unequal = deferred = 0
    for p in (dev, host):
        got = p.host_arrays()
        deferred += int((got["status"][:nt] != 0).sum()) + int((hout["status"][:nt] != 0).sum())
        if p is host and all(np.array_equal(got[k][:nt], hout[k][:nt]) for k in ("status", "format", "nsamples", "ncalls")) and \
                all(np.array_equal(got[k], hout[k]) for k in ("signal", "basecallpos", "basecalls1", "basecalls2", "qual")):
            continue  # (the same layout: whole buffers)
        for i in range(nt):
            a, b = hostlib.read_unpack(got, i), hostlib.read_unpack(hout, i)
            same = a["status"] == b["status"] and all(np.array_equal(np.asarray(a.get(k)), np.asarray(b.get(k))) for k in ("signal", "basecallpos", "qual")) \
                and a.get("basecalls1") == b.get("basecalls1") and a.get("basecalls2") == b.get("basecalls2")
            unequal += 0 if same else 1
    out.update(compared=2 * nt, unequal=unequal, deferred=deferred)
    return out, dev, hout


def chain(ctx, flat, dev, hout, reps):
    """file bytes -> .abif table, resident, against the host stages on 16 threads"""
    from tracy_amd import capi, hostlib
    nt = flat["nt"]
    ns, npos = int(hout["nsamples"][0]), int(hout["ncalls"][0])
    assert (hout["nsamples"][:nt] == ns).all() and (hout["ncalls"][:nt] == npos).all()
    sig = hout["signal"][:4 * ns * nt].reshape(nt, 4, ns).astype(np.int32)  # (exact capacities: the regions follow each other)
    pos = hout["basecallpos"][:npos * nt].reshape(nt, npos)
    t = dict(device_chain=[], host_read=[], host_basecall=[], host_render=[])
    # the three prepared calls, built once: the images, every intermediate and the text stay on the device; a round is their three runs
    bc = ctx.basecall_traces(dev.run(ctx))
    render = capi.PreparedRender(capi.RENDER_TSV, device_bc=bc)
    render.with_capacity(render.bounds())
    state = dict(bc=bc, render=render)

    def device_chain():
        dev.run(ctx)
        bc.run(ctx)
        render.run(ctx)

    for rep in range(reps + 1):
        dc = timed(device_chain)
        t0 = time.perf_counter()
        hostlib.read_batch_raw(flat, hout, HOST_THREADS)
        t1 = time.perf_counter()
        hostlib.basecall_batch(sig, pos, 0.33, 0.0, HOST_THREADS, want=True)
        t2 = time.perf_counter()
        if rep == 0:
            hr = capi.PreparedRender(capi.RENDER_TSV, device_bc=state["bc"])
            hflat = hr.host_flat()
            hsizes = hostlib.render_batch_raw(hflat, 0, hostlib.render_alloc(nt, np.zeros(nt, np.uint64)), HOST_THREADS, sizes_only=True)["text_len"]
            htext = hostlib.render_alloc(nt, hsizes)
        t3 = time.perf_counter()
        hostlib.render_batch_raw(hflat, 0, htext, HOST_THREADS)
        t4 = time.perf_counter()
        if rep:
            for k, v in dict(device_chain=dc, host_read=t1 - t0, host_basecall=t2 - t1, host_render=t4 - t3).items():
                t[k].append(v)
    out = {k + "_ms": [round(1e3 * x, 3) for x in v] for k, v in t.items()}
    best = {k: min(v) for k, v in t.items()}
    host_chain = best["host_read"] + best["host_basecall"] + best["host_render"]
    out.update(device_chain_files_per_s=round(nt / best["device_chain"], 1), host_chain_16_threads_files_per_s=round(nt / host_chain, 1),
               ratio=round(host_chain / best["device_chain"], 2))
    res = state["render"].results(fill_deferred=False)
    unequal = sum(0 if (r["status"] == 0 and r["text"] == hostlib.render_unpack(htext, i).get("text")) else 1 for i, r in enumerate(res))
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "t.abif")
        for i in range(min(nt, 50)):
            hostlib.trace_txt(p, sig[i], pos[i])
            with open(p, "rb") as f:
                unequal += 0 if res[i].get("text") == f.read() else 1
    out.update(compared=nt + min(nt, 50), unequal=unequal,
               deferred=int((state["bc"].meta["status"][:nt] != 0).sum()) + int((state["render"].meta["status"][:nt] != 0).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_device_line.json"))
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi, hostlib
    nt, mf = a.traces, 1000
    flat = hostlib.read_pack(images(nt, mf))
    ctx = tracy_amd.Context(0)
    capi._check(capi.lib().tracyhip_timing_enable(ctx._h, 1))
    out = {"traces": nt, "bases": mf, "samples": 12 * mf + 12, "reps": a.reps, "host_threads": HOST_THREADS,
           "file_bytes_each": int(flat["file_len"][0])}
    for dt in (np.int16, np.int32):
        out[np.dtype(dt).name], dev, hout = width(ctx, flat, dt, a.reps)
        if dt == np.int16:
            out["chain_tsv_int16"] = chain(ctx, flat, dev, hout, a.reps)
        del dev, hout
        torch.cuda.empty_cache()
    ctx.close()
    parts = [v for v in out.values() if isinstance(v, dict)]
    out["unequal"] = sum(v["unequal"] for v in parts)
    out["deferred"] = sum(v["deferred"] for v in parts)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["unequal"] == 0 and out["deferred"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
