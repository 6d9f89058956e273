"""Device basecalling on synthetic chromatograms (hostlib.synth_decompose_batch signals, one call position every 12 samples), one JSON line:
device traces/s with everything resident (tracyhip_basecall_traces, TRACYHIP_MEM_DEVICE, int16 and int32 samples), with host buffers
(int16 and int32: upload, kernel and the copy back of every result included), the host chain's traces/s on the same data on this
process's threads (tracyhost_basecall_batch), the deferred count, a sampled comparison of every field with the host chain, and the
chained figure signals -> tracyhip_align_traces with the profiles never leaving the device.  Step times end in a device
synchronisation; warm-up steps are not timed.

    python tools/basecall_device_line.py [--traces 10000] [--bases 1000] [--steps 10] [--warmup 2] [--threads 16] [--align-traces 10000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

SCORE = (3, -5, -10, -4)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=10000)
    ap.add_argument("--bases", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--align-traces", type=int, default=10000)
    ap.add_argument("--stringency", type=float, default=4.0)
    ap.add_argument("--sample", type=int, default=200, help="traces compared field by field with the host chain")
    a = ap.parse_args()

    import tracy_amd
    from tracy_amd import capi, hostlib
    nt, mf = a.traces, a.bases
    data = hostlib.synth_decompose_batch(7000, nt, mf + 400, mf, a.threads, mix=1)
    sig32 = data["signal"]  # [nt][4][ns]
    ns = sig32.shape[2]
    assert int(np.abs(sig32).max()) < 32768
    sig16 = sig32.astype(np.int16)
    pos = np.tile(np.arange(mf, dtype=np.int32) * 12 + 6, (nt, 1))
    ctx = tracy_amd.Context(0)

    out = dict(tool="basecall_device_line", traces=nt, bases=mf, samples_per_trace=ns, steps=a.steps, warmup=a.warmup, threads=a.threads,
               stringency=a.stringency, device=torch.cuda.get_device_name(0))
    rates = {}
    keep = None
    for name, sig, dev in (("resident_int16", sig16, True), ("resident_int32", sig32, True), ("host_int16", sig16, False), ("host_int32", sig32, False)):
        p = capi.PreparedBasecall(list(sig), list(pos), 0.33, a.stringency, device=dev)
        ts = timed(lambda: p.run(ctx), a.steps, a.warmup)
        rates[name] = dict(step_s=[round(t, 6) for t in ts], traces_per_s=round(nt / min(ts), 1), traces_per_s_median=round(nt / float(np.median(ts)), 1))
        out["deferred_" + name] = int((p.meta["status"] != 0).sum())
        if name == "resident_int16":
            keep = p
        elif name == "host_int16":
            hostp = p
        else:
            del p
    # the feeding case: signals in host buffers, results stay on the device (what the next device stage takes) -- upload + call per step
    host16 = torch.from_numpy(keep.signal)
    pinned16 = host16.pin_memory()
    for name, src in (("upload_int16_pageable_then_resident", host16), ("upload_int16_pinned_then_resident", pinned16)):
        def step(src=src):
            keep.d_signal.copy_(src)
            keep.run(ctx)
        ts = timed(step, a.steps, a.warmup)
        rates[name] = dict(step_s=[round(t, 6) for t in ts], traces_per_s=round(nt / min(ts), 1), traces_per_s_median=round(nt / float(np.median(ts)), 1))
    out["device"] = rates

    # the host chain on the same data (int32, what the readers produce), threads as granted
    hs = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        secs, _ = hostlib.basecall_batch(sig32, pos, 0.33, a.stringency, a.threads, want=False)
        wall = time.perf_counter() - t0
        if i >= a.warmup:
            hs.append((secs, wall))
    best = min(s for s, _ in hs)
    out["host_chain"] = dict(chain_s=[round(s, 6) for s, _ in hs], wall_with_trace_copies_s=[round(w, 6) for _, w in hs],
                             traces_per_s=round(nt / best, 1), traces_per_s_per_thread=round(nt / best / a.threads, 1))
    out["host_int16_over_host_chain"] = round(rates["host_int16"]["traces_per_s"] / out["host_chain"]["traces_per_s"], 3)
    out["host_int32_over_host_chain"] = round(rates["host_int32"]["traces_per_s"] / out["host_chain"]["traces_per_s"], 3)

    # sampled comparison, every field
    k = min(a.sample, nt)
    idx = np.linspace(0, nt - 1, k).astype(int)
    _, want = hostlib.basecall_batch(sig32[idx], pos[idx], 0.33, a.stringency, a.threads)
    rows_d, rows_h = keep.results(False), hostp.results(False)
    same = 0
    for j, t in enumerate(idx):
        n = int(want["bc_len"][j])
        ok = True
        for r in (rows_d[t], rows_h[t]):
            ok &= r["status"] == 0 and r["bc_len"] == n and r["primary"] == want["primary"][j, :n].tobytes() and r["secondary"] == want["secondary"][j, :n].tobytes()
            ok &= np.array_equal(r["bcpos"], want["bcpos"][j, :n]) and np.array_equal(r["estqual"], want["estqual"][j, :n])
            ok &= np.array_equal(r["profile"].reshape(-1).view(np.uint32), want["profiles"][j, :6 * n].view(np.uint32))
            ok &= (r["trim_left"], r["trim_right"]) == tuple(int(x) for x in want["trims"][j])
        same += bool(ok)
    out["compared"] = int(k)
    out["identical"] = int(same)

    # signals -> align_traces, everything on the device: basecall (int16 upload included), then the alignment on the profiles as they stand
    na = min(a.align_traces, nt)
    refs = capi.PackedSeqs([r.tobytes() for r in data["refs"][:na]], capi.SEQ_CHAR)
    d_refs = torch.from_numpy(refs.data).cuda()

    pb = capi.PreparedBasecall(list(sig16[:na]), list(pos[:na]), 0.33, 0, device=True)
    host_sig = torch.from_numpy(pb.signal)
    cap = np.full(na, mf, np.uint64) + refs.length[:na].astype(np.uint64)
    off = np.zeros(na, np.uint64)
    off[1:] = np.cumsum(cap)[:-1]
    res = capi.AlignResult()
    bufs = {}
    for f, dt in (("score_fwd", torch.int32), ("score_rev", torch.int32), ("forward", torch.uint8), ("score_prelim", torch.int32),
                  ("slice_begin", torch.int32), ("slice_len", torch.int32), ("ref_pos", torch.int32), ("score_final", torch.int32),
                  ("ops_len", torch.int32)):
        bufs[f] = torch.zeros(na, dtype=dt, device="cuda")
        setattr(res, f, bufs[f].data_ptr())
    bufs["ops"] = torch.zeros(int(cap.sum()), dtype=torch.uint8, device="cuda")
    res.ops = bufs["ops"].data_ptr()
    res.ops_offset = off.ctypes.data_as(C.POINTER(C.c_uint64))
    prm = capi.Params(SCORE[0], SCORE[1], SCORE[2], SCORE[3], 1, 0)

    def chain():
        pb.d_signal.copy_(host_sig)  # int16 signals from the host buffer
        pb.run(ctx)
        job = capi.AlignJob()
        job.ntraces = na
        job.profiles = pb.profiles_seqset()
        job.refs = refs.seqset(d_refs.data_ptr())
        job.trim_left = job.trim_right = 50
        torch.cuda.synchronize()
        capi._check(capi.lib().tracyhip_align_traces(ctx._h, C.byref(job), C.byref(prm), capi.MEM_DEVICE, C.byref(res)))

    def align_only():
        job = capi.AlignJob()
        job.ntraces = na
        job.profiles = pb.profiles_seqset()
        job.refs = refs.seqset(d_refs.data_ptr())
        job.trim_left = job.trim_right = 50
        capi._check(capi.lib().tracyhip_align_traces(ctx._h, C.byref(job), C.byref(prm), capi.MEM_DEVICE, C.byref(res)))

    ts = timed(chain, a.steps, a.warmup)
    assert int(pb.meta["bc_len"][:na].min()) == mf and not pb.meta["status"].any()
    ta = timed(align_only, a.steps, a.warmup)
    out["signals_to_align"] = dict(traces=na, step_s=[round(t, 6) for t in ts], traces_per_s=round(na / min(ts), 1),
                                   align_only_step_s=[round(t, 6) for t in ta], align_only_traces_per_s=round(na / min(ta), 1),
                                   note="per step: int16 signals copied from a pageable host buffer, tracyhip_basecall_traces, tracyhip_align_traces on the device profiles as they stand")
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
