"""A plate of traces against shared wildtype traces (tracyhip_align_traces with wildtype profiles as `refs`), one JSON line: traces/s of the one call
with host buffers (MEM_HOST), of the one call with payloads and results in device memory (MEM_DEVICE), and of the FORMER sequence on
the same data in the same run -- what `tracy_amd_cli align -r wildtype.ab1` did per block before the call existed: the host
reverse-complements every job's wildtype, both strands of every job are uploaded for tracyhip_gotoh_score, the host decides the strand
after the copy back, tracyhip_gotoh_align runs the final alignments and tracyhip_alignment_rows uploads the payloads a second time.
Every trace is compared between the two forms (strand, final score, op string, both rows).

The data: N synthetic 1 kb trace-like profiles, P of them per 1 kb wildtype (2 % substitutions), every other trace read from the
reverse strand; trims 50 / 50.  Step times end in a device synchronisation; warm-up steps are not timed.  The former sequence is timed
twice: its three library calls with the strand decision between them (packed inputs prepared before the clock starts, like the one
call's), and separately the host work it needs before them (reverse complement and packing of the second strand).

    python tools/wildtype_device_line.py [--traces 10000] [--per-wildtype 96] [--steps 3] [--warmup 1]
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
TRIM = 50
TIMERS = ("score", "trace", "walk", "misc")


def profile_of(rng, seq):
    n = len(seq)
    w = rng.random((4, n), dtype=np.float32) * np.float32(0.06)
    idx = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), np.frombuffer(seq, np.uint8))
    w[idx, np.arange(n)] += rng.uniform(0.75, 1.0, n).astype(np.float32)
    p = np.zeros((6, n), np.float32)
    p[:4] = w / w.sum(0, keepdims=True)
    return p


def revcomp(p):
    return np.ascontiguousarray(np.stack([p[3, ::-1], p[2, ::-1], p[1, ::-1], p[0, ::-1], p[4, ::-1], p[5, ::-1]]))


def build(n, per, length=1000, seed=47):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    traces, wild, ridx = [], [], []
    for i in range(n):
        if i % per == 0:
            g = lut[rng.integers(0, 4, size=length + 100)]
            wild.append(profile_of(rng, g[50:50 + length].tobytes()))
        a = g[int(rng.integers(0, 100)):][:length].copy()
        hit = rng.random(length) < 0.02
        a[hit] = lut[rng.integers(0, 4, size=int(hit.sum()))]
        p = profile_of(rng, a.tobytes())
        traces.append(revcomp(p) if i % 2 else p)
        ridx.append(len(wild) - 1)
    return traces, wild, np.array(ridx, np.uint32)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=10000)
    ap.add_argument("--per-wildtype", type=int, default=96)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi
    lib = capi.lib()
    nt = a.traces
    traces, wild, ridx = build(nt, a.per_wildtype)
    ctx = tracy_amd.Context(0)
    out = {"traces": nt, "per_wildtype": a.per_wildtype, "wildtypes": len(wild), "length": 1000, "score": SCORE, "trim": TRIM,
           "steps": a.steps, "warmup": a.warmup}

    # ---- the one call, host buffers ----
    p = capi.PreparedAlign(traces, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=wild, rows=True)
    one = lambda prep, mem: capi._check(lib.tracyhip_align_traces(ctx._h, C.byref(prep.job), C.byref(prep.prm), mem, C.byref(prep.out)))
    dt = timed(lambda: one(p, capi.MEM_HOST), a.steps, a.warmup)
    st = ctx.last_call_stats()
    out.update(host_traces_per_s=round(nt / dt, 1), host_ms=round(1e3 * dt, 3), chunks=st["wt_chunks"], host_syncs=st["host_syncs"])
    got = p.results()
    out["forward"] = int(got["forward"].sum())

    # ---- the one call, payloads and results resident on the device ----
    q = capi.PreparedAlign(traces, None, SCORE, TRIM, TRIM, ref_index=ridx, ref_profiles=wild, rows=True)
    pp, pw = q.keep[0], q.keep[1]
    dp, dw = torch.from_numpy(pp.data).cuda(), torch.from_numpy(pw.data).cuda()
    q.job.profiles, q.job.refs = pp.seqset(dp.data_ptr()), pw.seqset(dw.data_ptr())
    dres = {k: torch.zeros(v.nbytes, dtype=torch.uint8, device="cuda") for k, v in q.res.items()}
    for k, v in dres.items():
        setattr(q.out, k, v.data_ptr())
    dt = timed(lambda: one(q, capi.MEM_DEVICE), a.steps, a.warmup)
    out.update(device_traces_per_s=round(nt / dt, 1), device_ms=round(1e3 * dt, 3))
    for k, v in dres.items():
        q.res[k] = v.cpu().numpy().view(q.res[k].dtype)
    gotd = q.results()
    keys = ("score_fwd", "score_rev", "forward", "score_final")
    out["mem_device_identical"] = bool(all(np.array_equal(got[k], gotd[k]) for k in keys) and got["btr"] == gotd["btr"] and
                                       got["rows0"] == gotd["rows0"] and got["rows1"] == gotd["rows1"])

    # ---- the former sequence: host reverse complement, three calls, the strand decided on the host ----
    t0 = time.perf_counter()
    both = []
    for i in range(nt):  # forward, then reverse complement, per JOB (even where 96 jobs share one wildtype)
        w = wild[int(ridx[i])]
        both += [w, revcomp(w)]
    pref = capi.PackedSeqs(both, capi.SEQ_PROFILE)
    out["former_host_revcomp_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    ptrim = capi.PackedSeqs([np.ascontiguousarray(t[:, TRIM:t.shape[1] - TRIM]) for t in traces], capi.SEQ_PROFILE)
    pfull = p.keep[0]
    idx1 = np.repeat(np.arange(nt, dtype=np.uint32), 2)
    idx2 = np.arange(2 * nt, dtype=np.uint32)
    sp, keep1, _, _ = capi.Context._pairs(ptrim, pref, idx1, idx2)
    prm = capi.Params(SCORE[0], SCORE[1], SCORE[2], SCORE[3], 1, 0)
    gs = np.zeros(2 * nt, np.int32)
    cap = pfull.length[:nt].astype(np.uint64) + pref.length[0::2].astype(np.uint64)
    off = np.zeros(nt, np.uint64)
    off[1:] = np.cumsum(cap)[:-1]
    total = int(cap.sum())
    ops, r0, r1 = np.zeros(total, np.uint8), np.zeros(total, np.uint8), np.zeros(total, np.uint8)
    olen, sc = np.zeros(nt, np.uint32), np.zeros(nt, np.int32)
    u8p, u32p, u64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    state = {}
    # the pair list of the final alignments is prepared before the clock starts, like everything else; the strand decision between the
    # calls -- part of the former sequence -- only fills its a2 indices
    pick = np.zeros(nt, np.uint32)
    even = 2 * np.arange(nt, dtype=np.uint32)
    fp, keep2, _, _ = capi.Context._pairs(pfull, pref, np.arange(nt, dtype=np.uint32), pick)
    pick = keep2[-1]  # (the array the pair list points to)

    def former():
        capi._check(lib.tracyhip_gotoh_score(ctx._h, C.byref(sp), C.byref(prm), capi.MEM_HOST, gs.ctypes.data_as(i32p)))
        fwd = gs[0::2] > gs[1::2]
        np.add(even, np.where(fwd, 0, 1), out=pick, casting="unsafe")
        capi._check(lib.tracyhip_gotoh_align(ctx._h, C.byref(fp), C.byref(prm), capi.MEM_HOST, sc.ctypes.data_as(i32p), ops.ctypes.data_as(u8p),
                                             off.ctypes.data_as(u64p), olen.ctypes.data_as(u32p)))
        capi._check(lib.tracyhip_alignment_rows(ctx._h, C.byref(fp), capi.MEM_HOST, ops.ctypes.data_as(u8p), off.ctypes.data_as(u64p),
                                                olen.ctypes.data_as(u32p), r0.ctypes.data_as(u8p), r1.ctypes.data_as(u8p)))
        state["fwd"] = fwd

    dt = timed(former, a.steps, a.warmup)
    out.update(former_traces_per_s=round(nt / dt, 1), former_ms=round(1e3 * dt, 3))
    ctx.close()

    # ---- every trace compared between the two forms ----
    cut = lambda arr, i: arr[int(off[i]):int(off[i]) + int(olen[i])].tobytes()
    mism = 0
    for i in range(nt):
        bad = int(got["forward"][i]) != int(state["fwd"][i]) or int(got["score_final"][i]) != int(sc[i]) or \
            int(got["score_fwd"][i]) != int(gs[2 * i]) or int(got["score_rev"][i]) != int(gs[2 * i + 1]) or \
            got["btr"][i] != cut(ops, i) or got["rows0"][i] != cut(r0, i) or got["rows1"][i] != cut(r1, i)
        mism += int(bad)
    out.update(compared=nt, identical=bool(mism == 0), mismatches=mism,
               speedup_host_vs_former=round(out["host_traces_per_s"] / out["former_traces_per_s"], 3))
    print(json.dumps(out))
    return 0 if mism == 0 and out["mem_device_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
