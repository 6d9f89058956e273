"""De novo assembly of a batch of trace groups on the device (tracyhip_denovo_traces), one JSON line: groups/s with host buffers
(MEM_HOST) and with payloads and results in device memory (MEM_DEVICE), and -- in the same run -- the same groups through the path the
one-group command takes (tracy_amd/host/msa.hpp through msalib: revSeqBasedOnDist with one small score call per trace and iteration,
the overlap filter with one traceback call per round, msa() with one call per tree height, the merges, createProfile and the
consensus in host C++).  A sample of groups is compared between the two, every field.

The per-group path is driven through the Python binding here (the filter's verdicts in Python), so its figure carries some
interpreter time per round; the device calls and their round trips are the same ones the command makes.

The data: G synthetic amplicon groups, each K trace-like profiles of 1 kb tiled over a 3 kb region with 1 % substitutions, every
third one read from the reverse strand.  Step times end in a device synchronisation; warm-up steps are not timed.  The stage split is
the wall time of the call's stages (each ends in a synchronisation), printed by the library under the option `verbose`; the kernel
times are those of tracyhip_timing_get.

    python tools/denovo_device_line.py [--groups 200] [--traces 8] [--steps 3] [--warmup 1] [--check 20]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

from tools.assemble_device_line import build_groups  # noqa: E402  (the same groups; the references are not used)

SCORE = (3, -5, -10, -4)
ENDFREE = SCORE + (1, 1)  # AlignConfig<true,true>
FRACMATCH, CALLED = 0.5, 0.1
NONE = 0xffffffff
TIMERS = (("score", 0), ("trace", 1), ("walk", 2), ("misc", 8))


def overlap_ok(na, gs, size):
    f32 = np.float32
    thr = float(f32(f32(f32(na) * f32(FRACMATCH)) * f32(SCORE[0])) + f32(f32(f32(na) * (f32(1) - f32(FRACMATCH))) * f32(SCORE[1])))
    return na / float(size) > 0.1 and na > 25 and gs > thr


def per_group_path(ctx, msalib, traces):
    """one group as the one-group command runs it: assemble_cli.inc, de novo branch"""
    K = len(traces)
    profs, fwd = msalib.rev_seq_based_on_dist(ctx, traces, SCORE)
    nxt, state, partner = [0] * K, [0] * K, [NONE] * K
    while True:
        who = []
        for i in range(K):
            if state[i]:
                continue
            if nxt[i] == i:
                nxt[i] += 1
            if nxt[i] >= K:
                state[i] = -1
                continue
            who.append(i)
        if not who:
            break
        sc, btr = ctx.align([profs[i] for i in who], [profs[nxt[i]] for i in who], ENDFREE)
        for k, i in enumerate(who):
            if overlap_ok(btr[k].count(b"s"), int(sc[k]), profs[i].shape[1]):
                state[i], partner[i] = 1, nxt[i]
            else:
                nxt[i] += 1
    keep = [i for i in range(K) if state[i] == 1]
    res = dict(forward=[int(f) for f in fwd], partner=partner, row=[NONE] * K, rows=[], gapped=b"", cons=b"", qual=b"")
    if len(keep) < 2:
        return res
    rows, sidx = msalib.msa(ctx, [profs[i] for i in keep], SCORE)
    for r, s in enumerate(sidx):
        res["row"][keep[s]] = r
    gapped, cs, qs = msalib.consensus(rows, CALLED, False)
    res.update(rows=rows, gapped=gapped, cons=cs, qual=qs)
    return res


class quiet_stdout:
    """file descriptor 1 to /dev/null for a while (revSeqBasedOnDist of msa.hpp prints its progress dots as the reference does)"""

    def __enter__(self):
        sys.stdout.flush()
        self.saved, self.null = os.dup(1), os.open(os.devnull, os.O_WRONLY)
        os.dup2(self.null, 1)

    def __exit__(self, *exc):
        os.dup2(self.saved, 1)
        os.close(self.saved)
        os.close(self.null)


def stage_line(ctx, call):
    """one call under the option `verbose`: the library's stage line from stderr, as a dict of its numbers"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            ctx.set_option("verbose", 1)
            call()
        finally:
            ctx.set_option("verbose", 0)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    line = [ln for ln in text.splitlines() if ln.startswith("tracyhip_denovo_traces:")]
    if not line:
        return {}
    return {k: float(v) for k, v in re.findall(r"(\w+_ms|pairs|rounds|heights|chunks) ([0-9.]+)", line[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=200)
    ap.add_argument("--traces", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=20, help="groups compared between the batched call and the per-group path")
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi, msalib
    groups, _ = build_groups(a.groups, a.traces)
    ctx = tracy_amd.Context(0)
    lib = capi.lib()
    out = {"groups": a.groups, "traces_per_group": a.traces, "trace_len": 1000, "region_len": 3000, "score": SCORE}
    call = lambda p, mem: capi._check(lib.tracyhip_denovo_traces(ctx._h, C.byref(p.job), C.byref(p.prm), mem, C.byref(p.out)))

    p = capi.PreparedDenovo(groups, SCORE, FRACMATCH, CALLED)
    for _ in range(a.warmup):
        call(p, capi.MEM_HOST)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        call(p, capi.MEM_HOST)
    dt = (time.perf_counter() - t0) / a.steps
    stats = ctx.last_call_stats()
    out.update(host_groups_per_s=round(a.groups / dt, 1), host_ms=round(1e3 * dt, 3), chunks=stats["denovo_chunks"], rounds=stats["denovo_rounds"],
               tree_heights=stats["denovo_steps"], host_syncs=stats["host_syncs"])
    got = p.results()
    out["kept_traces"] = int((got["partner"] != NONE).sum())
    out["assembled_groups"] = int((got["nrows"] > 0).sum())

    q = capi.PreparedDenovo(groups, SCORE, FRACMATCH, CALLED)
    q.to_device()
    for _ in range(a.warmup):
        call(q, capi.MEM_DEVICE)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        call(q, capi.MEM_DEVICE)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    out.update(device_groups_per_s=round(a.groups / dt, 1), device_ms=round(1e3 * dt, 3))
    q.from_device()
    gotd = q.results()
    same = all(np.array_equal(got[k], gotd[k]) for k in ("forward", "partner", "row", "nrows", "ncol", "cons_len")) and \
        all(got[k] == gotd[k] for k in ("rows", "gapped", "cons", "qual"))
    out["mem_device_identical"] = bool(same)

    # the stages of one more device-payload call: wall time per stage, kernel time per timer
    out["stage_ms"] = stage_line(ctx, lambda: call(q, capi.MEM_DEVICE))
    lib.tracyhip_timing_enable(ctx._h, 1)
    lib.tracyhip_timing_reset(ctx._h)
    call(q, capi.MEM_DEVICE)
    torch.cuda.synchronize()
    lib.tracyhip_timing_enable(ctx._h, 0)
    kt = capi.KernelTiming()
    kernels = {}
    for name, which in TIMERS:
        lib.tracyhip_timing_get(ctx._h, which, C.byref(kt))
        kernels[name] = dict(ms=round(kt.ms, 3), launches=int(kt.launches), gcells=round(kt.cells / 1e9, 3))
    out["kernel_ms"] = kernels

    # the per-group path: every group once (after one untimed group that warms its kernels up)
    with quiet_stdout():
        per_group_path(ctx, msalib, groups[0])
        t0 = time.perf_counter()
        base = [per_group_path(ctx, msalib, t) for t in groups]
        dt = time.perf_counter() - t0
    out.update(per_group_groups_per_s=round(a.groups / dt, 1), per_group_ms=round(1e3 * dt, 3),
               speedup_host=round(dt / (1e-3 * out["host_ms"]), 2), speedup_device=round(dt / (1e-3 * out["device_ms"]), 2))
    ctx.close()
    idx = np.linspace(0, a.groups - 1, min(a.check, a.groups)).astype(int).tolist()
    first = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    mism = 0
    for g in idx:
        lo, hi = int(first[g]), int(first[g + 1])
        bad = any(got[k][lo:hi].tolist() != base[g][k] for k in ("forward", "partner", "row"))
        bad = bad or any(got[k][g] != base[g][k] for k in ("rows", "gapped", "cons", "qual"))
        mism += int(bad)
    out.update(checked=len(idx), mismatches=mism)
    print(json.dumps(out))
    return 0 if mism == 0 and same else 1


if __name__ == "__main__":
    sys.exit(main())
