"""Two-trace consensus of a batch on the device (tracyhip_consensus_traces), one JSON line: pairs/s with host buffers (MEM_HOST) and with
payloads and results in device memory (MEM_DEVICE), the consensus columns the device screen handed to the host gtLetter, a CPU baseline
from the oracle restatement (tests/consensus_oracle.py over pyoracle's DP, on --threads processes; a checker and baseline only) and the
result of checking a sample of pairs against that restatement field by field.

The data: N synthetic pairs of 1 kb trace-like profiles (the called base carries most of each column) of two overlapping windows of a
random genome with 2 % substitutions; every other second trace is read from the reverse strand.  Step times end in a device
synchronisation; warm-up steps are not timed.

    python tools/consensus_device_line.py [--pairs 10000] [--steps 3] [--warmup 1] [--check 200] [--threads 16]
"""
import argparse
import json
import multiprocessing
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

SCORE = (3, -5, -10, -4)
FIELDS = ("score_fwd", "score_rev", "forward", "score", "num_aligned", "num_match", "status")


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


def build_pairs(n, length=1000, seed=31):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    first, second = [], []
    for i in range(n):
        g = lut[rng.integers(0, 4, size=2 * length)]
        s2 = int(rng.integers(100, 400))
        a = g[:length].copy()
        b = g[s2:s2 + length].copy()
        for x in (a, b):
            hit = rng.random(length) < 0.02
            x[hit] = lut[rng.integers(0, 4, size=int(hit.sum()))]
        pa, pb = profile_of(rng, a.tobytes()), profile_of(rng, b.tobytes())
        first.append(pa)
        second.append(revcomp(pb) if i % 2 else pb)
    return first, second


def oracle_one(args):
    p1, f2 = args
    import assemble_oracle as ao
    import consensus_oracle as co
    import pyoracle as orc
    r2 = np.ascontiguousarray(orc.revcomp_profile(f2))
    gf = orc.gotoh_score_prof(p1, f2, 1, 1, SCORE)
    gr = orc.gotoh_score_prof(p1, r2, 1, 1, SCORE)
    fwd = gf > gr
    p2 = f2 if fwd else r2
    sc, btr = orc.gotoh_prof(p1, np.ascontiguousarray(p2), 1, 1, SCORE)
    row0, row1, _ = ao.rows_of(p1, p2, btr)
    aligned = sum(1 for a, b in zip(row0, row1) if a != "-" and b != "-")
    matches = sum(1 for a, b in zip(row0, row1) if a != "-" and b != "-" and a == b)
    ok = not (aligned < 25 or (matches / aligned if aligned else 0.0) < float(np.float32(0.5)))
    cons, qual = co.pairwise_consensus(row0, row1, p1, p2, True, False) if ok else ("", [])
    return dict(score_fwd=gf, score_rev=gr, forward=int(fwd), score=sc, num_aligned=aligned, num_match=matches, status=0 if ok else 1,
                rows=(row0.encode(), row1.encode()), cons=cons.encode(), qual=list(qual))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=200, help="pairs compared with the oracle restatement (and timed as the CPU baseline)")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi
    first, second = build_pairs(a.pairs)
    ctx = tracy_amd.Context(0)
    out = {"pairs": a.pairs, "length": 1000, "score": SCORE}

    p = capi.PreparedConsensus(first, second, SCORE)
    for _ in range(a.warmup):
        capi._check(capi.lib().tracyhip_consensus_traces(ctx._h, capi.C.byref(p.job), capi.C.byref(p.prm), capi.MEM_HOST, capi.C.byref(p.out)))
    t0 = time.perf_counter()
    for _ in range(a.steps):
        capi._check(capi.lib().tracyhip_consensus_traces(ctx._h, capi.C.byref(p.job), capi.C.byref(p.prm), capi.MEM_HOST, capi.C.byref(p.out)))
    dt = (time.perf_counter() - t0) / a.steps
    stats = ctx.last_call_stats()
    out.update(host_pairs_per_s=round(a.pairs / dt, 1), host_ms=round(1e3 * dt, 3), fixup_columns=stats["cons_fixup_columns"],
               chunks=stats["cons_chunks"], host_syncs=stats["host_syncs"])
    got = p.results()
    out["no_overlap"] = int((got["status"] == 1).sum())
    out["forward"] = int(got["forward"].sum())

    q = capi.PreparedConsensus(first, second, SCORE)
    q.to_device()
    for _ in range(a.warmup):
        capi._check(capi.lib().tracyhip_consensus_traces(ctx._h, capi.C.byref(q.job), capi.C.byref(q.prm), capi.MEM_DEVICE, capi.C.byref(q.out)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        capi._check(capi.lib().tracyhip_consensus_traces(ctx._h, capi.C.byref(q.job), capi.C.byref(q.prm), capi.MEM_DEVICE, capi.C.byref(q.out)))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    out.update(device_pairs_per_s=round(a.pairs / dt, 1), device_ms=round(1e3 * dt, 3))
    q.from_device()
    gotd = q.results()
    same = all(np.array_equal(got[k], gotd[k]) for k in FIELDS) and got["rows"] == gotd["rows"] and got["cons"] == gotd["cons"] and \
        all(np.array_equal(x, y) for x, y in zip(got["qual"], gotd["qual"]))
    out["mem_device_identical"] = bool(same)
    ctx.close()

    # CPU baseline and checker: the oracle restatement on a sample, on `threads` processes
    idx = np.linspace(0, a.pairs - 1, min(a.check, a.pairs)).astype(int).tolist()
    t0 = time.perf_counter()
    with ProcessPoolExecutor(max_workers=a.threads, mp_context=multiprocessing.get_context("spawn")) as ex:  # (CPU only, fresh processes)
        want = list(ex.map(oracle_one, [(first[i], second[i]) for i in idx], chunksize=max(1, len(idx) // (4 * a.threads))))
    dt = time.perf_counter() - t0
    out.update(cpu_oracle_threads=a.threads, cpu_oracle_pairs_per_s=round(len(idx) / dt, 1))
    mism = 0
    for i, w in zip(idx, want):
        bad = any(int(got[k][i]) != int(w[k]) for k in FIELDS) or got["rows"][i] != w["rows"] or got["cons"][i] != w["cons"] or \
            [int(v) for v in got["qual"][i]] != w["qual"]
        mism += int(bad)
    out.update(checked=len(idx), mismatches=mism)
    print(json.dumps(out))
    return 0 if mism == 0 and same else 1


if __name__ == "__main__":
    sys.exit(main())
