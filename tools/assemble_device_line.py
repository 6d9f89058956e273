"""Reference-guided assembly of a batch of trace groups on the device (tracyhip_assemble_traces), one JSON line: groups/s with host
buffers (MEM_HOST) and with payloads and results in device memory (MEM_DEVICE), and -- in the same run -- the same groups through the
path the one-group command takes: per group one strand-score call, then per chain step ONE one-pair tracyhip_gotoh_align with the host's
createProfile (msalib) before it and the host merge after it, and the host consensus.  A sample of groups is compared between the two,
every field.

The per-group path is driven through the Python binding here (merges in numpy, createProfile / consensus in the host C++), so its
figure carries some interpreter time per step; the device calls and their round trips are the same ones the command makes.

The data: G synthetic amplicon groups, each K trace-like profiles of 1 kb tiled over a 3 kb reference with 1 % substitutions, every
third one read from the reverse strand.  Step times end in a device synchronisation; warm-up steps are not timed.

    python tools/assemble_device_line.py [--groups 200] [--traces 8] [--steps 3] [--warmup 1] [--check 20]
"""
import argparse
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
SEMI = SCORE + (1, 0)  # AlignConfig<true,false>
FRACMATCH, CALLED = 0.5, 0.1
LETTERS = np.frombuffer(b"ACGTNN", np.uint8)


def profile_of(rng, seq):
    n = len(seq)
    w = rng.random((4, n), dtype=np.float32) * np.float32(0.06)
    idx = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), seq)
    w[idx, np.arange(n)] += rng.uniform(0.75, 1.0, n).astype(np.float32)
    p = np.zeros((6, n), np.float32)
    p[:4] = w / w.sum(0, keepdims=True)
    return p


def revcomp(p):
    return np.ascontiguousarray(np.stack([p[3, ::-1], p[2, ::-1], p[1, ::-1], p[0, ::-1], p[4, ::-1], p[5, ::-1]]))


def onehot(seq):
    p = np.zeros((6, len(seq)), np.float32)
    p[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), seq), np.arange(len(seq))] = 1.0
    return p


def build_groups(G, K, ref_len=3000, tlen=1000, seed=47):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    groups, refs = [], []
    for g in range(G):
        region = lut[rng.integers(0, 4, size=ref_len)]
        traces = []
        for i in range(K):
            start = int(i * (ref_len - tlen) / max(K - 1, 1))
            seq = region[start:start + tlen].copy()
            hit = rng.random(tlen) < 0.01
            seq[hit] = lut[rng.integers(0, 4, size=int(hit.sum()))]
            p = profile_of(rng, seq)
            traces.append(revcomp(p) if i % 3 == 1 else p)
        groups.append(traces)
        refs.append(onehot(region))
    return groups, refs


def cons_row(p, ops, skip):
    """_profileConsChar of a profile along forward-order ops: '-' where the op is `skip`"""
    chars = LETTERS[np.argmax(p, axis=0)]  # (the first maximum)
    take = ops != skip
    row = np.full(len(ops), ord("-"), np.uint8)
    row[take] = chars[:int(take.sum())]
    return row


def per_group_path(ctx, msalib, traces, pref):
    """one group as the one-group command runs it: assemble_cli.inc, reference-guided branch"""
    K = len(traces)
    revs = [revcomp(p) for p in traces]
    both = [x for pair in zip(traces, revs) for x in pair]
    gs = ctx.score(both, [pref], SEMI, idx1=np.arange(2 * K), idx2=np.zeros(2 * K, np.uint32))
    order = []
    for i in range(K):
        gf, gr = int(gs[2 * i]), int(gs[2 * i + 1])
        size = float(traces[i].shape[1])
        thr = size * float(np.float32(FRACMATCH)) * SCORE[0] + size * float(np.float32(1) - np.float32(FRACMATCH)) * SCORE[1]
        if gf > thr or gr > thr:
            order.append((-max(gf, gr), i, gf >= gr))
    order.sort()
    if not order:
        return dict(rows=[], gapped=b"", cons=b"", qual=b"")
    chosen = [traces[i] if f else revs[i] for _, i, f in order]
    _, btr = ctx.align([chosen[0]], [pref], SEMI)
    ops = np.frombuffer(btr[0], np.uint8)[::-1]
    align = np.stack([cons_row(chosen[0], ops, ord("h")), cons_row(pref, ops, ord("v"))])
    for p in chosen[1:]:
        ap = np.ascontiguousarray(msalib.profile_of_alignment([r.tobytes() for r in align]))
        _, btr = ctx.align([p], [ap], SEMI)
        ops = np.frombuffer(btr[0], np.uint8)[::-1]
        take = ops != ord("v")
        comb = np.full((align.shape[0] + 1, len(ops)), ord("-"), np.uint8)
        comb[0] = cons_row(p, ops, ord("h"))
        comb[1:, take] = align
        align = comb
    rows = [r.tobytes() for r in align]
    gapped, cs, qs = msalib.consensus(rows, CALLED, True)
    return dict(rows=rows, gapped=gapped, cons=cs, qual=qs)


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
    groups, refs = build_groups(a.groups, a.traces)
    ctx = tracy_amd.Context(0)
    out = {"groups": a.groups, "traces_per_group": a.traces, "trace_len": 1000, "ref_len": 3000, "score": SCORE}
    call = lambda p, mem: capi._check(capi.lib().tracyhip_assemble_traces(ctx._h, capi.C.byref(p.job), capi.C.byref(p.prm), mem, capi.C.byref(p.out)))

    p = capi.PreparedAssemble(groups, refs, SCORE, FRACMATCH, CALLED, False)
    for _ in range(a.warmup):
        call(p, capi.MEM_HOST)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        call(p, capi.MEM_HOST)
    dt = (time.perf_counter() - t0) / a.steps
    stats = ctx.last_call_stats()
    out.update(host_groups_per_s=round(a.groups / dt, 1), host_ms=round(1e3 * dt, 3), chunks=stats["asm_chunks"], chain_steps=stats["asm_steps"],
               host_syncs=stats["host_syncs"])
    got = p.results()
    out["matching_traces"] = int((got["rank"] != 0xffffffff).sum())

    q = capi.PreparedAssemble(groups, refs, SCORE, FRACMATCH, CALLED, False)
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
    same = all(np.array_equal(got[k], gotd[k]) for k in ("score_fwd", "score_rev", "forward", "rank", "nrows", "ncol", "cons_len")) and \
        all(got[k] == gotd[k] for k in ("rows", "gapped", "cons", "qual"))
    out["mem_device_identical"] = bool(same)

    # the per-group path: every group once (after one untimed group that warms its kernels up)
    per_group_path(ctx, msalib, groups[0], refs[0])
    t0 = time.perf_counter()
    base = [per_group_path(ctx, msalib, t, r) for t, r in zip(groups, refs)]
    dt = time.perf_counter() - t0
    out.update(per_group_groups_per_s=round(a.groups / dt, 1), per_group_ms=round(1e3 * dt, 3),
               speedup_host=round(dt / (1e-3 * out["host_ms"]), 2), speedup_device=round(dt / (1e-3 * out["device_ms"]), 2))
    ctx.close()
    idx = np.linspace(0, a.groups - 1, min(a.check, a.groups)).astype(int).tolist()
    mism = sum(int(any(got[k][g] != base[g][k] for k in ("rows", "gapped", "cons", "qual"))) for g in idx)
    out.update(checked=len(idx), mismatches=mism)
    print(json.dumps(out))
    return 0 if mism == 0 and same else 1


if __name__ == "__main__":
    sys.exit(main())
