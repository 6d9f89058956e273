"""What per-trace trims buy a batch that was trimmed by quality, one JSON line: N synthetic traces whose ends are of uneven quality (so
that trimTrace at stringency 2 gives them different pairs), aligned on one context (a) by ONE tracyhip_align_traces call with
trim_left_each / trim_right_each and (b) the former way, one call with scalar trims per distinct pair.  Host buffers, structs prepared
before the clock starts; a step ends when its last call has returned (each call ends in a device synchronisation).  The results of both
ways are compared.

    python tools/trims_each_line.py [--traces 10000] [--bases 1000] [--window 4000] [--steps 5] [--warmup 1] [--threads 16]
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
KEYS = ("forward", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final", "ops_len")


def uneven_batch(nt, mf, window, threads, chunk=1000):
    """profiles, references and trimTrace's pair of every trace; the chromatograms go chunk by chunk (1.9 GB per 10 000 traces at once)"""
    from tracy_amd import hostlib
    rng = np.random.default_rng(12)
    profs, refs, trims = [], [], []
    for lo in range(0, nt, chunk):
        k = min(chunk, nt - lo)
        d = hostlib.synth_decompose_batch(9000 + lo, k, window, mf, threads, mix=0)
        sig = d["signal"]
        for t in range(k):  # a second peak at 0.7 of the first under the leading a and the trailing b bases
            a, b = int(rng.choice([0, 10, 25, 45, 70, 100])), int(rng.choice([0, 15, 30, 60, 90]))
            for sl in (slice(0, 12 * a), slice(sig.shape[2] - 12 * b, sig.shape[2])):
                sig[t, :, sl] = np.maximum(sig[t, :, sl], (0.7 * np.roll(sig[t, :, sl], 1, axis=0)).astype(sig.dtype))
        pos = np.tile(np.arange(mf, dtype=np.int32) * 12 + 6, (k, 1))
        _, got = hostlib.basecall_batch(sig, pos, 0.33, 2.0, threads)
        for t in range(k):
            n = int(got["bc_len"][t])
            profs.append(np.ascontiguousarray(got["profiles"][t, :6 * n].reshape(6, n)))
            refs.append(d["refs"][t].tobytes())
            trims.append((int(got["trims"][t][0]) & 0xFFFF, int(got["trims"][t][1]) & 0xFFFF))
    return profs, refs, np.array(trims, np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=10000)
    ap.add_argument("--bases", type=int, default=1000)
    ap.add_argument("--window", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    a = ap.parse_args()

    import tracy_amd
    from tracy_amd import capi
    profs, refs, trims = uneven_batch(a.traces, a.bases, a.window, a.threads)
    nt = len(profs)
    groups = {}
    for i, p in enumerate(map(tuple, trims.tolist())):
        groups.setdefault(p, []).append(i)
    ctx = tracy_amd.Context(0)
    lib = capi.lib()

    def call(p):
        capi._check(lib.tracyhip_align_traces(ctx._h, C.byref(p.job), C.byref(p.prm), capi.MEM_HOST, C.byref(p.out)))

    one = capi.PreparedAlign(profs, refs, SCORE, trims[:, 0], trims[:, 1])
    per_pair = [(idx, capi.PreparedAlign([profs[i] for i in idx], [refs[i] for i in idx], SCORE, l, r)) for (l, r), idx in groups.items()]

    def timed(fn):
        ts = []
        for s in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if s >= a.warmup:
                ts.append(time.perf_counter() - t0)
        return ts

    ta = timed(lambda: call(one))
    stats = ctx.last_call_stats()
    tb = timed(lambda: [call(p) for _, p in per_pair])
    # the same answers either way
    ra = one.results()
    same = True
    for idx, p in per_pair:
        rb = p.results()
        same &= all(np.array_equal(np.asarray(ra[k])[idx], rb[k]) for k in KEYS) and [ra["btr"][i] for i in idx] == rb["btr"]
    ms_a, ms_b = 1e3 * float(np.median(ta)), 1e3 * float(np.median(tb))
    print(json.dumps(dict(tool="trims_each_line", traces=nt, bases=a.bases, window=a.window, stringency=2, distinct_pairs=len(groups),
                          largest_group=max(len(v) for v in groups.values()), steps=a.steps, warmup=a.warmup,
                          one_call_ms=round(ms_a, 3), one_call_step_ms=[round(1e3 * t, 3) for t in ta],
                          one_call_stream_ordered=int(stats["stream_ordered"]), one_call_fallback_traces=int(stats["fallback_traces"]),
                          per_pair_calls=len(per_pair), per_pair_ms=round(ms_b, 3), per_pair_step_ms=[round(1e3 * t, 3) for t in tb],
                          per_pair_over_one_call=round(ms_b / ms_a, 3), identical=bool(same), device=torch.cuda.get_device_name(0))))
    ctx.close()


if __name__ == "__main__":
    main()
