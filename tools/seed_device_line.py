"""Device k-mer seeding on configs[3]'s data (BASELINE configs[3]: 1 000 000 traces of 1 kb against a 50 Mb genome), one JSON line:
index upload (seconds, bytes), device seeding traces/s (tracyhip_seed_traces, windows left on the device), host seeding traces/s on the
same data (tracyhost_seed_batch on this rank's threads), the deferred count, how many traces were compared with host seeding and
whether all were bit-identical, and seed + extend traces/s with device seeding (windows kept on the device, tracyhip_align_traces with
`oriented` and MEM_DEVICE).  The data is built as tools/legs.py SeedExtendLeg builds it: seeded random genome, every other trace from
the reverse strand, 1 % substitutions.  Step times end in a device synchronisation; warm-up steps are not timed.

    python tools/seed_device_line.py [--traces 1000000] [--genome-mb 50] [--steps 3] [--warmup 1] [--extend-traces 125000]

The repeat workload (--repeat-copies N --repeat-unit L): the same genome with one dispersed exact family -- N copies of a random unit of
L bases (L >= 1000) written over it at random places -- and every trace drawn from inside the unit, so no trace has a unique k-mer and
each casts ~N votes per window in the second pass.  With --spill the context runs with the option seed_spill and such traces are
answered on the device; without it they are deferred and seeded on the host inside the timed call.  Every line has n_deferred, n_spilled and
the spill launches of the last call; the repeat workload leaves the extend part out.

    python tools/seed_device_line.py --traces 100000 --repeat-copies 30 --repeat-unit 2000 --spill
"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

from legs import SCORE, rank_threads  # noqa: E402


def build_data(total, genome_mb, mf=1000, block=62500):
    """genome text and the packed consensus of every trace (SeedExtendLeg's recipe, rank 0 of one)"""
    rng = np.random.default_rng(22)
    n = int(genome_mb * 1e6)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seq = lut[rng.integers(0, 4, size=n, dtype=np.uint8)]
    starts = rng.integers(0, n - mf - 50, size=total)
    errs = np.random.default_rng(23)
    comp = np.array([3, 2, 1, 0], dtype=np.uint8)
    lut_inv = np.zeros(256, np.uint8)
    lut_inv[lut] = np.arange(4, dtype=np.uint8)
    blob = np.empty(total * mf + 1, np.uint8)
    blob[-1] = 0
    codes = []  # kept for the profiles of the extend part
    win = np.arange(mf, dtype=np.int64)
    for lo in range(0, total, block):
        hi = min(total, lo + block)
        c = lut_inv[seq[starts[lo:hi, None].astype(np.int64) + win[None, :]]]
        odd = (np.arange(lo, hi) % 2).astype(bool)
        c[odd] = comp[c[odd][:, ::-1]]
        flip = errs.random((hi - lo, mf)) < 0.01
        c = np.where(flip, (c + 1) % 4, c).astype(np.uint8)
        blob[lo * mf:hi * mf] = lut[c].reshape(-1)
        codes.append(c)
    packed = dict(n=total, blob=blob.tobytes(), offs=np.arange(total, dtype=np.uint64) * np.uint64(mf), lens=np.full(total, mf, np.uint32))
    return seq.tobytes(), packed, codes


def build_repeat_data(total, genome_mb, copies, unit, mf=1000):
    """a random genome with `copies` exact copies of one random unit of `unit` bases at random places that do not touch each other, and
    the packed consensus of traces drawn from inside the unit: every other one from the reverse strand, 1 % substitutions"""
    rng = np.random.default_rng(24)
    n = int(genome_mb * 1e6)
    if unit < mf or copies < 1 or copies * 2 * unit > n:
        raise SystemExit("--repeat-unit must be at least %d and the copies must fit the genome" % mf)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = rng.integers(0, 4, size=n, dtype=np.uint8)
    fam = rng.integers(0, 4, size=unit, dtype=np.uint8)
    cells = rng.choice(n // (2 * unit), size=copies, replace=False)  # one copy per cell of 2 x unit bases: apart from each other
    for cell in cells:
        at = int(cell) * 2 * unit + int(rng.integers(0, unit))
        codes[at:at + unit] = fam
    starts = rng.integers(0, unit - mf + 1, size=total)
    c = fam[starts[:, None].astype(np.int64) + np.arange(mf, dtype=np.int64)[None, :]]
    odd = (np.arange(total) % 2).astype(bool)
    c[odd] = (3 - c[odd])[:, ::-1]
    flip = np.random.default_rng(25).random(c.shape) < 0.01
    c = np.where(flip, (c + 1) % 4, c).astype(np.uint8)
    packed = dict(n=total, blob=lut[c].tobytes() + b"\0", offs=np.arange(total, dtype=np.uint64) * np.uint64(mf), lens=np.full(total, mf, np.uint32))
    return lut[codes].tobytes(), packed, None


def sub_pack(packed, lo, hi, mf=1000):
    return dict(n=hi - lo, blob=packed["blob"][lo * mf:hi * mf] + b"\0", offs=np.arange(hi - lo, dtype=np.uint64) * np.uint64(mf),
                lens=np.full(hi - lo, mf, np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=1000000)
    ap.add_argument("--genome-mb", type=float, default=50.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--extend-traces", type=int, default=125000)
    ap.add_argument("--no-host", action="store_true", help="skip host seeding (and the comparison)")
    ap.add_argument("--repeat-copies", type=int, default=0, help="the repeat workload: copies of one dispersed exact family (0: the random genome)")
    ap.add_argument("--repeat-unit", type=int, default=2000, help="... bases of its unit; the traces are drawn from inside it")
    ap.add_argument("--spill", action="store_true", help="run with the option seed_spill: traces over the LDS vote lists are answered on the device")
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi, hostlib
    threads = rank_threads(1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t0 = time.perf_counter()
    if a.repeat_copies:
        text, packed, codes = build_repeat_data(a.traces, a.genome_mb, a.repeat_copies, a.repeat_unit)
    else:
        text, packed, codes = build_data(a.traces, a.genome_mb)
    data_s = time.perf_counter() - t0
    tmp = tempfile.mkdtemp(prefix="tracy_seed_line_")
    out = dict(metric="seed_device_line", traces=a.traces, genome_mb=a.genome_mb, trace_len=1000, host_threads=threads, seed_spill=int(a.spill))
    if a.repeat_copies:
        out.update(repeat_copies=a.repeat_copies, repeat_unit=a.repeat_unit)
    try:
        gpath = os.path.join(tmp, "genome.fa")
        with open(gpath, "wb") as f:
            f.write(b">chrSyn\n" + text + b"\n")
        t0 = time.perf_counter()
        g = hostlib.Genome(gpath, 15, threads)
        out["index_build_s"] = round(time.perf_counter() - t0, 3)
        ctx = tracy_amd.Context(0)
        ctx.set_option("seed_spill", 1 if a.spill else 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dg = g.to_device(ctx)
        torch.cuda.synchronize()
        out["index_upload_s"] = round(time.perf_counter() - t0, 3)
        out["index_upload_bytes"] = dg.bytes
        # device seeding: the consensus to the device, the kernel, metadata back; windows stay on the device
        sd, times = None, []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sd = dg.seed_packed(packed, 50, 50, 3, 1000, threads, out=sd, mem=capi.MEM_DEVICE)
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(time.perf_counter() - t0)
        out["device_seed_s"] = [round(x, 4) for x in times]
        out["device_seed_traces_per_s"] = round(a.traces / float(np.median(times)), 1)
        out["deferred"] = out["n_deferred"] = int(sd["n_deferred"])
        out["n_spilled"] = int(sd["n_spilled"])
        out["seed_spill_launches"] = ctx.last_call_stats()["seed_spill_launches"]
        out["anchored"] = int((sd["status"][:a.traces] == 1).sum())
        if not a.no_host:
            t0 = time.perf_counter()
            hs = g.seed_packed(packed, 50, 50, 3, 1000, threads)
            hs_s = time.perf_counter() - t0
            out["host_seed_traces_per_s"] = round(a.traces / hs_s, 1)
            same = all(np.array_equal(sd[k][:a.traces], hs[k][:a.traces]) for k in ("status", "forward", "kmersupport", "pos", "contig", "slice_len"))
            B = 50000
            for lo in range(0, a.traces, B):  # window bytes (both buffers were zero past slice_len)
                hi = min(a.traces, lo + B)
                same = same and np.array_equal(sd["slices_2d"][lo:hi].cpu().numpy(), hs["slices_2d"][lo:hi])
            out["compared_with_host"] = a.traces
            out["bit_identical"] = bool(same)
            out["device_over_host"] = round(out["device_seed_traces_per_s"] / out["host_seed_traces_per_s"], 2)
            del hs
        del sd
        # seed + extend: device seeding (MEM_DEVICE) -> tracyhip_align_traces(oriented, MEM_DEVICE), block by block
        E = 0 if a.repeat_copies else min(a.extend_traces, a.traces)
        if E > 0:
            blocks = [(lo, min(E, lo + 62500)) for lo in range(0, E, 62500)]
            packs = [sub_pack(packed, lo, hi) for lo, hi in blocks]
            profs = []
            for lo, hi in blocks:
                c = codes[lo // 62500][:hi - lo]  # (build_data's blocks are these blocks)
                pr = np.full((hi - lo, 6, 1000), 0.0, np.float32)
                pr[:, :4, :] = 0.02
                for code in range(4):
                    pr[:, code, :][c == code] = 0.94
                profs.append(pr)
            outs = [None] * len(blocks)
            ext_times = []
            for it in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b, (lo, hi) in enumerate(blocks):
                    s = outs[b] = dg.seed_packed(packs[b], 50, 50, 3, 1000, threads, out=outs[b], mem=capi.MEM_DEVICE)
                    ok = np.nonzero(s["status"][:hi - lo] == 1)[0]
                    cap = s["slices_2d"].shape[1]
                    pp = capi.PackedSeqs([], capi.SEQ_PROFILE)
                    pp.count, pp.data = len(ok), profs[b]
                    pp.offset = ok.astype(np.uint64) * np.uint64(6 * 1000)
                    pp.length = np.full(max(len(ok), 1), 1000, np.uint32)
                    pw = capi.PackedSeqs([], capi.SEQ_CHAR)
                    pw.count = len(ok)
                    pw.offset = ok.astype(np.uint64) * np.uint64(cap)
                    pw.length = np.ascontiguousarray(s["slice_len"][ok], dtype=np.uint32)
                    prep = capi.PreparedAlign(pp, pw, SCORE, 50, 50, oriented=np.ascontiguousarray(s["forward"][ok], dtype=np.uint8))
                    dprof = torch.from_numpy(profs[b]).to(dev)
                    prep.job.profiles = pp.seqset(dprof.data_ptr())
                    prep.job.refs = pw.seqset(s["slices_2d"].data_ptr())
                    dres = {k: torch.empty(v.shape, dtype=torch.int32 if str(v.dtype) == "uint32" else getattr(torch, str(v.dtype)), device=dev)
                            for k, v in prep.res.items()}
                    for k, v in dres.items():
                        setattr(prep.out, k, v.data_ptr())
                    capi._check(capi.lib().tracyhip_align_traces(ctx._h, C.byref(prep.job), C.byref(prep.prm), capi.MEM_DEVICE, C.byref(prep.out)))
                torch.cuda.synchronize()
                if it >= a.warmup:
                    ext_times.append(time.perf_counter() - t0)
            out["seed_extend_traces"] = E
            out["seed_extend_s"] = [round(x, 4) for x in ext_times]
            out["seed_extend_traces_per_s"] = round(E / float(np.median(ext_times)), 1)
        out["data_build_s"] = round(data_s, 2)
        dg.close()
        g.close()
        ctx.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
