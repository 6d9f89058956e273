"""The genome k-mer index built on the device (tracyhip_genome_build) against the host's in-memory build (GenomeIndex::build), one JSON
line: genome size, ntab, the largest bucket; host build seconds on this rank's threads (FASTA load reported apart); device build seconds
(text upload included, the call ends in a synchronisation; warm-up builds not timed); copy-back seconds (tracyhip_genome_download);
`identical` (directory and table compared in full); and how many of N seeded traces (tracyhip_seed_traces) answer the same on the
device-built index as host seeding on the host-built one, window bytes included.

Default data: configs[3]'s recipe (tools/seed_device_line.py build_data: a 50 Mb seeded random genome, traces of 1 kb with 1 %
substitutions, every other one reverse-complemented).  --genome-mb 1000 (or more) adds a 1 Mb poly-A run and a 2 Mb tandem-repeat block
(a 171-bp unit) to the random text.  Where the host build is skipped (--no-host; the default above --host-max-mb) the line checks
device-only invariants instead: dir monotone and ending at ntab, the table in the host's order, ntab = the valid windows, and the code of a
sample of entries at their positions.

    python tools/index_device_line.py [--genome-mb 50] [--kmer 15] [--steps 3] [--warmup 1] [--traces 10000] [--no-host]
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

from legs import rank_threads  # noqa: E402
from seed_device_line import build_data  # noqa: E402

FIELDS = ("status", "forward", "kmersupport", "pos", "contig", "slice_len")


def large_text(genome_mb):
    """a random genome of genome_mb Mb with a 1 Mb poly-A run and a 2 Mb tandem-repeat block (171-bp unit) written into it"""
    rng = np.random.default_rng(31)
    n = int(genome_mb * 1e6)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seq = np.empty(n, np.uint8)
    B = 1 << 27
    for lo in range(0, n, B):
        seq[lo:min(n, lo + B)] = lut[rng.integers(0, 4, size=min(n, lo + B) - lo, dtype=np.uint8)]
    a0 = n // 3
    seq[a0:a0 + 1000000] = ord("A")
    unit = lut[rng.integers(0, 4, size=171, dtype=np.uint8)]
    t0 = 2 * n // 3
    seq[t0:t0 + 171 * 11696] = np.tile(unit, 11696)
    return seq


def text_desc(text_nl, k, bits):
    """a build descriptor over one contig: text_nl = the contig + '\\n' (uint8)"""
    from tracy_amd import capi
    starts = np.zeros(1, np.uint64)
    lengths = np.array([len(text_nl) - 1], np.uint32)
    d = capi.GenomeDesc()
    d.k, d.bucket_bits, d.dir, d.tab, d.ntab = k, bits, None, None, 0
    d.text, d.text_len, d.ncontigs = text_nl.ctypes.data, len(text_nl), 1
    d.starts, d.lengths, d.contig_id = starts.ctypes.data, lengths.ctypes.data, None
    return d, (starts, lengths)


def valid_windows(text_nl, k):
    """windows of k letters from ACGT: from the runs between other bytes"""
    code = np.frombuffer(b"ACGT", np.uint8)
    bad = np.nonzero(~np.isin(text_nl, code))[0]
    edges = np.concatenate([[-1], bad, [len(text_nl)]]).astype(np.int64)
    runs = np.diff(edges) - 1
    return int(np.maximum(runs - k + 1, 0).sum())


def check_invariants(text_nl, k, bits, dirs, tab, sample=200000):
    """device-only checks of a table: dir monotone from 0 to ntab, the host's order (slot, code, pos), ntab = the valid windows, and the
    codes of a sample of entries recomputed from the text"""
    ntab = len(tab)
    res = dict(dir_monotone_to_ntab=bool(dirs[0] == 0 and dirs[-1] == ntab and np.all(dirs[1:] >= dirs[:-1])))
    mask = np.uint64((1 << bits) - 1)
    ordered = True
    B = 1 << 26
    for lo in range(0, max(ntab - 1, 0), B):
        hi = min(ntab, lo + B + 1)
        c, p = tab[lo:hi, 0], tab[lo:hi, 1]
        s = c & mask
        ds, dc, dp = s[1:] > s[:-1], c[1:] > c[:-1], p[1:] > p[:-1]
        es, ec = s[1:] == s[:-1], c[1:] == c[:-1]
        ordered = ordered and bool(np.all(ds | (es & (dc | (ec & dp)))))
        # the directory names every entry's bucket
        idx = np.arange(lo, hi, dtype=np.uint64)
        ordered = ordered and bool(np.all((dirs[s.astype(np.int64)] <= idx) & (idx < dirs[s.astype(np.int64) + 1])))
    res["table_in_host_order"] = ordered
    res["ntab_is_valid_windows"] = ntab == valid_windows(text_nl, k)
    rng = np.random.default_rng(5)
    pick = rng.integers(0, ntab, size=min(sample, ntab)) if ntab else np.zeros(0, np.int64)
    lut = np.full(256, 0, np.uint64)
    lut[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint64)
    pos = (tab[pick, 1] & np.uint64((1 << 63) - 1)).astype(np.int64)
    flip = (tab[pick, 1] >> np.uint64(63)).astype(bool)
    code = np.zeros(len(pick), np.uint64)
    rc = np.zeros(len(pick), np.uint64)
    for j in range(k):
        x = lut[text_nl[pos + j]]
        code = (code << np.uint64(2)) | x
        rc = rc | ((np.uint64(3) - x) << np.uint64(2 * j))
    key = np.where(rc < code, rc, code)
    res["sampled_codes_right"] = bool(np.array_equal(key, tab[pick, 0]) and np.array_equal(flip, rc < code))
    res["sampled"] = int(len(pick))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=float, default=50.0)
    ap.add_argument("--kmer", type=int, default=15)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--traces", type=int, default=10000, help="traces seeded on both indexes and compared")
    ap.add_argument("--no-host", action="store_true", help="skip the host build: device-only invariants")
    ap.add_argument("--host-max-mb", type=float, default=200.0, help="largest genome the host build runs on unless --host")
    ap.add_argument("--host", action="store_true", help="run the host build at any size")
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi, hostlib
    threads = rank_threads(1)
    torch.cuda.set_device(0)
    k = a.kmer
    bits = hostlib.default_bucket_bits(k)
    large = a.genome_mb >= 1000
    host = not a.no_host and (a.host or a.genome_mb <= a.host_max_mb)
    t0 = time.perf_counter()
    if large:
        seq = large_text(a.genome_mb)
        packed = None
    else:
        text, packed, _ = build_data(a.traces, a.genome_mb)
        seq = np.frombuffer(text, np.uint8)
    text_nl = np.empty(len(seq) + 1, np.uint8)
    text_nl[:-1] = seq
    text_nl[-1] = ord("\n")
    del seq
    out = dict(metric="index_device_line", genome_mb=a.genome_mb, genome_bytes=int(len(text_nl) - 1), kmer=k, bucket_bits=bits,
               host_threads=threads, data_build_s=round(time.perf_counter() - t0, 2))
    if large:
        out["injected"] = "1 Mb poly-A, 2 Mb tandem repeat (171-bp unit)"
    ctx = tracy_amd.Context(0)
    desc, keep = text_desc(text_nl, k, bits)
    # device build: upload + build, synchronised inside the call; the handle of the last step is kept
    times, dh = [], None
    for it in range(a.warmup + a.steps):
        if dh is not None:
            capi.genome_free(dh)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dh = capi.genome_build(ctx, desc)
        t1 = time.perf_counter()
        if it >= a.warmup:
            times.append(t1 - t0)
    out["device_build_s"] = [round(x, 4) for x in times]
    out["device_build_median_s"] = round(float(np.median(times)), 4)
    out["device_bytes"] = capi.genome_bytes(dh)
    t0 = time.perf_counter()
    ddir, dtab = capi.genome_download(dh, bits)
    out["copy_back_s"] = round(time.perf_counter() - t0, 3)
    out["ntab"] = int(len(dtab))
    out["largest_bucket"] = int(np.diff(ddir).max()) if len(ddir) > 1 else 0
    tmp = tempfile.mkdtemp(prefix="tracy_index_line_")
    try:
        if host:
            gpath = os.path.join(tmp, "genome.fa")
            with open(gpath, "wb") as f:
                f.write(b">chrSyn\n")
                f.write(text_nl.tobytes())
            fn = hostlib.lib().tracyhost_genome_load
            fn.restype = C.c_void_p
            t0 = time.perf_counter()
            hl = fn(gpath.encode())
            load_s = time.perf_counter() - t0
            hostlib.lib().tracyhost_genome_free(C.c_void_p(hl))
            t0 = time.perf_counter()
            g = hostlib.Genome(gpath, k, threads)
            open_s = time.perf_counter() - t0
            out["host_load_s"] = round(load_s, 3)
            out["host_build_s"] = round(open_s - load_s, 3)
            out["device_over_host"] = round((open_s - load_s) / out["device_build_median_s"], 1)
            v = g.view()
            out["identical"] = bool(v["bucket_bits"] == bits and np.array_equal(v["dir"], ddir) and np.array_equal(v["tab"], dtab))
            del v
            if packed is not None and a.traces:
                # seeding on the device-built index (deferred traces: host seeding on the host-built table) vs host seeding on the host build
                dg = hostlib.DeviceGenome.wrap(g, ctx, dh)
                dh = None
                sd = dg.seed_packed(packed, 50, 50, 3, 1000, threads)
                hs = g.seed_packed(packed, 50, 50, 3, 1000, threads)
                n = a.traces
                same = np.ones(n, bool)
                for key in ("status", "slice_len"):
                    same &= sd[key][:n] == hs[key][:n]
                anch = hs["status"][:n] == 1
                for key in FIELDS:
                    same &= ~anch | (sd[key][:n] == hs[key][:n])
                same &= np.all(sd["slices_2d"][:n] == hs["slices_2d"][:n], axis=1)
                out["seeded_traces"] = n
                out["seeded_matched"] = int(same.sum())
                out["seeded_deferred"] = int(sd["n_deferred"])
                dg.close()
            g.close()
        else:
            out["host_build_s"] = None
            out["identical"] = None
            t0 = time.perf_counter()
            out["invariants"] = check_invariants(text_nl, k, bits, ddir, dtab)
            out["invariants_s"] = round(time.perf_counter() - t0, 2)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        if dh is not None:
            capi.genome_free(dh)
        ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
