"""The variant lists of a `tracy decompose` batch on the device (tracyhip_decompose_variants), one JSON line.  The data is the configs[2]
workload of bench.py (tools/legs.py DecomposeLeg: heterozygous 1 kb traces against 3 kb windows, both strands); tracyhip_decompose_traces
runs once, then the variants call is timed on its results

  - with payloads and results in device memory (MEM_DEVICE), and
  - with host buffers (MEM_HOST: strings and tables staged in, the used records and text packed on the device and copied back),

with the wall time of the call's stages (option `verbose`: plan, re-alignments of the reverse traces, rows + scan, results) and the
bytes of the variant payload against the bytes of the full decompose result.  A sample of traces is compared field by field with the
oracle chain (tests/indigo_oracle.py call_variants over rows the oracle builds; reverse traces re-aligned by the oracle's gotoh).

In the same run, on the same arrays, the path the command line took before the call existed and still takes for truncated traces
(tracy_amd_cli.cpp call_variants): the rows of the forward traces' allele alignments expanded on the device and copied back, the reverse
traces' alleles and slices reverse-complemented on the host, uploaded through tracyhip_gotoh_align, their rows copied back, then
callVariants + stable_sort on 16 host threads (tracy_amd/host: tracyhost_revcomp_batch, tracyhost_call_variants_batch).  Every trace of
the batch is compared between the two, field by field.

    python tools/variants_device_line.py [--traces 100000] [--steps 3] [--warmup 1] [--check 48] [--threads 16]
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
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (before the library: torch's HIP runtime is the one that sees the devices)

SCORE = (3, -5, -10, -4)
TRIMS = (50, 50)
MAXV, MAXT = 256, 4096


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
    line = [ln for ln in text.splitlines() if ln.startswith("tracyhip_decompose_variants:")]
    return {k: float(v) for k, v in re.findall(r"(\w+_ms|called|reverse|truncated|chunks|host_syncs) ([0-9.]+)", line[-1])} if line else {}


def host_copy(leg, capi):
    """the leg's job and decompose result on host arrays (the payloads the variants call reads), and what keeps them alive"""
    keep = {}

    def h(name, t):
        keep[name] = np.ascontiguousarray(t.cpu().numpy()).reshape(-1)  # (primary and references are [nt][len] tensors: one flat payload each)
        return keep[name].ctypes.data
    job = capi.DecomposeJob()
    C.memmove(C.byref(job), C.byref(leg.job), C.sizeof(job))
    job.bc.primary = h("pri", leg.t_pri)
    job.bc.secondary = h("sec", leg.t_sec)
    job.refs.data = h("refs", leg.t_ref)
    res = capi.DecomposeResult()
    C.memmove(C.byref(res), C.byref(leg.out), C.sizeof(res))
    for name in ("status", "forward", "secdecomp"):
        setattr(res, name, h(name, leg.res[name]))
    for k in range(2):
        for nm in ("slice_begin", "slice_len", "ref_pos"):
            getattr(res, nm)[k] = h("%s%d" % (nm, k), leg.res["%s%d" % (nm, k)])
        res.ops[k] = h("ops%d" % k, leg.keep[k][1])
        res.ops_len[k] = h("olen%d" % k, leg.keep[k][2])
    return job, res, keep


def oracle_list(keep, leg, t, slice_pos):
    import indigo_oracle as io
    import pyoracle as orc
    from sage_oracle import revcomp
    mf, n = leg.mf, leg.n
    forward = bool(keep["forward"][t])
    ref = keep["refs"][t * n:(t + 1) * n].tobytes()
    refslice = ref if forward else revcomp(ref)
    var = []
    for k, name in enumerate(("pri", "secdecomp")):
        seq = io.trimmed_seq(keep[name][t * mf:(t + 1) * mf].tobytes(), *TRIMS)
        sb, sl = int(keep["slice_begin%d" % k][t]), int(keep["slice_len%d" % k][t])
        s = refslice[sb:sb + sl]
        if forward:
            off = int(leg.keep[k][0][t])
            r0, r1 = orc.create_alignment_str(keep["ops%d" % k][off:off + int(keep["olen%d" % k][t])].tobytes(), seq, s)
        else:
            rseq, rs = revcomp(seq), revcomp(s)
            _, btr = orc.gotoh_str(rseq, rs, 1, 0, SCORE)
            r0, r1 = orc.create_alignment_str(btr, rseq, rs)
        io.call_variants(r0, r1, "chr", slice_pos + int(keep["ref_pos%d" % k][t]), var)
    io.sort_variants(var)
    return [dict(pos=v["pos"], basenum=v["basenum"], gt=v["gt"], ref=v["ref"].encode(), alt=v["alt"].encode(),
                 call_index=(TRIMS[0] + v["basenum"] - 1) if forward else mf - (TRIMS[1] + v["basenum"])) for v in var]


def present_path(ctx, keep, leg, sp, threads, buf):
    """tracy_amd_cli.cpp call_variants on the batch's arrays; returns the seconds of its timed part (everything but laying out index arrays)"""
    from tracy_amd import capi, hostlib
    lib, hl = capi.lib(), hostlib.lib()
    nt, mf, n = leg.nt, leg.mf, leg.n
    m = mf - TRIMS[0] - TRIMS[1]
    u8p, vp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))), (lambda a: C.c_void_p(a.ctypes.data))
    ok = keep["status"] == 0
    fw = np.flatnonzero(ok & (keep["forward"] != 0)).astype(np.uint64)
    rv = np.flatnonzero(ok & (keep["forward"] == 0)).astype(np.uint64)
    cap = [int(leg.keep[k][4]) for k in range(2)]
    region = [0, nt * cap[0], nt * (cap[0] + cap[1])]  # rows of allele 1 | allele 2 | the re-alignments, in one buffer per row
    sb = [keep["slice_begin%d" % k].astype(np.uint64) for k in range(2)]
    sl = [keep["slice_len%d" % k].astype(np.uint32) for k in range(2)]
    nr = len(rv)
    # the reverse traces' strings: [allele 1, allele 2] x trace, and the oriented slices the command holds in rs1 / rs2 (made here, untimed)
    rl1 = np.full(2 * nr, m, np.uint32)
    rl2 = np.stack([sl[0][rv], sl[1][rv]], 1).reshape(-1).astype(np.uint32)
    ro1 = np.arange(2 * nr, dtype=np.uint64) * np.uint64(m)
    ro2 = np.concatenate([[0], np.cumsum(rl2.astype(np.uint64))[:-1]]).astype(np.uint64) if nr else np.zeros(0, np.uint64)
    src_seq = [(rv * np.uint64(mf) + np.uint64(TRIMS[0])).astype(np.uint64)] * 2
    osl = np.zeros(max(int(rl2.sum()), 1), np.uint8)
    if nr:  # oriented = revcomp(reference); its slice [sb, sb + sl) is the reverse complement of reference[n - sb - sl, n - sb)
        src = np.stack([rv * np.uint64(n) + np.uint64(n) - sb[k][rv] - sl[k][rv].astype(np.uint64) for k in range(2)], 1).reshape(-1).astype(np.uint64)
        assert hl.tracyhost_revcomp_batch(vp(keep["refs"]), capi._u64p(src), capi._u32p(rl2), C.c_uint32(2 * nr), vp(osl), capi._u64p(ro2), C.c_uint32(threads)) == 0
    rcap = (rl1.astype(np.uint64) + rl2.astype(np.uint64))
    roff = np.concatenate([[0], np.cumsum(rcap)[:-1]]).astype(np.uint64) if nr else np.zeros(0, np.uint64)
    rtot = int(rcap.sum())
    rows = [np.zeros(region[2] + max(rtot, 1), np.uint8) for _ in range(2)]
    rseq, rsl = np.zeros(max(2 * nr * m, 1), np.uint8), np.zeros(max(int(rl2.sum()), 1), np.uint8)
    rops, rolen = np.zeros(max(rtot, 1), np.uint8), np.zeros(max(2 * nr, 1), np.uint32)
    prm = capi.Params(SCORE[0], SCORE[1], SCORE[2], SCORE[3], 1, 0)
    t0 = time.perf_counter()
    # forward traces: rows from the op strings the decompose call returned, copied back
    for k, name in enumerate(("pri", "secdecomp")):
        if not len(fw):
            break
        o1 = (fw * np.uint64(mf) + np.uint64(TRIMS[0])).astype(np.uint64)
        l1 = np.full(len(fw), m, np.uint32)
        o2 = (fw * np.uint64(n) + sb[k][fw]).astype(np.uint64)
        l2 = np.ascontiguousarray(sl[k][fw])
        pr = capi.Pairs()
        pr.npairs = len(fw)
        pr.a1 = capi.SeqSet(capi.SEQ_CHAR, keep[name].ctypes.data, capi._u64p(o1), capi._u32p(l1), len(fw))
        pr.a2 = capi.SeqSet(capi.SEQ_CHAR, keep["refs"].ctypes.data, capi._u64p(o2), capi._u32p(l2), len(fw))
        oo = np.ascontiguousarray(leg.keep[k][0][fw.astype(np.int64)]).astype(np.uint64)
        ol = np.ascontiguousarray(keep["olen%d" % k][fw.astype(np.int64)]).astype(np.uint32)
        capi._check(lib.tracyhip_alignment_rows(ctx._h, C.byref(pr), capi.MEM_HOST, u8p(keep["ops%d" % k]), capi._u64p(oo), capi._u32p(ol),
                                                C.c_void_p(rows[0].ctypes.data + region[k]), C.c_void_p(rows[1].ctypes.data + region[k])))
    # reverse traces: reverse complements on the host threads, one upload through tracyhip_gotoh_align, rows copied back
    if nr:
        for k, name in enumerate(("pri", "secdecomp")):
            dst = np.ascontiguousarray(ro1[k::2])
            assert hl.tracyhost_revcomp_batch(vp(keep[name]), capi._u64p(src_seq[k]), capi._u32p(np.full(nr, m, np.uint32)), C.c_uint32(nr), vp(rseq),
                                              capi._u64p(dst), C.c_uint32(threads)) == 0
        assert hl.tracyhost_revcomp_batch(vp(osl), capi._u64p(ro2), capi._u32p(rl2), C.c_uint32(2 * nr), vp(rsl), capi._u64p(ro2), C.c_uint32(threads)) == 0
        pr = capi.Pairs()
        pr.npairs = 2 * nr
        pr.a1 = capi.SeqSet(capi.SEQ_CHAR, rseq.ctypes.data, capi._u64p(ro1), capi._u32p(rl1), 2 * nr)
        pr.a2 = capi.SeqSet(capi.SEQ_CHAR, rsl.ctypes.data, capi._u64p(ro2), capi._u32p(rl2), 2 * nr)
        capi._check(lib.tracyhip_gotoh_align(ctx._h, C.byref(pr), C.byref(prm), capi.MEM_HOST, None, u8p(rops), capi._u64p(roff), capi._u32p(rolen)))
        capi._check(lib.tracyhip_alignment_rows(ctx._h, C.byref(pr), capi.MEM_HOST, u8p(rops), capi._u64p(roff), capi._u32p(rolen),
                                                C.c_void_p(rows[0].ctypes.data + region[2]), C.c_void_p(rows[1].ctypes.data + region[2])))
    # callVariants of both alleles of every trace + stable_sort on the host threads
    off = np.zeros(2 * nt, np.uint64)
    ln = np.zeros(2 * nt, np.uint32)
    pos = np.zeros(2 * nt, np.int32)
    fi, ri = fw.astype(np.int64), rv.astype(np.int64)
    for k in range(2):
        off[2 * fi + k] = np.uint64(region[k]) + leg.keep[k][0][fi].astype(np.uint64)
        ln[2 * fi + k] = keep["olen%d" % k][fi]
        off[2 * ri + k] = np.uint64(region[2]) + roff[k::2]
        ln[2 * ri + k] = rolen[:2 * nr][k::2]
        pos[k::2] = sp.astype(np.int64) + keep["ref_pos%d" % k].astype(np.int64)
    bl = np.full(nt, mf, np.uint32)
    s = buf.struct
    assert hl.tracyhost_call_variants_batch(C.c_uint32(nt), vp(rows[0]), vp(rows[1]), capi._u64p(off), capi._u32p(ln), pos.ctypes.data_as(C.POINTER(C.c_int32)),
                                            u8p(np.ascontiguousarray(keep["forward"])), capi._u32p(bl), C.c_uint32(TRIMS[0]), C.c_uint32(TRIMS[1]),
                                            C.c_uint32(s.max_variants), C.c_uint32(s.max_text), C.c_void_p(s.var), C.c_void_p(s.text), C.c_void_p(s.var_n),
                                            C.c_void_p(s.var_flags), C.c_uint32(threads)) == 0
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=48, help="traces compared with the oracle chain")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the former path")
    a = ap.parse_args()
    from tracy_amd import capi
    from tools.legs import DecomposeLeg
    dev = torch.device("cuda", 0)
    leg = DecomposeLeg(a.traces, 3000, 1000, 0, 1, dev)
    leg.step()
    torch.cuda.synchronize()
    ctx, lib, nt = leg.ctx, capi.lib(), leg.nt
    sp = np.zeros(nt, np.uint32)
    out = {"traces": nt, "trace_len": leg.mf, "window_len": leg.n, "score": SCORE, "max_variants": MAXV, "max_text": MAXT}

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps

    bd = capi.VariantBuffers(nt, MAXV, MAXT, device=True)
    call_d = lambda: capi._check(lib.tracyhip_decompose_variants(ctx._h, C.byref(leg.job), C.byref(leg.out), capi._u32p(sp), C.byref(leg.prm),
                                                                 capi.MEM_DEVICE, C.byref(bd.struct)))
    dt = timed(call_d)
    st = ctx.last_call_stats()
    out.update(device_ms=round(1e3 * dt, 3), device_traces_per_s=round(nt / dt, 1), called=st["var_traces"], reverse=st["var_realigned"],
               truncated=st["var_truncated"], chunks=st["var_chunks"], host_syncs=st["host_syncs"])
    out["stage_ms"] = stage_line(ctx, call_d)
    if out["stage_ms"].get("realign_ms") is not None:
        total = sum(out["stage_ms"][k] for k in ("plan_ms", "realign_ms", "rows_scan_ms", "results_ms"))
        out["realign_share"] = round(out["stage_ms"]["realign_ms"] / total, 3) if total else None
    got_d, flags_d = bd.lists()

    job, res, keep = host_copy(leg, capi)
    bh = capi.VariantBuffers(nt, MAXV, MAXT)
    call_h = lambda: capi._check(lib.tracyhip_decompose_variants(ctx._h, C.byref(job), C.byref(res), capi._u32p(sp), C.byref(leg.prm), capi.MEM_HOST,
                                                                 C.byref(bh.struct)))
    dt = timed(call_h)
    out.update(host_ms=round(1e3 * dt, 3), host_traces_per_s=round(nt / dt, 1), host_syncs_host_buffers=ctx.last_call_stats()["host_syncs"])
    got_h, flags_h = bh.lists()
    out["mem_kinds_identical"] = bool(got_d == got_h and np.array_equal(flags_d, flags_h))

    # what a caller has to move: the records and text in use against everything tracyhip_decompose_traces returns for the batch
    nrec = sum(len(g) for g in got_d)
    text = sum(len(v["ref"]) + len(v["alt"]) for g in got_d for v in g)
    payload = 32 * nrec + text + 8 * nt
    full = sum(v.numel() * v.element_size() for v in leg.res.values()) + sum(k[1].numel() + 4 * k[2].numel() + 4 * k[3].numel() for k in leg.keep) + \
        2 * leg.t_pri.numel()
    out.update(variants=nrec, variant_payload_bytes=payload, full_result_bytes=full, result_bytes_ratio=round(full / max(payload, 1), 1))

    # the former path on the same arrays: once to warm its buffers up, once timed; every trace compared
    bp = capi.VariantBuffers(nt, MAXV, MAXT)
    present_path(ctx, keep, leg, sp, a.threads, bp)
    dt = present_path(ctx, keep, leg, sp, a.threads, bp)
    got_p, flags_p = bp.lists()
    differ = [t for t in range(nt) if got_p[t] != got_d[t] or int(flags_p[t]) != int(flags_d[t])]
    out.update(host_path_ms=round(1e3 * dt, 3), host_path_threads=a.threads, host_path_over_device=round(1e3 * dt / out["device_ms"], 2),
               host_path_over_host_buffers=round(1e3 * dt / out["host_ms"], 2), host_path_traces_differing=len(differ), host_path_first_differing=differ[:4])

    idx = np.linspace(0, nt - 1, min(a.check, nt)).astype(int).tolist()
    mism, seen, errors = 0, 0, []
    for t in idx:
        if int(keep["status"][t]) != 0:
            mism += int(got_d[t] != [])
            continue
        seen += 1
        try:
            mism += int(got_d[t] != oracle_list(keep, leg, t, 0))
        except Exception as e:  # the oracle could not take the trace's arrays: reported, counted as a mismatch
            errors.append(dict(trace=t, forward=int(keep["forward"][t]), error=repr(e)[:120],
                               geometry=[[int(keep["%s%d" % (nm, k)][t]) for nm in ("slice_begin", "slice_len", "ref_pos", "olen")] for k in range(2)]))
            mism += 1
    out.update(checked=len(idx), checked_called=seen, mismatches=mism, check_errors=errors[:4])
    print(json.dumps(out))
    return 0 if mism == 0 and not differ and out["mem_kinds_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
