"""The text printed from a plate of final alignments (tracyhip_render_alignments), one JSON line.  Per form (the plot at key 0 and 60
columns per block, the FASTA, the JSON tail): ms of the call with rows, names and text resident on the device; the kernel time of its
launches (letters + count + scan from the sizes-only call, emit as the rest); the call from host buffers end to end; the host writers
(tracyhost_alntext_batch: plotAlignment / alignFastaOut / the tail of traceAlignJsonOut into a TextBuf per alignment) on 16 threads on
the same data in the same run; and the comparison that decides whether the command line should print on the device:
    rows_back_then_host_print     the two rows copied device -> host, then the host writers on 16 threads
    device_print_then_text_back   the device call, then the text copied device -> host
each with a pinned and with a pageable destination.  Every alignment's text is compared between the host writers and both device forms.

The data: the rows of the final alignments of N synthetic 1 kb traces against their 1.4 kb windows, odd traces on the reverse strand
(hostlib.synth_decompose_batch, what bench.py's workloads align): one align_traces call, tracyhip_reference_slices and
tracyhip_alignment_rows in the same process.  One warm-up round and `--reps` timed rounds, the forms interleaved; a timed device step
ends in a device synchronisation.

    python tools/alntext_device_line.py [--alignments 10000] [--reps 3] [--out profiles/alntext_device_line.json]
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
HOST_THREADS = 16
TIMER_MISC = 8
FORM_NAMES = {0: "plot", 1: "fasta", 2: "json"}
KEY, LINE = 0, 60


class KernelTiming(C.Structure):
    _fields_ = [("ms", C.c_double), ("launches", C.c_uint64), ("cells", C.c_uint64), ("bytes", C.c_uint64)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def final_rows(ctx, profiles, refs):
    """align_traces, reference_slices and alignment_rows from host buffers: per trace (row0, row1) and the per-trace numbers"""
    from tracy_amd import capi
    nt = len(profiles)
    res = ctx.align_traces(profiles, refs, SCORE, 50, 50)
    slices = ctx.reference_slices(refs, res["forward"], res["slice_begin"], res["slice_len"])
    pp, ps = capi.PackedSeqs(profiles, capi.SEQ_PROFILE), capi.PackedSeqs(slices, capi.SEQ_CHAR)
    pr = capi.Pairs()
    pr.npairs, pr.a1, pr.a2 = nt, pp.seqset(), ps.seqset()
    olen = np.ascontiguousarray(res["ops_len"], dtype=np.uint32)
    off = np.zeros(nt, np.uint64)
    off[1:] = np.cumsum(olen.astype(np.uint64))[:-1]
    ops = np.frombuffer(b"".join(res["btr"]) + b"\0", np.uint8).copy()
    r0, r1 = np.zeros_like(ops), np.zeros_like(ops)
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    capi._check(capi.lib().tracyhip_alignment_rows(ctx._h, C.byref(pr), capi.MEM_HOST, u8p(ops), capi._u64p(off), capi._u32p(olen), u8p(r0), u8p(r1)))
    cut = lambda a: [a[int(off[t]):int(off[t]) + int(olen[t])].tobytes() for t in range(nt)]
    return cut(r0), cut(r1), res


class Form:
    """one form over the data set: the prepared calls and the clocks of their steps"""

    def __init__(self, ctx, form, args):
        from tracy_amd import capi, hostlib
        self.ctx, self.form, self.nt = ctx, form, len(args["rows0"])
        self.dev = capi.PreparedAlnText(form, key=KEY, linelimit=LINE, device=True, **args)
        self.sizes = self.dev.sizes(ctx)
        self.dev.with_capacity(self.sizes)
        self.host = capi.PreparedAlnText(form, key=KEY, linelimit=LINE, device=False, **args).with_capacity(self.sizes)
        self.flat = self.host.flat
        self.hout = hostlib.alntext_alloc(self.nt, self.sizes)
        self.text_bytes = int(self.sizes.astype(np.int64).sum())
        self.binary = [self.dev.d["rows0"], self.dev.d["rows1"]]  # what the copy back of the rows moves
        self.binary_bytes = int(sum(t.numel() * t.element_size() for t in self.binary))
        self.t = {k: [] for k in ("device_resident", "host_buffers", "host_writers_16_threads", "kernel_measure", "kernel_all", "rows_back_pinned",
                                  "rows_back_pageable", "text_back_pinned", "text_back_pageable")}

    def kernel_ms(self, fn):
        from tracy_amd import capi
        lib = capi.lib()
        capi._check(lib.tracyhip_timing_reset(self.ctx._h))
        dt = timed(fn)
        kt = KernelTiming()
        capi._check(lib.tracyhip_timing_get(self.ctx._h, TIMER_MISC, C.byref(kt)))
        return dt, kt.ms

    def round(self, keep, pinned, pageable):
        from tracy_amd import hostlib
        o = self.dev.o
        _, measure = self.kernel_ms(lambda: self.dev.sizes(self.ctx))
        self.dev._bind(o)
        dt, every = self.kernel_ms(lambda: self.dev.run(self.ctx))
        host = timed(lambda: self.host.run(self.ctx))
        t0 = time.perf_counter()
        hostlib.alntext_batch_raw(self.flat, self.form, self.hout, KEY, LINE, HOST_THREADS)
        writers = time.perf_counter() - t0
        back = {}
        txt = self.dev.o["text"]
        for kind, dst in (("pinned", pinned), ("pageable", pageable)):  # (both destinations exist and have been written before the clock starts)
            def binary():
                at = 0
                for src in self.binary:
                    dst[at:at + src.numel()].copy_(src)
                    at += src.numel()
            back["rows_back_" + kind] = timed(binary)
            back["text_back_" + kind] = timed(lambda: dst[:txt.numel()].copy_(txt))
        if keep:
            for k, v in dict(device_resident=dt, host_buffers=host, host_writers_16_threads=writers, kernel_measure=1e-3 * measure, kernel_all=1e-3 * every,
                             **back).items():
                self.t[k].append(v)

    def report(self):
        from tracy_amd import hostlib
        best = {k: min(v) for k, v in self.t.items()}
        out = {k + "_ms": [round(1e3 * x, 3) for x in v] for k, v in self.t.items()}
        out["text_bytes"], out["rows_bytes"] = self.text_bytes, self.binary_bytes
        out["text_over_rows"] = round(self.text_bytes / self.binary_bytes, 2)
        out["kernel_emit_ms"] = round(1e3 * (best["kernel_all"] - best["kernel_measure"]), 3)
        out["text_GBps"] = round((2 * self.binary_bytes + self.text_bytes) / best["kernel_all"] / 1e9, 1)  # (the rows once per pass)
        out["device_resident_alignments_per_s"] = round(self.nt / best["device_resident"], 1)
        out["host_buffers_alignments_per_s"] = round(self.nt / best["host_buffers"], 1)
        out["host_writers_16_threads_alignments_per_s"] = round(self.nt / best["host_writers_16_threads"], 1)
        out["host_buffers_win_over_host_writers"] = bool(best["host_buffers"] < best["host_writers_16_threads"])
        for kind in ("pinned", "pageable"):
            a = best["rows_back_" + kind] + best["host_writers_16_threads"]
            b = best["device_resident"] + best["text_back_" + kind]
            out["chain_%s" % kind] = dict(rows_back_then_host_print_ms=round(1e3 * a, 3), device_print_then_text_back_ms=round(1e3 * b, 3),
                                          device_print_wins=bool(b < a), ratio=round(a / b, 2))
        # every alignment between the host writers and the two device forms: whole buffers first (the layouts are the same)
        want = self.hout
        unequal = deferred = 0
        for p in (self.dev, self.host):
            got = p.host_arrays()
            deferred += int((got["status"][:self.nt] != 0).sum())
            if np.array_equal(got["text_len"][:self.nt], want["text_len"][:self.nt]) and np.array_equal(got["text"], want["text"]):
                continue
            for t in range(self.nt):
                a, b = hostlib.alntext_unpack(got, t), hostlib.alntext_unpack(want, t)
                unequal += 0 if (a["status"] == b["status"] and a.get("text") == b.get("text")) else 1
        out.update(compared=2 * self.nt, unequal=unequal, deferred=deferred)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alignments", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alntext_device_line.json"))
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi, hostlib
    nt, mf = a.alignments, 1000
    d = hostlib.synth_decompose_batch(4711, nt, mf + 400, mf, 0, 1)  # (the data of tools/render_device_line.py)
    ctx = tracy_amd.Context(0)
    rows0, rows1, res = final_rows(ctx, list(d["profiles"]), [r.tobytes() for r in d["refs"]])
    capi._check(capi.lib().tracyhip_timing_enable(ctx._h, 1))
    pos, ln, fwd = res["ref_pos"].astype(np.int64), res["slice_len"].astype(np.int64), res["forward"]
    plot1 = [b">Ref chr%d:%d-%d %s" % (t % 24, pos[t] + 1, pos[t] + ln[t], b"forward" if fwd[t] else b"reversecomplement") for t in range(nt)]
    chrs = [b"chr%d" % (t % 24) for t in range(nt)]
    common = dict(rows0=rows0, rows1=rows1, ref_pos=pos, ref_len=ln, forward=fwd, score=res["score_final"])
    names = {0: dict(name0=[b">Alt"] * nt, name1=plot1), 1: dict(name0=[b"trace%05d" % t for t in range(nt)], name1=chrs), 2: dict(name0=[b""] * nt, name1=chrs)}
    out = {"alignments": nt, "bases": mf, "columns_mean": round(float(np.mean([len(r) for r in rows0])), 1), "reverse": int(nt - fwd.sum()), "key": KEY,
           "linelimit": LINE, "reps": a.reps, "host_threads": HOST_THREADS}
    fs = {f: Form(ctx, f, dict(common, **names[f])) for f in (0, 1, 2)}
    room = max(max(f.text_bytes, f.binary_bytes) for f in fs.values()) + 64
    pinned, pageable = torch.zeros(room, dtype=torch.uint8, pin_memory=True), torch.zeros(room, dtype=torch.uint8)
    pageable.fill_(1)  # (every page touched)
    for rep in range(a.reps + 1):  # (the first round warms up and is not kept)
        for f in fs:
            fs[f].round(rep > 0, pinned, pageable)
    for f in fs:
        out[FORM_NAMES[f]] = fs[f].report()
    ctx.close()
    parts = [out[FORM_NAMES[f]] for f in fs]
    out["compared"] = sum(v["compared"] for v in parts)
    out["unequal"] = sum(v["unequal"] for v in parts)
    out["deferred"] = sum(v["deferred"] for v in parts)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["unequal"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
