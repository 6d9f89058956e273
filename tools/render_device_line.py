"""The text of a plate of traces (tracyhip_render_traces), one JSON line.  Per form and sample width: ms of the call with chromatograms,
basecalls and text resident on the device; the kernel time of its launches (count + scan from the sizes-only call, emit as the rest)
and text_GBps = (chromatogram bytes read by the launches + text bytes written) / kernel time; the call from host buffers end to end; the
host writers (tracyhost_render_batch: traceTxtOut / traceJsonBody / assemblyTrace into a TextBuf per trace) on 16 threads on the same
data in the same run; and the comparison that decides whether the command line should print on the device:
    binary_back_then_host_print   the chromatograms and basecall arrays copied device -> host, then the host writers on 16 threads
    device_print_then_text_back   the device call, then the text copied device -> host
each with a pinned and with a pageable destination.  Every trace's text is compared between the host writers and both device forms.

The data: N synthetic 1 kb traces of 12 012 samples x 4 (hostlib.synth_decompose_batch, what bench.py's decompose workload renders) for
the table and the JSON body, and their gapped chromatograms along the rows of one align_traces call (the "plain" workload of
tools/pad_device_line.py, padded by tracyhip_pad_traces in the same process) for the gapped trace.  One warm-up round and `--reps` timed
rounds, the forms of a data set interleaved; a timed device step ends in a device synchronisation.

    python tools/render_device_line.py [--traces 10000] [--reps 3] [--out profiles/render_device_line.json]
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
FORM_NAMES = {0: "tsv", 1: "json", 2: "gapped"}


class KernelTiming(C.Structure):
    _fields_ = [("ms", C.c_double), ("launches", C.c_uint64), ("cells", C.c_uint64), ("bytes", C.c_uint64)]


def rows_of(btr):
    """row 0 of the alignments from their op strings (push order): 'h' is a gap of the trace; only '-' against a letter is read"""
    out = []
    for b in btr:
        ops = np.frombuffer(b, np.uint8)[::-1]
        out.append(np.where(ops == ord("h"), ord("-"), ord("N")).astype(np.uint8).tobytes())
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


class Form:
    """one form x sample width over one data set: the prepared calls and the clocks of their steps"""

    def __init__(self, ctx, form, sigs, bc, trims, dt):
        from tracy_amd import capi, hostlib
        self.ctx, self.form, self.nt, self.sb = ctx, form, len(sigs), np.dtype(dt).itemsize
        tl, tr = trims if trims else (None, None)
        sigs = [s.astype(dt) if s.dtype != dt else s for s in sigs]
        self.dev = capi.PreparedRender(form, sigs, bc, tl, tr, device=True, sample_dtype=dt)
        self.sizes = self.dev.sizes(ctx)
        self.dev.with_capacity(self.sizes)
        self.host = capi.PreparedRender(form, sigs, bc, tl, tr, device=False, sample_dtype=dt).with_capacity(self.sizes)
        self.flat = self.host.flat
        self.hout = hostlib.render_alloc(self.nt, self.sizes)
        self.text_bytes = int(self.sizes.astype(np.int64).sum())
        # what the binary copy back moves: the chromatograms and the basecall arrays the form prints
        keys = ["signal", "bcpos", "primary", "secondary", "estqual"] + (["consensus"] if form == 0 else [])
        self.binary = [self.dev.d[k] for k in keys]
        self.binary_bytes = int(sum(t.numel() * t.element_size() for t in self.binary))
        self.t = {k: [] for k in ("device_resident", "host_buffers", "host_writers_16_threads", "kernel_measure", "kernel_all", "binary_back_pinned",
                                  "binary_back_pageable", "text_back_pinned", "text_back_pageable")}

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
        hostlib.render_batch_raw(self.flat, self.form, self.hout, HOST_THREADS)
        writers = time.perf_counter() - t0
        back = {}
        txt = self.dev.o["text"]
        for kind, dst in (("pinned", pinned), ("pageable", pageable)):  # (both destinations exist and have been written before the clock starts)
            def binary():
                for src in self.binary:
                    dst[:src.numel() * src.element_size()].view(src.dtype).copy_(src)
            back["binary_back_" + kind] = timed(binary)
            back["text_back_" + kind] = timed(lambda: dst[:txt.numel()].copy_(txt))
        if keep:
            for k, v in dict(device_resident=dt, host_buffers=host, host_writers_16_threads=writers, kernel_measure=1e-3 * measure, kernel_all=1e-3 * every,
                             **back).items():
                self.t[k].append(v)

    def report(self):
        from tracy_amd import hostlib
        best = {k: min(v) for k, v in self.t.items()}
        out = {k + "_ms": [round(1e3 * x, 3) for x in v] for k, v in self.t.items()}
        ns_bytes = 4 * self.sb * int(self.flat["nsamples"][:self.nt].astype(np.int64).sum())
        reads = 2  # every form reads each sample once per pass (count, emit)
        out["text_bytes"], out["binary_bytes"] = self.text_bytes, self.binary_bytes
        out["text_over_binary"] = round(self.text_bytes / self.binary_bytes, 2)
        out["kernel_emit_ms"] = round(1e3 * (best["kernel_all"] - best["kernel_measure"]), 3)
        out["text_GBps"] = round((reads * ns_bytes + self.text_bytes) / best["kernel_all"] / 1e9, 1)
        out["device_resident_traces_per_s"] = round(self.nt / best["device_resident"], 1)
        out["host_buffers_traces_per_s"] = round(self.nt / best["host_buffers"], 1)
        out["host_writers_16_threads_traces_per_s"] = round(self.nt / best["host_writers_16_threads"], 1)
        for kind in ("pinned", "pageable"):
            a = best["binary_back_" + kind] + best["host_writers_16_threads"]
            b = best["device_resident"] + best["text_back_" + kind]
            out["chain_%s" % kind] = dict(binary_back_then_host_print_ms=round(1e3 * a, 3), device_print_then_text_back_ms=round(1e3 * b, 3),
                                          device_print_wins=bool(b < a), ratio=round(a / b, 2))
        # every trace between the host writers and the two device forms: whole buffers first (the layouts are the same), traces where they differ
        want = self.hout
        unequal = deferred = 0
        for p in (self.dev, self.host):
            got = p.host_arrays()
            deferred += int((got["status"][:self.nt] != 0).sum()) + int((want["status"][:self.nt] != 0).sum())
            if np.array_equal(got["text_len"][:self.nt], want["text_len"][:self.nt]) and np.array_equal(got["text"], want["text"]):
                continue
            for t in range(self.nt):
                a, b = hostlib.render_unpack(got, t), hostlib.render_unpack(want, t)
                unequal += 0 if (a["status"] == b["status"] and a.get("text") == b.get("text")) else 1
        out.update(compared=2 * self.nt, unequal=unequal, deferred=deferred)
        return out


def dataset(ctx, forms, sigs, bc, trims, reps):
    out = {}
    for dt in (np.int32, np.int16):
        fs = {f: Form(ctx, f, sigs, bc, trims if f == 0 else None, dt) for f in forms}
        room = max(max(f.text_bytes, f.binary_bytes) for f in fs.values()) + 64
        pinned, pageable = torch.zeros(room, dtype=torch.uint8, pin_memory=True), torch.zeros(room, dtype=torch.uint8)
        pageable.fill_(1)  # (every page touched)
        for rep in range(reps + 1):  # (the first round warms up and is not kept)
            for f in forms:
                fs[f].round(rep > 0, pinned, pageable)
        del pinned, pageable
        for f in forms:
            out["%s_%s" % (FORM_NAMES[f], np.dtype(dt).name)] = fs[f].report()
        del fs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_device_line.json"))
    a = ap.parse_args()
    import tracy_amd
    from tracy_amd import capi, hostlib
    nt, mf = a.traces, 1000
    d = hostlib.synth_decompose_batch(4711, nt, mf + 400, mf, 0, 1)  # (the data of tools/pad_device_line.py)
    d["estqual"] = (np.arange(nt * mf, dtype=np.int64).reshape(nt, mf) % 61).astype(np.uint8)
    ctx = tracy_amd.Context(0)
    capi._check(capi.lib().tracyhip_timing_enable(ctx._h, 1))
    ns = int(d["signal"].shape[2])
    out = {"traces": nt, "bases": mf, "samples": ns, "reps": a.reps, "host_threads": HOST_THREADS}
    sigs = [d["signal"][t] for t in range(nt)]
    bc = [dict(bcpos=d["bcpos"][t], primary=d["primary"][t], secondary=d["secondary"][t], consensus=d["primary"][t], estqual=d["estqual"][t])
          for t in range(nt)]
    trims = (np.full(nt, 50, np.uint32), np.full(nt, 50, np.uint32))
    out["synthetic"] = dataset(ctx, (0, 1), sigs, bc, trims, a.reps)
    # the gapped chromatograms of the same traces along their alignment rows
    res = ctx.align_traces(list(d["profiles"]), [r.tobytes() for r in d["refs"]], SCORE, 50, 50)
    padded = ctx.pad_traces(sigs, bc, rows_of(res["btr"]), device=True).results(fill_deferred=False)
    assert all(r["status"] == 0 for r in padded)
    psigs = [r["signal"] for r in padded]
    pbc = [dict(bcpos=r["bcPos"], primary=r["primary"], secondary=r["secondary"], consensus=r["consensus"], estqual=r["estQual"]) for r in padded]
    out["padded"] = dataset(ctx, (2,), psigs, pbc, None, a.reps)
    out["padded"]["pseudo_calls"] = int(sum(r["primary"].count(b"-") for r in padded))
    ctx.close()
    parts = [v for part in ("synthetic", "padded") for v in out[part].values() if isinstance(v, dict)]
    out["unequal"] = sum(v["unequal"] for v in parts)
    out["deferred"] = sum(v["deferred"] for v in parts)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["unequal"] == 0 and out["deferred"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
