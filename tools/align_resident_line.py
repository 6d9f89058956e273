"""`tracy_amd_cli align --batch` with and without --resident on the same files, one JSON line.  The workload is the command-line row of the
README (tools/legs.py CliLeg: N synthetic 1 kb ABIF files on a tmpfs, one FASTA window per trace, written before any clock starts).  The
two forms run alternately, `--reps` times each, with the same --threads; every run has a directory of its own for its output files, and the
four files of every line of a resident run are compared byte for byte with those of the host run before it (then both sets are deleted: a
run writes ~0.4 MB per trace).  Reported per run: traces/s of the whole command, its TRACY_AMD_CLI_TIMERS line, the lines the device
answered; and the number of files compared and found identical.

    python tools/align_resident_line.py [--traces 10000] [--reps 3] [--threads 16] [--out profiles/align_resident_line.json]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

EXTS = (".abif", ".align.fa", ".txt", ".json")


def run_cli(cli, rows, outdir, threads, resident):
    """one command over the manifest's (trace, reference) pairs with its output files under outdir"""
    os.makedirs(outdir)
    man = os.path.join(outdir, "manifest.tsv")
    with open(man, "w") as f:
        f.write("".join("%s\t%s\t%s\n" % (t, r, os.path.join(outdir, "o%06d" % i)) for i, (t, r) in enumerate(rows)))
    cmd = [cli, "align", "--batch", man, "-d", "0", "--threads", str(threads)] + (["--resident"] if resident else [])
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, TRACY_AMD_CLI_TIMERS="1"))
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (" ".join(cmd[:4]), p.returncode, p.stderr[-600:]))
    timers = {}
    for ln in p.stderr.splitlines():
        if ln.startswith("timers:"):
            tok = ln.split()[1:]
            timers = {tok[i]: float(tok[i + 1]) for i in range(0, len(tok) - 1, 2)}
    answered = None
    for ln in p.stdout.splitlines():
        if "] Device: " in ln:
            answered = int(ln.split("] Device: ", 1)[1].split()[0])
    return {"mode": "resident" if resident else "host", "traces_per_s": round(len(rows) / dt, 1), "wall_s": round(dt, 3), "timers": timers,
            "device_answered": answered}


def compare(a, b, n, threads):
    """(files compared, files identical) over the four files of every line of two runs"""
    def one(i):
        same = 0
        for ext in EXTS:
            x, y = os.path.join(a, "o%06d%s" % (i, ext)), os.path.join(b, "o%06d%s" % (i, ext))
            with open(x, "rb") as fx, open(y, "rb") as fy:
                same += fx.read() == fy.read()
        return same
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return len(EXTS) * n, sum(ex.map(one, range(n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_resident_line.json"))
    a = ap.parse_args()
    from legs import CliLeg
    leg = CliLeg(a.traces, 0, 1, SimpleNamespace(index=0))
    out = {"metric": "traces/s, `tracy_amd_cli align --batch` end to end, with and without --resident, same files, alternating",
           "traces": a.traces, "bases": 1000, "reps": a.reps, "host_threads": a.threads, "files_on": "%s (%s)" % (leg.fs, os.path.dirname(leg.tmp)), "runs": []}
    try:
        man, d, prep_s, b = leg.make_files("align", 10000, 1000)
        del b
        rows = [tuple(ln.split("\t")[:2]) for ln in open(man).read().splitlines()]
        out["files_prepared_s"] = round(prep_s, 1)
        compared = identical = 0
        for rep in range(a.reps):
            dirs = {}
            for resident in (False, True):
                dirs[resident] = os.path.join(leg.tmp, "run%d_%s" % (rep, "resident" if resident else "host"))
                out["runs"].append(run_cli(leg.cli, rows, dirs[resident], a.threads, resident))
            c, s = compare(dirs[False], dirs[True], a.traces, a.threads)
            compared += c
            identical += s
            for v in dirs.values():
                shutil.rmtree(v, ignore_errors=True)
        out["files_compared"], out["files_identical"] = compared, identical
        for mode in ("host", "resident"):
            v = sorted(r["traces_per_s"] for r in out["runs"] if r["mode"] == mode)
            out[mode + "_traces_per_s"] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
        out["device_answered"] = [r["device_answered"] for r in out["runs"] if r["mode"] == "resident"]
        out["resident_over_host_median"] = round(out["resident_traces_per_s"]["median"] / out["host_traces_per_s"]["median"], 2)
    finally:
        shutil.rmtree(leg.tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["files_compared"] == out["files_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
