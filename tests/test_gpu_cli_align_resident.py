"""`tracy_amd_cli align --batch --resident`: the trace files of the manifest go to the device once, the text of the four output files comes
back once (tracy_amd/cli/align_resident.inc).  One manifest of 14 lines -- ABIF and SCF traces, FASTA references on both strands, two lines
on one FASTA, a reference far shorter than its trace, a trace of 60 calls, three lines on one wildtype trace, and three lines the device
must leave to the host path (a file that is no trace, trims that take the whole trace, a FASTA above 50 kb) -- is run with the flag and
without it: every file, the return code and the messages must be the same, and the files of four lines must be the oracle's
(tests/sage_oracle.py through expected_files), so that the command is not only compared with itself.

One deviation from "no output file for a bad line": the host path writes <prefix>.abif before it looks at the reference (prepare(), as the
reference's sage.h does), so the line whose FASTA is too long has an .abif in the run WITHOUT the flag, and the flag must not change what
the host path does.  For that one file the test asks for the same bytes in both runs; for every other file of a bad line, for absence."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli import CLI, expected_files, genomic_trace, synth_case, write_genome
from test_gpu_cli_trims import ALIGN_EXT, rough_ends
from test_host_and_abi import make_trace
from test_trace_io import write_scf3

pytestmark = pytest.mark.gpu
TRIMS = ["-q", "20", "-u", "20"]  # the 60-call trace keeps 20 calls; the 30-call trace is the one line these trims take all of
BAD = {7: "no trace", 12: "trims", 13: "long FASTA"}
ORACLE_LINES = (0, 1, 11, 8)  # three FASTA lines (line 1 on the reverse strand) and one wildtype line
N = 14


def fasta_for(rng, path, core, left, right, reverse=False):
    import sage_oracle as so
    fl = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())  # noqa: E731
    ref = fl(left) + bytes(core) + fl(right)
    if reverse:
        ref = so.revcomp(ref)
    with open(path, "w") as f:
        f.write(">chrSyn test\n")
        for i in range(0, len(ref), 70):
            f.write(ref[i:i + 70].decode() + "\n")


def small_trace(rng, path, nb):
    """an ABIF trace of nb calls; returns its basecalls"""
    from tracy_amd import hostlib
    tr, pos = make_trace(rng, nb, het=0.03)
    tr = np.minimum(tr, 32000)
    pri = hostlib.basecall(tr, pos, 0.33)[0]
    hostlib.write_abif(path, tr, pos, pri[:len(pos)].ljust(len(pos), b"N"), np.full(len(pos), 40, np.uint8))
    return pri.replace(b"N", b"C")


def build_manifest(d, rough):
    """(trace, reference, name) of the 14 lines; rough: a second peak under the ends of the good ABIF traces, so that -t 2 trims them apart"""
    from tracy_amd import hostlib
    rng = np.random.default_rng(20260)
    d = str(d)
    lines = [None] * N
    lines[0] = synth_case(rng, d, "f0", nb=550, nref=2500) + ("l00",)
    lines[1] = synth_case(rng, d, "f1", nb=480, nref=3000, reverse=True) + ("l01",)
    # an SCF trace against a FASTA that holds its calls
    tr, pos = make_trace(rng, 420, het=0.03)
    tr = np.minimum(tr, 32000)
    pri = hostlib.basecall(tr, pos, 0.33)[0].replace(b"N", b"C")
    write_scf3(os.path.join(d, "s2.scf"), tr, pos)
    fasta_for(rng, os.path.join(d, "s2.fa"), pri, 300, 400)
    lines[2] = (os.path.join(d, "s2.scf"), os.path.join(d, "s2.fa"), "l02")
    # a reference of 200 bp from the middle of a 520-call trace
    pri = small_trace(rng, os.path.join(d, "t3.ab1"), 520)
    fasta_for(rng, os.path.join(d, "t3.fa"), pri[160:360], 0, 0)
    lines[3] = (os.path.join(d, "t3.ab1"), os.path.join(d, "t3.fa"), "l03")
    # two lines on one FASTA file (with TRACY_AMD_CLI_BLOCK=5 they fall into different blocks)
    t4 = synth_case(rng, d, "f4", nb=600, nref=2000, reverse=True)
    lines[4] = t4 + ("l04",)
    lines[5] = t4 + ("l05",)
    pri = small_trace(rng, os.path.join(d, "t6.ab1"), 60)
    fasta_for(rng, os.path.join(d, "t6.fa"), pri, 200, 250)
    lines[6] = (os.path.join(d, "t6.ab1"), os.path.join(d, "t6.fa"), "l06")
    junk = os.path.join(d, "junk.ab1")
    open(junk, "wb").write(b"hello world, not a trace")
    lines[7] = (junk, lines[0][1], "l07")
    # three lines on one wildtype trace: the read it was made for, that read from the other strand, its first 400 calls
    w, wt = synth_case(rng, d, "w8", nb=450, wildtype=True)
    lines[8] = (w, wt, "l08")
    t = hostlib.read_trace(w)
    sig, p = t["signal"], t["basecallpos"]
    rsig = np.ascontiguousarray(sig[::-1, ::-1])
    rpos = (sig.shape[1] - 1 - p[::-1]).astype(np.int32)
    hostlib.write_abif(os.path.join(d, "w9.ab1"), rsig, rpos, b"N" * len(rpos), np.full(len(rpos), 30, np.uint8))
    lines[9] = (os.path.join(d, "w9.ab1"), wt, "l09")
    cut = int(p[400]) - 4
    hostlib.write_abif(os.path.join(d, "w10.ab1"), np.ascontiguousarray(sig[:, :cut]), p[:400], b"N" * 400, np.full(400, 30, np.uint8))
    lines[10] = (os.path.join(d, "w10.ab1"), wt, "l10")
    lines[11] = synth_case(rng, d, "f11", nb=680, nref=2200) + ("l11",)
    pri = small_trace(rng, os.path.join(d, "t12.ab1"), 30)
    lines[12] = (os.path.join(d, "t12.ab1"), lines[6][1], "l12")
    pri = small_trace(rng, os.path.join(d, "t13.ab1"), 400)
    fasta_for(rng, os.path.join(d, "t13.fa"), pri, 30000, 30000)
    lines[13] = (os.path.join(d, "t13.ab1"), os.path.join(d, "t13.fa"), "l13")
    pairs = {}  # line -> what trimTrace gives it at stringency 2
    if rough:
        for i, (trace, _, _) in enumerate(lines):
            if i in BAD or not trace.endswith(".ab1") or i in (5, 6):
                continue
            t = hostlib.read_trace(trace)
            sig = rough_ends(t["signal"], t["basecallpos"], (0, 25, 45, 70)[i % 4], (0, 30, 60)[i % 3], rng)
            pri = hostlib.basecall(sig, t["basecallpos"], 0.33)[0]
            n = len(t["basecallpos"])
            hostlib.write_abif(trace, sig, t["basecallpos"], pri[:n].ljust(n, b"N"), np.full(n, 40, np.uint8))
            l, r = hostlib.trim_trace(sig, t["basecallpos"], 0.33, 2)
            pairs[i] = (l & 0xFFFF, r & 0xFFFF)
    return lines, pairs


def run(lines, outdir, extra=(), resident=False, env=None):
    """the manifest through `align --batch`; returns (process, prefixes)"""
    os.makedirs(outdir, exist_ok=True)
    prefixes = [os.path.join(outdir, name) for _, _, name in lines]
    man = os.path.join(outdir, "manifest.tsv")
    with open(man, "w") as f:
        f.write("".join("%s\t%s\t%s\n" % (t, r, p) for (t, r, _), p in zip(lines, prefixes)))
    cmd = [CLI, "align", "--batch", man] + list(extra) + (["--resident"] if resident else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    return p, prefixes


def files_of(prefix):
    return {ext: (open(prefix + ext, "rb").read() if os.path.exists(prefix + ext) else None) for ext in ALIGN_EXT}


def same_runs(a, b, n=N):
    """(process, prefixes) of two runs: the same files line by line, the same return code, the same messages"""
    (pa, fa), (pb, fb) = a, b
    assert pa.returncode == pb.returncode, (pa.returncode, pb.returncode, pa.stderr[-800:], pb.stderr[-800:])
    assert sorted(pa.stderr.splitlines()) == sorted(pb.stderr.splitlines())
    for i in range(n):
        x, y = files_of(fa[i]), files_of(fb[i])
        for ext in ALIGN_EXT:
            assert x[ext] == y[ext], (i, ext, None if x[ext] is None else len(x[ext]), None if y[ext] is None else len(y[ext]))


def device_line(stdout):
    return [ln.split("] ", 1)[1] for ln in stdout.splitlines() if "] Device: " in ln]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """the manifest, and its two runs: with the flag and without it"""
    d = tmp_path_factory.mktemp("resident")
    lines, _ = build_manifest(d, rough=False)
    return dict(dir=str(d), lines=lines, resident=run(lines, str(d / "res"), TRIMS, resident=True), host=run(lines, str(d / "host"), TRIMS))


def test_resident_run_writes_the_files_of_the_host_path(plain):
    lines = plain["lines"]
    assert len(lines) == N and sum(t.endswith(".scf") for t, _, _ in lines) == 1
    assert lines[4][:2] == lines[5][:2] and len({r for i, (_, r, _) in enumerate(lines) if i in (8, 9, 10)}) == 1
    res, host = plain["resident"], plain["host"]
    same_runs(res, host)
    assert res[0].returncode == 2, res[0].stderr[-800:]  # (bad lines: the code of a --batch run that skipped some)
    for i in range(N):
        for tag, (_, prefixes) in (("resident", res), ("host", host)):
            got = files_of(prefixes[i])
            for ext in ALIGN_EXT:
                if i not in BAD:
                    assert got[ext], (tag, i, ext)
                elif (i, ext) == (13, ".abif"):
                    # the one file of a bad line that the host path has always written (before it loads the reference); see the module's text
                    assert got[ext] is not None and got[ext] == files_of(host[1][i])[ext], (tag, i)
                else:
                    assert got[ext] is None, (tag, i, ext)
    assert device_line(res[0].stdout) == ["Device: 11 of 14 traces read, basecalled, aligned and written"]
    assert device_line(host[0].stdout) == [] and "Device:" not in host[0].stdout
    for msg in ("Unknown trace file type!", "The sum of the left and right trim size is larger than the trace!", "Reference is larger than 50Kbp"):
        assert sum(msg in ln for ln in res[0].stderr.splitlines()) == 1, msg
    assert sum(ln.startswith("skipping ") for ln in res[0].stderr.splitlines()) == 3
    steps = [ln.split("] ", 1)[1] for ln in res[0].stdout.splitlines() if ln.startswith("[")][1:]
    assert [s for s in steps if not s.startswith("Device:")] == ["Load ab1 file", "Find reference match", "Alignment", "Output", "Done."]
    # the short reference: its row carries gaps at both ends
    fa = open(res[1][3] + ".align.fa").read().split("\n")
    assert fa[3].startswith("-") and fa[3].endswith("-") and len(fa[3].strip("-")) < 260, fa[3][:80]
    # both strands, both kinds
    txt = {i: open(res[1][i] + ".txt").read() for i in range(N) if i not in BAD}
    assert "reversecomplement" in txt[1] and " forward\n" in txt[0] and "reversecomplement" in txt[9] and ">Ref wildtype:" in txt[8]


@pytest.mark.parametrize("line", ORACLE_LINES)
def test_resident_files_against_the_oracle(plain, line):
    trace, ref, _ = plain["lines"][line]
    prefix = plain["resident"][1][line]
    want, _ = expected_files(trace, ref, os.path.splitext(os.path.basename(trace))[0], trim=(20, 20))
    for ext, txt in want.items():
        assert open(prefix + ext).read() == txt, (line, ext)
    if line == 1:
        assert "reversecomplement" in want[".txt"]


def test_resident_with_a_line_limit(plain):
    d, lines = plain["dir"], plain["lines"]
    a = run(lines, os.path.join(d, "res45"), TRIMS + ["-l", "45"], resident=True)
    b = run(lines, os.path.join(d, "host45"), TRIMS + ["-l", "45"])
    same_runs(a, b)
    assert device_line(a[0].stdout) == ["Device: 11 of 14 traces read, basecalled, aligned and written"]
    assert open(a[1][0] + ".txt", "rb").read() != open(plain["resident"][1][0] + ".txt", "rb").read()  # (the option reached the plot)


def test_resident_in_three_blocks(plain):
    """TRACY_AMD_CLI_BLOCK=5: lines 0-4, 5-9, 10-13 -- the shared FASTA (lines 4, 5) and the shared wildtype (8, 9 | 10) fall into different
    blocks, the last block is partial; the files are those of the one-block run"""
    d, lines = plain["dir"], plain["lines"]
    a = run(lines, os.path.join(d, "res_b5"), TRIMS, resident=True, env={"TRACY_AMD_CLI_BLOCK": "5"})
    same_runs(a, plain["resident"])
    assert device_line(a[0].stdout) == ["Device: 11 of 14 traces read, basecalled, aligned and written"]


def test_resident_with_a_trim_stringency(tmp_path):
    lines, pairs = build_manifest(tmp_path, rough=True)
    assert len(set(pairs.values())) >= 4, pairs
    a = run(lines, str(tmp_path / "res"), ["-t", "2"], resident=True)
    b = run(lines, str(tmp_path / "host"), ["-t", "2"])
    same_runs(a, b)
    answered = int(device_line(a[0].stdout)[0].split()[1])
    written = sum(os.path.exists(p + ".json") for p in a[1])
    assert answered == written >= 10, (answered, written, a[0].stderr[-800:])  # (every line that has files was the device's)
    # the trims reached the device: the .abif table marks them, and a trimmed line is the oracle's for its own pair
    want, _ = expected_files(lines[1][0], lines[1][1], "f1", trim=pairs[1])
    for ext, txt in want.items():
        assert open(a[1][1] + ext).read() == txt, ext


def test_resident_leaves_an_indexed_genome_to_the_host_path(tmp_path):
    rng = np.random.default_rng(2719)
    gpath, contigs = write_genome(rng, str(tmp_path), ncontigs=2, clen=6000)
    lines = [(genomic_trace(rng, str(tmp_path), "g%d" % i, contigs, nb=int(rng.integers(300, 500)), reverse=bool(i % 2)), gpath, "g%d" % i) for i in range(3)]
    a = run(lines, str(tmp_path / "res"), ["-d", "0,0"], resident=True)
    b = run(lines, str(tmp_path / "host"))
    same_runs(a, b, n=3)
    assert a[0].returncode == 0, a[0].stderr[-800:]
    assert device_line(a[0].stdout) == ["Device: 0 of 3 traces read, basecalled, aligned and written"]
    assert sum("--resident runs on one GPU" in ln for ln in a[0].stdout.splitlines()) == 1
    for p in a[1]:
        assert all(files_of(p)[ext] for ext in ALIGN_EXT), p
