"""`align -t 2 --batch` and `decompose -t 2 --batch`: trimTrace gives every trace of the manifest its own (trimLeft, trimRight), the block
goes through ONE device call with per-trace trims, and every output file is the one the one-trace command writes for that trace."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli import CLI, expected_files
from test_host_and_abi import make_trace

pytestmark = pytest.mark.gpu
ALIGN_EXT = (".txt", ".json", ".align.fa", ".abif")
DECOMPOSE_EXT = (".decomp", ".align1", ".align2", ".align3", ".json", ".abif")


def rough_ends(sig, pos, a, b, rng):
    """a second peak under the first `a` and the last `b` basecalls: ambiguous calls there, which trimTrace cuts off"""
    sig = sig.copy()
    n = len(pos)
    for j in list(range(a)) + list(range(n - b, n)):
        p = int(pos[j])
        top = int(np.argmax(sig[:, p]))
        other = (top + 1 + int(rng.integers(0, 3))) % 4
        lo, hi = max(p - 5, 0), min(p + 6, sig.shape[1])
        sig[other, lo:hi] = np.maximum(sig[other, lo:hi], (sig[top, lo:hi] * 0.7).astype(sig.dtype))
    return sig


def timers(stderr):
    line = [ln for ln in stderr.split("\n") if ln.startswith("timers:")]
    assert len(line) == 1, stderr
    w = line[0].split()
    return {w[i]: float(w[i + 1]) for i in range(1, len(w) - 1, 2)}


def run_batch_and_singles(tmp_path, command, rows, exts, extra=()):
    """the manifest through --batch (timers on), then every trace alone; the files of both, byte for byte"""
    man = str(tmp_path / "manifest.tsv")
    open(man, "w").write("".join("\t".join(r) + "\n" for r in rows))
    env = dict(os.environ, TRACY_AMD_CLI_TIMERS="1")
    p = subprocess.run([CLI, command, "-t", "2", "--batch", man, *extra], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr
    t = timers(p.stderr)
    assert t["traces"] == len(rows) and t["device_calls"] == 1, t  # one block, one reference kind: one call, whatever the trims
    for trace, ref, prefix in rows:
        single = prefix + "_single"
        q = subprocess.run([CLI, command, "-t", "2", "-r", ref, "-o", single, *extra, trace], capture_output=True, text=True, timeout=300)
        assert q.returncode == 0, (trace, q.stderr)
        for ext in exts:
            assert open(prefix + ext, "rb").read() == open(single + ext, "rb").read(), (trace, ext)


def test_align_batch_with_a_trim_stringency(tmp_path):
    from tracy_amd import hostlib
    import sage_oracle as so
    rng = np.random.default_rng(5)
    rows, pairs = [], []
    for i in range(12):
        tr, pos = make_trace(rng, int(rng.integers(400, 700)), het=0.03)
        tr = rough_ends(np.minimum(tr, 32000), pos, (0, 25, 45, 70)[i % 4], (0, 30, 60)[i % 3], rng)
        l, r = hostlib.trim_trace(tr, pos, 0.33, 2)
        pairs.append((l & 0xFFFF, r & 0xFFFF))
        pri = hostlib.basecall(tr, pos, 0.33)[0]
        trace = str(tmp_path / ("a%d.ab1" % i))
        hostlib.write_abif(trace, tr, pos, pri[:len(pos)].ljust(len(pos), b"N"), np.full(len(pos), 40, np.uint8))
        core = bytearray(pri.replace(b"N", b"C"))
        del core[200:203]
        fl = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())  # noqa: E731
        ref = fl(int(rng.integers(100, 900))) + bytes(core) + fl(int(rng.integers(100, 900)))
        if i % 2:
            ref = so.revcomp(ref)
        ref_path = str(tmp_path / ("a%d.fa" % i))
        open(ref_path, "w").write(">chrSyn\n%s\n" % ref.decode())
        rows.append((trace, ref_path, str(tmp_path / ("ares%d" % i))))
    assert len(set(pairs)) >= 4, pairs
    assert all(l + r < 300 for l, r in pairs), pairs  # (no trace trimmed away: the commands refuse those)
    run_batch_and_singles(tmp_path, "align", rows, ALIGN_EXT)
    for (trace, ref, prefix), pair in zip(rows, pairs):
        want, _ = expected_files(trace, ref, os.path.splitext(os.path.basename(trace))[0], trim=pair)
        for ext, txt in want.items():
            assert open(prefix + ext).read() == txt, (trace, ext, pair)


def test_decompose_batch_with_a_trim_stringency(tmp_path):
    from tracy_amd import hostlib
    import sage_oracle as so
    rng = np.random.default_rng(6)
    rows, pairs = [], []
    for i in range(12):
        ref, sig, pos, _ = hostlib.synth_decompose(6100 + i, 1200 + 50 * i, 400 + 25 * i, 12, 0, 0.6)
        sig = rough_ends(np.minimum(sig, 32000), pos, (0, 25, 45, 70)[i % 4], (0, 30, 60)[i % 3], rng)
        l, r = hostlib.trim_trace(sig, pos, 0.33, 2)
        pairs.append((l & 0xFFFF, r & 0xFFFF))
        trace = str(tmp_path / ("d%d.ab1" % i))
        hostlib.write_abif(trace, sig, pos, b"N" * len(pos), np.full(len(pos), 30, np.uint8))
        ref_path = str(tmp_path / ("d%d.fa" % i))
        open(ref_path, "w").write(">amplicon%d\n%s\n" % (i, (so.revcomp(ref) if i % 2 else ref).decode()))
        rows.append((trace, ref_path, str(tmp_path / ("dres%d" % i))))
    assert len(set(pairs)) >= 4, pairs
    run_batch_and_singles(tmp_path, "decompose", rows, DECOMPOSE_EXT + (".vcf",), extra=("-v",))
