"""The row-block wave bodies of `tracy assemble` (tracy_amd/csrc/assemble_wave.h: msa_merge, msa_profile, msa_consensus) on the 64-fiber
host wave, against the host C++ (msalib.profile_of_alignment, msalib.consensus: tracy_amd/host/msa.hpp) and the Python restatements of
tests/msa_oracle.py -- exact equality, profile floats bit for bit.  Plus the argument checks of tracyhip_assemble_traces, which need
no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import msa_oracle as mo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

BLOCKS = ((1, 1), (1, 4), (3, 2))
COLUMNS = (1, 63, 64, 65, 300)
ALPHABET = b"ACGTACGTACGTN-acgtnX"  # lower-case letters and a foreign byte among them


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libemu_assemble.so")
    srcs = [os.path.join(HERE, "emu", "emu_assemble.cpp"), os.path.join(HERE, "emu", "host_wave.h"),
            os.path.join(ROOT, "tracy_amd/csrc/assemble_wave.h"), os.path.join(ROOT, "tracy_amd/csrc/dp_lane.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0]],
                              stderr=subprocess.DEVNULL)
    return C.CDLL(so)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def op_strings(rng, L):
    """forward-order op strings of L columns: all 's'; leading and trailing 'h'; 'v' runs (across the 64-column rounds where L allows);
    a random mix"""
    out = {"all_s": "s" * L}
    lead, trail = min(L // 3, 70), min(L // 4, 5)
    out["h_ends"] = "h" * lead + "s" * (L - lead - trail) + "h" * trail if L > 1 else "h"
    v = ["s"] * L
    for start in (60, 120, 250):  # 60..70 and 120..135 cross the rounds that begin at 64 and 128
        for j in range(start, min(start + (11 if start == 60 else 16), L)):
            v[j] = "v"
    if L <= 60:
        for j in range(L // 2, min(L // 2 + 3, L)):
            v[j] = "v"
    out["v_runs"] = "".join(v)
    out["mix"] = "".join(rng.choice(list("ssssshv"), size=L).tolist())
    return out


def random_rows(rng, n, c, all_gap_row):
    rows = [bytes(rng.choice(list(ALPHABET), size=c).tolist()) for _ in range(n)]
    for i in range(n):  # leading / trailing gaps: the spans differ from row to row
        a, b = int(rng.integers(0, c // 3 + 1)), int(rng.integers(0, c // 3 + 1))
        rows[i] = (b"-" * a + rows[i][a:c - b] + b"-" * b)[:c]
    if all_gap_row and n > 1:
        rows[n - 1] = b"-" * c
    return rows


def random_profile(rng, c):
    p = rng.random((6, c)).astype(np.float32)
    p[:, ::5] = 0.25  # ties: the first maximum wins
    p[5, 1::7] = 2.0  # the gap row wins: 'N', never '-'
    return np.ascontiguousarray(p)


def merge_oracle(ops, a1, a2):
    """the merge of msa_oracle.palign (msa.h:121-150; assemble.h:266-284 with one new row)"""
    rows = [[] for _ in range(len(a1) + len(a2))]
    x = y = 0
    for op in ops:
        for k in range(len(a1)):
            rows[k].append(a1[k][x:x + 1] if op != "h" else b"-")
        x += op != "h"
        for k in range(len(a2)):
            rows[len(a1) + k].append(a2[k][y:y + 1] if op != "v" else b"-")
        y += op != "v"
    return [b"".join(r) for r in rows]


def span_oracle(row):
    idx = [j for j, ch in enumerate(row) if ch != ord("-")]
    return (idx[0], idx[-1]) if idx else (-1, -1)


def run_merge(emu, ops, left, right):
    """left / right: a list of byte rows, or a float32 [6][c] profile"""
    L = len(ops)
    push = np.frombuffer(ops[::-1].encode(), np.uint8).copy()

    def side(x):
        if isinstance(x, np.ndarray):
            return None, x, 1, x.shape[1]
        return np.frombuffer(b"".join(x) + b"\0", np.uint8).copy(), None, len(x), len(x[0])
    r1, p1, n1, c1 = side(left)
    r2, p2, n2, c2 = side(right)
    out = np.full((n1 + n2) * L + 1, 0x7e, np.uint8)
    span = np.full(2 * (n1 + n2), -7, np.int32)
    rc = emu.emu_msa_merge(_p(push), C.c_uint32(L), _p(r1), _p(p1), C.c_uint32(n1), C.c_uint32(c1), _p(r2), _p(p2), C.c_uint32(n2),
                           C.c_uint32(c2), _p(out), _p(span))
    assert rc == 0 and out[-1] == 0x7e
    return [out[i * L:(i + 1) * L].tobytes() for i in range(n1 + n2)], span.reshape(-1, 2)


def run_profile(emu, rows):
    n, c = len(rows), len(rows[0])
    blob = np.frombuffer(b"".join(rows) + b"\0", np.uint8).copy()
    prof = np.full(6 * c + 1, -7.0, np.float32)
    assert emu.emu_msa_profile(_p(blob), C.c_uint32(n), C.c_uint32(c), _p(prof)) == 0
    assert prof[-1] == -7.0
    return prof[:6 * c].reshape(6, c)


def run_consensus(emu, rows, fraction_called, ignore_last):
    n, c = len(rows), len(rows[0])
    blob = np.frombuffer(b"".join(rows) + b"\0", np.uint8).copy()
    gapped, cons, qual = (np.full(c + 1, 0x7e, np.uint8) for _ in range(3))
    ln = C.c_uint32(0xdead)
    assert emu.emu_msa_consensus(_p(blob), C.c_uint32(n), C.c_uint32(c), C.c_float(fraction_called), int(ignore_last), _p(gapped), _p(cons),
                                 _p(qual), C.byref(ln)) == 0
    k = ln.value
    assert k <= c and gapped[c] == 0x7e and (cons[k:] == 0x7e).all() and (qual[k:] == 0x7e).all()
    return gapped[:c].tobytes(), cons[:k].tobytes(), qual[:k].tobytes()


def cases():
    """(name, ops, left, right) over every block shape, column count and op pattern; single-row sides also as profiles"""
    rng = np.random.default_rng(20240611)
    for n1, n2 in BLOCKS:
        for L in COLUMNS:
            for name, ops in op_strings(rng, L).items():
                c1, c2 = sum(o != "h" for o in ops), sum(o != "v" for o in ops)
                if c1 == 0 or c2 == 0:
                    continue
                left = random_rows(rng, n1, c1, all_gap_row=False)
                right = random_rows(rng, n2, c2, all_gap_row=(name == "mix"))
                yield "%d+%d/%d/%s" % (n1, n2, L, name), ops, left, right
                if n1 == 1:
                    yield "p+%d/%d/%s" % (n2, L, name), ops, random_profile(rng, c1), right
                if n1 == 1 and n2 == 1:
                    yield "p+p/%d/%s" % (L, name), ops, random_profile(rng, c1), random_profile(rng, c2)


def as_rows(x):
    return [("".join(mo.cons_char(x, j) for j in range(x.shape[1]))).encode()] if isinstance(x, np.ndarray) else x


@pytest.fixture(scope="module")
def merged(emu):
    """every case merged once on the host wave: (name, rows) -- the inputs of the profile and consensus tests"""
    out = []
    for name, ops, left, right in cases():
        rows, span = run_merge(emu, ops, left, right)
        want = merge_oracle(ops, as_rows(left), as_rows(right))
        assert rows == want, name
        assert [tuple(s) for s in span.tolist()] == [span_oracle(r) for r in want], name
        out.append((name, rows))
    out.append(("crafted", [b"X-ACn", b"x-a--"]))  # a column of foreign bytes only; '-' inside both spans; a trailing gap outside one
    return out


def test_merge_matches_the_restated_merge(merged):
    names = [n for n, _ in merged]
    assert len(names) >= 3 * 5 * 3
    for shape in ("1+1/", "1+4/", "3+2/", "p+4/", "p+p/"):
        assert any(n.startswith(shape) for n in names), shape
    rows300 = dict(merged)["3+2/300/v_runs"]
    assert all(r[60:71] == b"-" * 11 and r[120:136] == b"-" * 16 for r in rows300[3:])  # the 'v' runs across the rounds at 64 and 128
    assert any(set(r) == {ord("-")} for n, rows in merged if n.endswith("mix") for r in rows)  # a row of gaps only
    assert any(b"X" in r for _, rows in merged for r in rows) and any(b"a" in r for _, rows in merged for r in rows)


def test_profile_is_the_host_profile_bit_for_bit(emu, merged):
    from tracy_amd import msalib
    zero_sum = 0
    for name, rows in merged:
        got = run_profile(emu, rows)
        host = msalib.profile_of_alignment(rows)
        assert got.tobytes() == np.ascontiguousarray(host).tobytes(), name
        py = mo.profile_of_alignment([r.decode("latin1") for r in rows])
        assert got.tobytes() == np.ascontiguousarray(py).tobytes(), name
        zero_sum += int((got.sum(0) == 0).sum())
    assert zero_sum > 0  # (columns of foreign bytes only: the sum is 0 and the counts stand as they are)
    crafted = run_profile(emu, dict(merged)["crafted"])
    assert crafted[:, 0].tolist() == [0] * 6 and crafted[:, 1].tolist() == [0, 0, 0, 0, 0, 1] and crafted[:, 4].tolist() == [0, 0, 0, 0, 1, 0]


@pytest.mark.parametrize("fraction_called", [0.1, 0.6])
@pytest.mark.parametrize("ignore_last", [0, 1])
def test_consensus_is_the_host_consensus(emu, merged, fraction_called, ignore_last):
    from tracy_amd import msalib
    called = uncalled = 0
    for name, rows in merged:
        got = run_consensus(emu, rows, fraction_called, ignore_last)
        assert got == msalib.consensus(rows, fraction_called, bool(ignore_last)), name
        py = mo.consensus([r.decode("latin1") for r in rows], fraction_called, bool(ignore_last))
        assert got == tuple(x.encode("latin1") for x in py), name
        called += len(got[1])
        uncalled += len(got[0]) - len(got[1])
    assert called > 1000 and uncalled > 100


# ---- the argument checks of tracyhip_assemble_traces ------------------------------------------------------------------------------


def _job(lens=((5, 7), (4,)), refs=(9, 6)):
    from tracy_amd import capi
    groups = [[np.full((6, n), 0.1, np.float32) for n in g] for g in lens]
    return capi.PreparedAssemble(groups, [np.full((6, n), 0.1, np.float32) for n in refs], (3, -5, -10, -4))


def test_argument_validation_needs_no_device():
    """tracyhip_assemble_validate: what tracyhip_assemble_traces checks before it touches a device"""
    from tracy_amd import capi
    lib = capi.lib()
    ERR_ARG = -1

    def check(p, mem=0):
        return lib.tracyhip_assemble_validate(C.byref(p.job), C.byref(p.prm), mem, C.byref(p.out))
    p = _job()
    assert check(p) == 0 and check(p, 1) == 0
    assert check(p, 2) == ERR_ARG
    assert lib.tracyhip_assemble_validate(None, C.byref(p.prm), 0, C.byref(p.out)) == ERR_ARG
    assert lib.tracyhip_assemble_validate(C.byref(p.job), None, 0, C.byref(p.out)) == ERR_ARG
    assert lib.tracyhip_assemble_validate(C.byref(p.job), C.byref(p.prm), 0, None) == ERR_ARG
    for field, bad in (("group_first", None), ("match_fraction", float("nan")), ("fraction_called", float("nan"))):
        p = _job()
        setattr(p.job, field, bad)
        assert check(p) == ERR_ARG, field
        assert field.split("_")[0] in lib.tracyhip_last_error().decode()
    for which in ("traces", "references"):
        for field in ("data", "offset", "length"):
            p = _job()
            setattr(getattr(p.job, which), field, None)
            assert check(p) == ERR_ARG, (which, field)
        p = _job()
        getattr(p.job, which).kind = capi.SEQ_CHAR
        assert check(p) == ERR_ARG, which
    for field, _ in capi.AssembleResult._fields_:
        p = _job()
        setattr(p.out, field, None)
        assert check(p) == ERR_ARG, field
    p = _job()  # group_first decreases
    p.first[1] = 3
    p.first[2] = 2
    assert check(p) == ERR_ARG and "decreases" in lib.tracyhip_last_error().decode()
    p = _job()  # ... runs past the set
    p.first[2] = 4
    assert check(p) == ERR_ARG
    p = _job()  # a trace without columns
    p.keep[0].length[1] = 0
    assert check(p) == ERR_ARG and "no columns" in lib.tracyhip_last_error().decode()
    p = _job()  # a reference without columns
    p.keep[1].length[0] = 0
    assert check(p) == ERR_ARG
    p = _job()  # ref_index out of range
    ridx = np.array([0, 2], np.uint32)
    p.job.ref_index = ridx.ctypes.data_as(C.POINTER(C.c_uint32))
    assert check(p) == ERR_ARG
    ridx[1] = 0  # two groups on one reference
    assert check(p) == 0
    p = _job()  # an empty batch is fine
    p.job.ngroups = 0
    assert check(p) == 0
    # the call itself answers the same before it looks for a device
    p = _job()
    p.job.match_fraction = float("nan")
    assert lib.tracyhip_assemble_traces(None, C.byref(p.job), C.byref(p.prm), 0, C.byref(p.out)) == ERR_ARG
    assert "match_fraction" in lib.tracyhip_last_error().decode()


# ---- what `assemble --batch` refuses before it opens a device ----------------------------------------------------------------------


def test_cli_batch_refusals_need_no_device(tmp_path):
    cli = os.path.join(ROOT, "tracy_amd", "bin", "tracy_amd_cli")
    assert os.path.exists(cli), "tracy_amd_cli is not built: run __graft_entry__.build()"
    for name in ("t1.ab1", "t2.ab1"):
        (tmp_path / name).write_bytes(b"x")
    (tmp_path / "r1.fa").write_text(">r\nACGT\n")
    (tmp_path / "r2.fa").write_text(">r\nACGTA\n")
    man = tmp_path / "m.tsv"
    man.write_text("# trace\treference\toutprefix\nt1.ab1\tr1.fa\tout/a\nt2.ab1\tr2.fa\tout/a\n")
    run = lambda args: subprocess.run([cli, "assemble"] + args, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    r = run(["--batch", "m.tsv"])  # de novo assembly has no batch mode
    assert r.returncode == 1 and "--batch needs a reference (-r)" in r.stderr
    r = run(["-r", "r1.fa", "--batch", "m.tsv"])  # two references under one outprefix: the message names the line
    assert r.returncode == 1 and "line 3" in r.stderr and "out/a" in r.stderr and "r2.fa" in r.stderr
    man.write_text("t1.ab1\tr1.fa\n")
    r = run(["-r", "r1.fa", "--batch", "m.tsv"])
    assert r.returncode == 1 and "Malformed manifest line 1" in r.stderr
    man.write_text("missing.ab1\t-\tout/a\n")
    r = run(["-r", "r1.fa", "--batch", "m.tsv"])
    assert r.returncode == 1 and "Trace file is missing: missing.ab1" in r.stderr


# ---- the whole chain on the host wave -----------------------------------------------------------------------------------------------


def test_chain_of_wave_bodies_is_the_oracle_chain(emu):
    """the reference-guided chain as assemble.hip composes it -- merge of two profiles, then per step profile, dynamic program (the
    oracle's here), merge with the trace as row 0, and the consensus -- against the restated chain the GPU test compares with"""
    import pyoracle as orc
    import test_gpu_assemble_batch as gb
    groups, refs, kinds = gb.make_groups()
    done = set()
    for g in range(16):  # every kind of group twice
        for incref in (False, True):
            want = gb.oracle_group(groups[g], refs[g], gb.SCORE, gb.FRACMATCH, gb.CALLED, incref)
            if not want["order"]:
                continue
            chosen = [groups[g][s["idx"]] if want["forward"][s["idx"]] else np.ascontiguousarray(orc.revcomp_profile(groups[g][s["idx"]]))
                      for s in want["order"]]
            _, btr = orc.gotoh_prof(chosen[0], refs[g], 1, 0, gb.SCORE)
            rows, _ = run_merge(emu, btr[::-1].decode(), chosen[0], refs[g])
            for p in chosen[1:]:
                prof = np.ascontiguousarray(run_profile(emu, rows))
                _, btr = orc.gotoh_prof(p, prof, 1, 0, gb.SCORE)
                rows, _ = run_merge(emu, btr[::-1].decode(), p, rows)
            assert rows == want["rows"], g
            assert run_consensus(emu, rows, gb.CALLED, not incref) == (want["gapped"], want["cons"], want["qual"]), g
            done.add(kinds[g])
    assert done == {"plain", "single", "tie", "insertion", "cross64", "cross256", "onecol"}
