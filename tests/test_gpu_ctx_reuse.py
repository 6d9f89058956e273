"""The scratch buffers of one context (tracyhip_ctx::dev, capi_internal.h) serve every entry point in turn, several roles to a slot.
Every call of the library, with host arrays, in a row on ONE context -- a small batch followed by a larger one, so that every buffer
regrows between its users, and the other way round -- must return what the same call returns on a context of its own."""
import ctypes as C

import numpy as np
import pytest

import pyoracle as orc
from decomp_cases import SC

pytestmark = pytest.mark.gpu

CALLS = ("align_traces", "pack_ragged", "trim_reference_slice", "find_breakpoint", "find_homozygous_breakpoint", "decompose_alleles",
         "secondary_decomposed", "allelic_fraction", "score", "consensus_traces", "assemble_traces", "basecall_traces", "align_traces_again")


def make_case(seed, n, mf, kind):
    """decomp_cases.make_case for a trace of mf bases, short ones included: the synthetic chromatogram places its indel at base 150,
    so it is made with 260 bases or more and cut behind base mf; the chain of indigo.h from there on as in decomp_cases"""
    from tracy_amd import hostlib
    ref, sig, pos, _ = hostlib.synth_decompose(seed, n, max(mf, 260), 30, kind, 0.6)
    pos = pos[:mf].copy()
    sig = np.ascontiguousarray(sig[:, :int(pos[-1]) + 13])
    pri, sec, _, bcpos = hostlib.basecall(sig, pos, 0.33)
    prof = hostlib.create_profile(sig, bcpos, pri, sec, 50, 50)
    bp = orc.find_breakpoint(prof)
    fwd = orc.create_profile_str(ref)
    _, btr = orc.gotoh_prof(prof, fwd, 1, 0, SC)
    rows = orc.create_alignment_prof(btr, prof, fwd)
    return dict(ref=ref, sig=sig, pos=pos, pri=pri, sec=sec, bcpos=bcpos, prof=prof, bp=bp, rows=rows)


def make_batch(seed, nt, lo, hi, ngroups):
    """nt traces of lo .. hi bases against references of 300 .. 600 bases, and pairs / groups of the same sizes"""
    from test_gpu_assemble_batch import make_groups
    from test_gpu_consensus_batch import make_pairs
    rng = np.random.default_rng(seed)
    cases = [make_case(seed * 100 + i, n=int(rng.integers(300, 601)), mf=int(rng.integers(lo, hi + 1)), kind=i % 2) for i in range(nt)]
    first, second = make_pairs(seed, nt, maxlen=hi)
    groups, grefs, _ = make_groups(seed, ngroups)
    stride = 48
    return dict(cases=cases, first=first, second=second, groups=groups, grefs=grefs, stride=stride,
                pack_src=rng.integers(0, 256, size=nt * stride).astype(np.uint8), pack_lens=rng.integers(0, stride + 1, size=nt).astype(np.int32))


def new_ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    c.set_option("no_stream", "1")
    return c


def trim_reference_slice(ctx, rows, reflen):
    from tracy_amd import capi
    n = len(rows)
    r0, r1, off, lens = capi._pack_rows(rows)
    rl = np.ascontiguousarray(reflen, dtype=np.uint32)
    fwd = (np.arange(n) % 2).astype(np.uint8)
    out = [np.zeros(n, dtype=np.uint32) for _ in range(3)]
    u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    rc = capi.lib().tracyhip_trim_reference_slice(ctx._h, C.c_uint32(n), r0.ctypes.data_as(u8p), r1.ctypes.data_as(u8p), capi._u64p(off), capi._u32p(lens),
                                                  capi._u32p(rl), fwd.ctypes.data_as(u8p), C.c_uint32(50), C.c_uint32(50), C.c_int(capi.MEM_HOST),
                                                  out[0].ctypes.data_as(u32p), out[1].ctypes.data_as(u32p), out[2].ctypes.data_as(u32p))
    assert rc == 0
    return out


def run(ctx, b, name):
    """one call of the list on the batch b"""
    import torch
    from tracy_amd import capi
    cs = b["cases"]
    hbc = lambda: capi.HostBaseCalls([c["sig"] for c in cs], [c["bcpos"] for c in cs], [c["pri"] for c in cs], [c["sec"] for c in cs])
    bps = lambda: [capi.Breakpoint(c["bp"].indelshift, c["bp"].traceleft, c["bp"].breakpoint, c["bp"].bestDiff) for c in cs]
    rows, reflen = [c["rows"] for c in cs], [len(c["ref"]) for c in cs]
    if name.startswith("align_traces"):
        res = ctx.align_traces([c["prof"] for c in cs], [c["ref"] for c in cs], SC, 50, 50)
        # the raw array, masked to [ops_offset[t], ops_offset[t] + ops_len[t]): what lies between two strings is no result
        used, at = np.zeros(res["ops"].shape, bool), 0
        for c, n in zip(cs, res["ops_len"]):
            used[at:at + int(n)] = True
            at += c["prof"].shape[1] + len(c["ref"])  # (PreparedAlign: a region of m + n bytes per trace, back to back)
        res["ops"] = np.where(used, res["ops"], 0).astype(np.uint8)
        return res
    if name == "pack_ragged":
        packed, nb = ctx.pack_ragged(torch.from_numpy(b["pack_src"]).cuda(), b["stride"], torch.from_numpy(b["pack_lens"]).cuda())
        return packed.cpu().numpy(), nb
    if name == "trim_reference_slice":
        return trim_reference_slice(ctx, rows, reflen)
    if name == "find_breakpoint":
        return ctx.find_breakpoint([c["prof"] for c in cs])
    if name == "find_homozygous_breakpoint":
        return ctx.find_homozygous_breakpoint(rows, [capi.Breakpoint(0, 1, 0, 0.0) for _ in cs])
    if name == "decompose_alleles":
        return ctx.decompose_alleles(hbc(), rows, bps(), reflen)
    if name == "secondary_decomposed":
        return ctx.secondary_decomposed(hbc())
    if name == "allelic_fraction":
        return ctx.allelic_fraction(hbc(), np.concatenate([np.frombuffer(c["sec"], dtype=np.uint8) for c in cs]), 50, 50)
    if name == "score":  # profile x profile: the ProfSeq list of build_problem
        return ctx.score(b["first"], b["second"], SC + (1, 1))
    if name == "consensus_traces":
        return ctx.consensus_traces(b["first"], b["second"], SC)
    if name == "assemble_traces":
        return ctx.assemble_traces(b["groups"], b["grefs"], SC)
    if name == "basecall_traces":
        return ctx.basecall_traces([c["sig"] for c in cs], [c["pos"] for c in cs])
    raise KeyError(name)


def same(a, b, where):
    """element for element; `where` names the call in a failure"""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], where + (k,))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, where + (i,))
    elif isinstance(a, C.Structure):
        assert bytes(a) == bytes(b), where
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where  # (bytes: NaN-proof, sign-of-zero-proof)
    else:
        assert a == b, where


@pytest.fixture(scope="module")
def batches():
    return dict(small=make_batch(5, 8, 60, 200, 3), large=make_batch(6, 24, 200, 400, 8))


@pytest.fixture(scope="module")
def alone(batches):
    """every call on a context of its own"""
    want = {}
    for size, b in batches.items():
        for name in CALLS:
            c = new_ctx()
            want[size, name] = run(c, b, name)
            c.close()
    return want


@pytest.mark.parametrize("order", [("small", "large"), ("large", "small")])
def test_every_call_in_a_row_on_one_context(batches, alone, order):
    ctx = new_ctx()
    try:
        for size in order:
            for name in CALLS:
                same(run(ctx, batches[size], name), alone[size, name], (size, name))
    finally:
        ctx.close()


def extents(b):
    """what sizes the payload buffers of a batch, in elements: bases, profile columns, reference bases, alignment columns, samples,
    columns of the pairs, columns of the groups' traces and references, packed bytes"""
    cs, gs = b["cases"], b["groups"]
    return (sum(len(c["pri"]) for c in cs), sum(c["prof"].shape[1] for c in cs), sum(len(c["ref"]) for c in cs),
            sum(len(c["rows"][0]) for c in cs), sum(c["sig"].shape[1] for c in cs), sum(p.shape[1] for p in b["first"]),
            sum(p.shape[1] for p in b["second"]), sum(p.shape[1] for g in gs for p in g), sum(r.shape[1] for r in b["grefs"]), len(b["pack_src"]))


def test_the_large_batch_outgrows_the_small_one(batches):
    """every payload extent by more than the slack DevBuf::ensure allocates (an eighth + 256 bytes; an element is a byte or more), so
    that going from the small batch to the large one regrows the buffer; and more traces, pairs, groups and traces in groups (arrays
    of a few bytes per trace may stay within that slack at these sizes: they are reused, not regrown)"""
    small, large = batches["small"], batches["large"]
    assert all(l > s + s // 8 + 256 for s, l in zip(extents(small), extents(large))), (extents(small), extents(large))
    assert len(large["cases"]) > len(small["cases"]) and len(large["groups"]) > len(small["groups"])
    assert sum(len(g) for g in large["groups"]) > sum(len(g) for g in small["groups"])


def test_the_calls_alone_return_something(batches, alone):
    """(the comparison above is not between two empty results)"""
    for size, b in batches.items():
        a = alone[size, "align_traces"]
        assert len(a["btr"]) == len(b["cases"]) and all(len(x) for x in a["btr"])
        assert alone[size, "pack_ragged"][1] == int(b["pack_lens"].sum())
        assert len(alone[size, "basecall_traces"]) == len(b["cases"])
