"""Needleman-Wunsch on the device (tracyhip_needle_score / tracyhip_needle_align) against the oracle, bit for bit, on the cases of
tests/needle_cases.py: the ten needle kernels in trace and score form (strings at strip heights 4, 8, 16, profiles at 4 and 8, each in
one pass and in several), the walk kernel, and the host driver around them -- order by strip height, 4-byte traceback words, chunks
under a workspace limit, index arrays, device buffers, the range guard.  tests/test_emu_needle.py runs the same cases through the same
wave bodies on the CPU; what only this file reaches is the DPP shift, the barriers between passes, the rounding intrinsics of the
profile score and the driver.

Nothing here looks at the bytes of `ops` between one pair's ops_len and the next pair's offset: the header does not promise them."""
import ctypes as C

import numpy as np
import pytest

import needle_cases as nc
import pyoracle as orc

pytestmark = pytest.mark.gpu

GOTOH_SC = (3, -5, -10, -4)
FILL_I32, FILL_U32, FILL_U8 = -77777777, 0xEEEEEEEE, 0xEE


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def oracle(case, cfg, sc, needle=True):
    """(score, btr, rows) of a case"""
    _, a, b = case
    if nc.is_prof(case):
        want = (orc.needle_prof if needle else orc.gotoh_prof)(a, b, cfg[0], cfg[1], sc)
        return want + (orc.create_alignment_prof(want[1], a, b),)
    want = (orc.needle_str if needle else orc.gotoh_str)(a, b, cfg[0], cfg[1], sc)
    return want + (orc.create_alignment_str(want[1], a, b),)


def compare_batch(ctx, cases, cfg, sc):
    """the cases in one ragged batch per call: scores, tracebacks, rows and score-only values equal the oracle's"""
    a1, a2 = [c[1] for c in cases], [c[2] for c in cases]
    scores, btr, rows = ctx.align(a1, a2, sc + cfg, needle=True, rows=True)
    sc_only = ctx.score(a1, a2, sc + cfg, needle=True)
    for i, case in enumerate(cases):
        want = oracle(case, cfg, sc)
        assert int(scores[i]) == want[0] and btr[i] == want[1], (case[0], cfg, sc)
        assert int(sc_only[i]) == want[0], (case[0], cfg, sc)
        assert rows[i] == want[2], (case[0], cfg, sc)


def raw_call(ctx, a1, a2, params, trace=True, needle=True, idx=(None, None), with_scores=True, device=False):
    """tracyhip_needle_align / _score (needle=False: the Gotoh calls) on arrays prefilled with a sentinel, in host memory or (device=True:
    sequence data, scores, ops and ops_len; the offset and length arrays stay host arrays) in device memory.  Returns the return code, the
    message and the arrays as the call left them."""
    from tracy_amd import capi
    pr, keep, p1, p2 = ctx._pairs(a1, a2, idx[0], idx[1])
    n = pr.npairs
    l1, l2 = ctx._pair_lengths(pr, p1, p2, idx[0], idx[1])
    cap = (l1 + l2).astype(np.uint64)
    off = np.zeros(max(n, 1), dtype=np.uint64)
    off[1:n] = np.cumsum(cap)[:-1]
    scores = np.full(max(n, 1), FILL_I32, np.int32)
    ops = np.full(max(int(cap.sum()), 1), FILL_U8, np.uint8)
    olen = np.full(max(n, 1), FILL_U32, np.uint32)
    ptr = {"scores": scores.ctypes.data, "ops": ops.ctypes.data, "olen": olen.ctypes.data}
    if device:
        import torch
        d1, d2 = torch.from_numpy(p1.data).cuda(), torch.from_numpy(p2.data).cuda()
        pr.a1, pr.a2 = p1.seqset(d1.data_ptr()), p2.seqset(d2.data_ptr())
        dev = {"scores": torch.from_numpy(scores).cuda(), "ops": torch.from_numpy(ops).cuda(), "olen": torch.from_numpy(olen.view(np.int32)).cuda()}
        ptr = {k: v.data_ptr() for k, v in dev.items()}
        torch.cuda.synchronize()
    prm = capi.Params(*params)
    mem = capi.MEM_DEVICE if device else capi.MEM_HOST
    ps = C.c_void_p(ptr["scores"]) if with_scores else None
    lib = capi.lib()
    if trace:
        fn = lib.tracyhip_needle_align if needle else lib.tracyhip_gotoh_align
        rc = fn(ctx._h, C.byref(pr), C.byref(prm), mem, ps, C.c_void_p(ptr["ops"]), off.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(ptr["olen"]))
    else:
        fn = lib.tracyhip_needle_score if needle else lib.tracyhip_gotoh_score
        rc = fn(ctx._h, C.byref(pr), C.byref(prm), mem, ps)
    msg = lib.tracyhip_last_error().decode() if rc else ""
    if device:
        ctx.synchronize()
        torch.cuda.synchronize()
        scores, ops, olen = dev["scores"].cpu().numpy(), dev["ops"].cpu().numpy(), dev["olen"].cpu().numpy().view(np.uint32)
    out = dict(rc=rc, msg=msg, scores=scores[:n], ops=ops, olen=olen[:n], off=off)
    if trace and rc == 0:
        out["btr"] = [ops[int(off[i]):int(off[i]) + int(olen[i])].tobytes() for i in range(n)]
    return out


def untouched(res, trace=True):
    return bool((res["scores"] == FILL_I32).all() and (not trace or ((res["ops"] == FILL_U8).all() and (res["olen"] == FILL_U32).all())))


def test_the_cases_hold_every_kernel():
    """here as well as in the CPU file: an edit of the sizes must not drop a kernel from the device tests unnoticed"""
    nc.assert_every_kernel_is_reached()


@pytest.mark.parametrize("cfg", nc.CONFIGS)
def test_strings_equal_the_oracle(ctx, cfg):
    for si, sc in enumerate(nc.SCORINGS):
        cases = nc.interleaved(nc.cases_of_scoring(nc.string_cases(), si))
        ks = [nc.strip_height(nc.shape(c)[0], False) for c in cases]
        # the caller's order is not the launch order (strip heights descending): results must come back by PairDesc::out
        assert ks[0] != ks[1] and sum(x != y for x, y in zip(ks, ks[1:])) >= 2 * min(ks.count(K) for K in (4, 8, 16))
        assert nc.classes(cases) == nc.STRING_CLASSES
        compare_batch(ctx, cases, cfg, sc)


@pytest.mark.parametrize("cfg", nc.CONFIGS)
def test_profiles_equal_the_oracle(ctx, cfg):
    """every kind exact: (m + n + 2) (|go| + |ge| + 37.5^2 x 5) + 10^6 is far below 2^29 at these sizes, so the range guard has no say"""
    for si, sc in enumerate(nc.SCORINGS):
        cases = nc.interleaved(nc.cases_of_scoring(nc.profile_cases(), si))
        assert nc.classes(cases) == nc.PROFILE_CLASSES
        compare_batch(ctx, cases, cfg, sc)


def test_index_arrays_and_null_scores(ctx):
    rng = np.random.default_rng(20263)
    # all pairs i < j of a set in descending length: rows of 16-, 8- and 4-row strips, several passes, an empty sequence
    seqs = [nc.rand_bytes(rng, m, b"ACGT") for m in (1100, 1000, 600, 300, 257, 130, 65, 64, 5, 1, 0)]
    seqs[2] = nc.noisy_copy(rng, seqs[5], 600, b"ACGT")
    profs = [nc.profile_of_kind(rng, m, "random") for m in (600, 300, 97, 64, 1)]
    profs[2] = nc.resampled(rng, profs[0], 97)
    sc, cfg = nc.SCORINGS[0], (1, 0)
    for pool, want_of in ((seqs, orc.needle_str), (profs, orc.needle_prof)):
        idx1 = [i for i in range(len(pool)) for j in range(len(pool)) if i < j]
        idx2 = [j for i in range(len(pool)) for j in range(len(pool)) if i < j]
        scores, btr = ctx.align(pool, pool, sc + cfg, needle=True, idx1=idx1, idx2=idx2)
        sc_only = ctx.score(pool, pool, sc + cfg, needle=True, idx1=idx1, idx2=idx2)
        for k, (i, j) in enumerate(zip(idx1, idx2)):
            want = want_of(pool[i], pool[j], cfg[0], cfg[1], sc)
            assert (int(scores[k]), btr[k]) == want and int(sc_only[k]) == want[0], (i, j)
        res = raw_call(ctx, pool, pool, sc + cfg, idx=(idx1, idx2), with_scores=False)
        assert res["rc"] == 0, res["msg"]
        assert res["btr"] == btr and (res["scores"] == FILL_I32).all()


def test_device_buffers(ctx):
    """TRACYHIP_MEM_DEVICE: the same scores, lengths and ops as the host-buffer call, strings and profiles, pairs of several passes among them"""
    sc, cfg = nc.SCORINGS[0], (0, 1)
    for cases in (nc.string_cases(), nc.profile_cases()):
        cases = nc.interleaved(cases)
        assert any((nc.klass(c) or (0, False))[1] for c in cases)
        a1, a2 = [c[1] for c in cases], [c[2] for c in cases]
        host = raw_call(ctx, a1, a2, sc + cfg)
        dev = raw_call(ctx, a1, a2, sc + cfg, device=True)
        assert host["rc"] == 0 and dev["rc"] == 0, (host["msg"], dev["msg"])
        assert np.array_equal(host["scores"], dev["scores"]) and np.array_equal(host["olen"], dev["olen"]) and host["btr"] == dev["btr"]
        # in device memory nothing but the pair's own bytes is written
        own = np.zeros(len(dev["ops"]), bool)
        for o, l in zip(dev["off"], dev["olen"]):
            own[int(o):int(o) + int(l)] = True
        assert (dev["ops"][~own] == FILL_U8).all()
        host_s = raw_call(ctx, a1, a2, sc + cfg, trace=False)
        dev_s = raw_call(ctx, a1, a2, sc + cfg, trace=False, device=True)
        assert host_s["rc"] == 0 and dev_s["rc"] == 0
        assert np.array_equal(host_s["scores"], dev_s["scores"]) and np.array_equal(host_s["scores"], host["scores"])
        for i in (0, len(cases) // 2, len(cases) - 1):
            assert int(dev["scores"][i]) == oracle(cases[i], cfg, sc)[0]
        dev_n = raw_call(ctx, a1, a2, sc + cfg, with_scores=False, device=True)  # scores == NULL in device memory too
        assert dev_n["rc"] == 0 and dev_n["btr"] == host["btr"] and (dev_n["scores"] == FILL_I32).all()


def test_chunks_under_a_workspace_limit(ctx):
    from tracy_amd import capi
    sc, cfg = nc.SCORINGS[0], (1, 0)
    cases = nc.interleaved(nc.string_cases())
    a1, a2 = [c[1] for c in cases], [c[2] for c in cases]
    needs = [nc.trace_bytes(*nc.shape(c), False) for c in cases]
    largest = max(needs)
    assert largest == max(nc.passes(len(a), nc.strip_height(len(a), False)) * (len(b) + 63) * 64 * 4 for _, a, b in cases) < (1 << 19)
    limit = max(largest, sum(needs) // 4)
    chunks = nc.planned_chunks(cases, limit)
    assert len(chunks) >= 3
    assert any(len({nc.klass(c)[0] for c in ch if nc.klass(c)}) > 1 for ch in chunks)  # a chunk of more than one launch
    whole = ctx.align(a1, a2, sc + cfg, needle=True)
    try:
        ctx.set_workspace_limit(limit)
        cut = ctx.align(a1, a2, sc + cfg, needle=True)
        assert np.array_equal(cut[0], whole[0]) and cut[1] == whole[1]
        ctx.set_workspace_limit(largest)  # the largest pair in a chunk of its own, to the byte
        cut = ctx.align(a1, a2, sc + cfg, needle=True)
        assert np.array_equal(cut[0], whole[0]) and cut[1] == whole[1]
        ctx.set_workspace_limit(largest - 1)
        res = raw_call(ctx, a1, a2, sc + cfg)
        assert res["rc"] == capi.ERR_OOM and str(largest) in res["msg"] and str(largest - 1) in res["msg"], res["msg"]
        assert untouched(res)
        # score-only calls need no traceback words: the same limit does not stop them
        assert np.array_equal(ctx.score(a1, a2, sc + cfg, needle=True), whole[0])
    finally:
        ctx.set_workspace_limit(0)
    for i, case in enumerate(cases):
        assert (int(whole[0][i]), whole[1][i]) == oracle(case, cfg, sc)[:2], case[0]


def value_bound(p1, p2, sc):
    """(m + n + 2) (|go| + |ge| + largest |substitution score|) + 10^6: the rule of tracyhip_params (tracy_hip.h) with the substitution
    score un-normalised profiles can reach, at most the product of the two largest column masses (rows A C G T N) times the larger of
    |match|, |mismatch|.  The cells are int32; the traceback form keeps two tag bits below the value."""
    ma, mb = (float(np.abs(p[:5]).sum(axis=0).max()) for p in (p1, p2))
    return (p1.shape[1] + p2.shape[1] + 2) * (abs(sc[2]) + abs(sc[3]) + max(ma, 1.001) * max(mb, 1.001) * max(abs(sc[0]), abs(sc[1]))) + 1e6


def test_range_and_argument_errors(ctx):
    from test_gpu_range import exact_or_range
    from tracy_amd import capi
    rng = np.random.default_rng(20264)
    sc, cfg = nc.SCORINGS[0], (1, 1)
    # needle takes two strings or two profiles
    p = nc.profile_of_kind(rng, 40, "random")
    for trace in (True, False):
        res = raw_call(ctx, [p], [b"ACGTACGTAC"], sc + cfg, trace=trace)
        assert res["rc"] == capi.ERR_ARG and "needle" in res["msg"], res
        assert untouched(res, trace)
    # a NaN anywhere in a profile
    p1, p2 = nc.profile_of_kind(rng, 200, "random"), nc.profile_of_kind(rng, 97, "random")
    p2[2, 17] = np.float32("nan")
    for trace in (True, False):
        res = raw_call(ctx, [p1], [p2], sc + cfg, trace=trace)
        assert res["rc"] == capi.ERR_RANGE, res
    # un-normalised profiles: the exact result or ERR_RANGE, never another value; exact where the bound leaves a twentieth of room in
    # the cells (31 bits score-only, two less with the traceback's tags).  The scale 20 000 is on one side only: on both, the
    # substitution scores pass 2^31 and the reference's own int arithmetic has no defined result.
    for scale1, scale2 in ((400.0, 400.0), (20000.0, 1.0)):
        for (m, n) in ((120, 97), (600, 300)):
            p1 = nc.profile_of_kind(rng, m, "random") * np.float32(scale1)
            p2 = nc.resampled(rng, p1, n) * np.float32(scale2 / scale1)
            bound = value_bound(p1, p2, sc)
            assert bound < 2 ** 31  # (the oracle's int holds it)
            want = orc.needle_prof(p1, p2, cfg[0], cfg[1], sc)
            assert orc.needle_score_prof(p1, p2, cfg[0], cfg[1], sc) == want[0]
            exact_or_range(lambda: int(ctx.score([p1], [p2], sc + cfg, needle=True)[0]), want[0], bound * 1.05 < 2 ** 31)

            def aligned():
                s, b = ctx.align([p1], [p2], sc + cfg, needle=True)
                return (int(s[0]), b[0])
            exact_or_range(aligned, want, bound * 1.05 < 2 ** 29)
    for trace in (True, False):
        res = raw_call(ctx, [b"ACGT"], [b"ACGT"], (50000, -4, -10, -1) + cfg, trace=trace)
        assert res["rc"] == capi.ERR_RANGE and untouched(res, trace), res


def test_back_to_back_with_gotoh_on_one_context(ctx):
    """Gotoh, needle, Gotoh on one context: both keep their traceback words and hand-over rows in the same two buffers, in words of
    eight bytes and of four"""
    picked = [c for c in nc.string_cases() if nc.shape(c) in ((0, 7), (5, 65), (257, 64), (513, 65), (1024, 64), (1281, 130), (2049, 63))]
    ppicked = [c for c in nc.profile_cases() if nc.shape(c)[0] in (65, 768, 1024)]  # (normalised kinds: Gotoh is not the subject here)
    assert len(picked) == 7 and len(ppicked) == 9 and {nc.kind_of(c) for c in ppicked} == {"random", "onehot", "dyadic"}
    cfg = (1, 0)
    for cases in (picked, ppicked):
        a1, a2 = [c[1] for c in cases], [c[2] for c in cases]
        for needle, sc in ((False, GOTOH_SC), (True, nc.SCORINGS[0]), (False, GOTOH_SC)):
            scores, btr = ctx.align(a1, a2, sc + cfg, needle=needle)
            for i, case in enumerate(cases):
                assert (int(scores[i]), btr[i]) == oracle(case, cfg, sc, needle)[:2], (case[0], needle)
