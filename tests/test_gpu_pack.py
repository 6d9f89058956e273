"""tracyhip_pack_ragged_multi (tracy_amd/csrc/pack.hip): the used parts of fixed-stride regions back to back, kind-major -- what a rank
does to its variable-length results before the final gather.  Every alignment of source and destination, empty regions, lengths that
exceed their stride (clamped), length words read with a stride out of a record array, int32 elements; against numpy.  And the shapes
only a large batch reaches, at the smallest sizes that cross each boundary: more scan workgroups than pack_top_kernel has threads (its
serial part), regions of several 256-byte steps in every alignment, the limit of sixteen payload kinds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import tracy_amd
    c = tracy_amd.Context(0)
    yield c
    c.close()


def expect(kinds_np, n):
    parts = []
    for buf, stride, lens, lens_stride in kinds_np:
        elem = buf.dtype.itemsize
        raw = buf.view(np.uint8)
        for i in range(n):
            ln = min(int(lens[i * lens_stride]) * elem, stride * elem)
            parts.append(raw[i * stride * elem:i * stride * elem + ln])
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pack_ragged_multi_against_numpy(ctx, seed):
    import torch
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 700))
    F = 5  # the lengths of the first two kinds are columns of an int32 record array
    rec = rng.integers(0, 50, size=(n, F)).astype(np.int32)
    s0, s1, s2 = 37, 64, 9
    rec[:, 1] = rng.integers(0, s0 + 6, size=n)   # some beyond the stride: clamped
    rec[:, 3] = rng.integers(0, s1 + 1, size=n)
    rec[rng.integers(0, n, size=max(1, n // 5)), 1] = 0  # empty regions
    lens2 = rng.integers(0, s2 + 1, size=n).astype(np.int32)
    b0 = rng.integers(0, 256, size=n * s0).astype(np.uint8)
    b1 = rng.integers(0, 256, size=n * s1).astype(np.uint8)
    b2 = rng.integers(-2**31, 2**31 - 1, size=n * s2).astype(np.int32)
    want = expect([(b0, s0, rec.reshape(-1)[1:], F), (b1, s1, rec.reshape(-1)[3:], F), (b2, s2, lens2, 1)], n)
    d_rec = torch.from_numpy(rec).cuda()
    flat = d_rec.reshape(-1)
    d = [torch.from_numpy(x).cuda() for x in (b0, b1, b2)]
    d_l2 = torch.from_numpy(lens2).cuda()
    packed, sizes = ctx.pack_ragged_multi([(d[0], s0, flat[1:], F), (d[1], s1, flat[3:], F), (d[2], s2, d_l2, 1)], n)
    assert sum(sizes) == want.size and np.array_equal(packed.cpu().numpy(), want)
    # one kind through tracyhip_pack_ragged, into a buffer that starts at an odd address
    out = torch.empty(n * s0 + 8, dtype=torch.uint8, device="cuda")
    p1, nb = ctx.pack_ragged(d[0], s0, flat[1:], n=n, lens_stride=F, out=out[3:])
    assert nb == sizes[0] and np.array_equal(p1.cpu().numpy(), want[:nb])


def test_pack_sizes_only_and_capacity_error(ctx):
    import ctypes as C
    import torch
    from tracy_amd import capi
    n, s = 40, 16
    lens = torch.arange(n, dtype=torch.int32, device="cuda") % (s + 1)
    buf = torch.arange(n * s, dtype=torch.int64, device="cuda").to(torch.uint8)
    total = int((torch.arange(n) % (s + 1)).sum())
    tot = C.c_uint64(0)
    lib = capi.lib()
    rc = lib.tracyhip_pack_ragged(ctx._h, C.c_void_p(buf.data_ptr()), C.c_uint64(s), C.c_uint32(1), C.c_void_p(lens.data_ptr()), C.c_uint32(1), C.c_uint32(n),
                                  None, C.c_uint64(0), C.byref(tot))
    assert rc == 0 and tot.value == total  # dst == NULL: the size only
    small = torch.empty(total - 1, dtype=torch.uint8, device="cuda")
    rc = lib.tracyhip_pack_ragged(ctx._h, C.c_void_p(buf.data_ptr()), C.c_uint64(s), C.c_uint32(1), C.c_void_p(lens.data_ptr()), C.c_uint32(1), C.c_uint32(n),
                                  C.c_void_p(small.data_ptr()), C.c_uint64(small.numel()), C.byref(tot))
    assert rc == capi.ERR_ARG
    assert tot.value == total


# ---- the shapes only large batches reach, at the smallest sizes that cross each boundary -----------------------------------------------
def _packed(ctx, kinds_np, n, out=None):
    """kinds_np: expect()'s list; the source tensors hold exactly n * stride elements"""
    import torch
    dev = []
    for buf, stride, lens, lens_stride in kinds_np:
        assert buf.size == n * stride
        dev.append((torch.from_numpy(buf).cuda(), stride, torch.from_numpy(np.ascontiguousarray(lens)).cuda(), lens_stride))
    packed, sizes = ctx.pack_ragged_multi(dev, n, out=out)
    return packed.cpu().numpy(), sizes, dev


def _kind_sizes(kinds_np, n):
    return [int(np.minimum(np.asarray(lens[:(n - 1) * ls + 1:ls], np.int64), stride).sum()) * buf.dtype.itemsize for buf, stride, lens, ls in kinds_np]


def test_pack_scan_serial_part_sixteen_kinds(ctx):
    """16 kinds x 17 000 regions: 16 x 67 = 1 072 scan workgroups, more than pack_top_kernel has threads -- every thread sums and
    rewrites a range of two, ranges straddle kind boundaries (67 is odd), and kind_end is written from inside a range.  Strides of
    1 .. 24 bytes, elements of 1 / 2 / 4 / 8 bytes, lengths out of a record array for some kinds, all-empty kinds, runs of 256 empty
    regions (whole scan workgroups that add nothing)."""
    rng = np.random.default_rng(16)
    n, F = 17000, 3
    shapes = [(np.uint8, 1), (np.uint8, 3), (np.int16, 1), (np.uint8, 7), (np.int32, 1), (np.int16, 5), (np.uint8, 13), (np.int64, 1),
              (np.int32, 3), (np.uint8, 24), (np.int16, 12), (np.int64, 2), (np.uint8, 5), (np.int32, 6), (np.int16, 3), (np.int64, 3)]
    assert sorted({np.dtype(t).itemsize for t, _ in shapes}) == [1, 2, 4, 8]
    assert all(1 <= np.dtype(t).itemsize * s <= 24 for t, s in shapes) and max(np.dtype(t).itemsize * s for t, s in shapes) == 24
    rec = np.zeros((n, F), np.int32)  # columns 0 and 2: the lengths of kinds 1 and 9
    kinds = []
    for k, (t, stride) in enumerate(shapes):
        buf = rng.integers(0, 256, size=n * stride * np.dtype(t).itemsize).astype(np.uint8).view(t)
        lens = rng.integers(0, stride + 2, size=n).astype(np.int32)  # (some beyond the stride: clamped)
        if k in (4, 15):  # all-empty kinds: one in the middle, and the last (its kind_end repeats the one before)
            lens[:] = 0
        if k in (0, 6, 11):  # whole scan workgroups of empty regions, the first and the last of a kind among them
            for blk in (0, 7, 8, 66):
                lens[256 * blk:256 * (blk + 1)] = 0
        if k == 1:
            rec[:, 0] = lens
            kinds.append((buf, stride, rec.reshape(-1), F))
        elif k == 9:
            rec[:, 2] = lens
            kinds.append((buf, stride, rec.reshape(-1)[2:], F))
        else:
            kinds.append((buf, stride, lens, 1))
    nw = len(shapes) * ((n + 255) // 256)
    assert nw == 1072 and (nw + 1023) // 1024 == 2
    want = expect(kinds, n)
    got, sizes, _ = _packed(ctx, kinds, n)
    assert sizes == _kind_sizes(kinds, n) and sizes[4] == 0 and sizes[15] == 0
    assert sum(sizes) == want.size and np.array_equal(got, want)


def test_pack_scan_serial_part_one_kind(ctx):
    """one kind of 262 400 regions: 1 025 scan workgroups -- threads 0 .. 511 take two each, thread 512 the last one alone, the other
    511 threads none"""
    rng = np.random.default_rng(17)
    n, stride = 262400, 8
    assert (n + 255) // 256 == 1025
    buf = rng.integers(0, 256, size=n * stride).astype(np.uint8)
    lens = rng.integers(0, stride + 1, size=n).astype(np.int32)
    want = expect([(buf, stride, lens, 1)], n)
    got, sizes, _ = _packed(ctx, [(buf, stride, lens, 1)], n)
    assert sizes == [want.size] and np.array_equal(got, want)


@pytest.mark.parametrize("dst_off", [0, 1, 2, 3])
def test_pack_long_regions_every_alignment(ctx, dst_off):
    """regions of 257 .. 1 100 bytes: two to five trips of a wave's 256-byte step, in both dword loops of pack_copy_kernel.  Strides
    = 0, 1, 2, 3 (mod 4), every tail length, the destination starting at offsets 0 .. 3: among the regions longer than 512 bytes every
    (destination head, source remainder) pair occurs.  One region is exactly head + 4 * 64 * 2 bytes (no tail), one is shorter than its head."""
    import torch
    rng = np.random.default_rng(40 + dst_off)
    n = 96
    strides = (1100, 1101, 1102, 1103)
    lens = [rng.integers(257, s + 1, size=n).astype(np.int32) for s in strides]
    for k in range(4):
        lens[k][:4] = 600 + 4 * np.arange(4) + np.arange(4)  # tails 0 .. 3 whatever the draw
    bufs = [rng.integers(0, 256, size=n * s).astype(np.uint8) for s in strides]
    cap = sum(n * s for s in strides)
    out = torch.empty(cap + 8, dtype=torch.uint8, device="cuda")[dst_off:]
    d0 = out.data_ptr()
    assert d0 % 4 == dst_off
    # region 40 of kind 0 ends on a dword and fills whole steps; 41 moves the next start to 1 (mod 4); 42 is shorter than its head of 3
    at = d0 + int(lens[0][:40].sum())
    head = (4 - at) & 3
    lens[0][40] = head + 4 * 64 * 2
    lens[0][41] = 301
    lens[0][42] = 2
    assert (4 - (at + int(lens[0][40]) + 301)) & 3 == 3
    kinds = [(bufs[k], strides[k], lens[k], 1) for k in range(4)]
    want = expect(kinds, n)
    got, sizes, dev = _packed(ctx, kinds, n, out=out)
    seen, at = set(), d0
    for k in range(4):
        s0 = dev[k][0].data_ptr()
        for i in range(n):
            ln = int(lens[k][i])
            head = (4 - at) & 3
            if ln > 512:
                seen.add((head, (s0 + i * strides[k] + head) & 3))
            at += ln
    assert len(seen) == 16, sorted(seen)
    assert {int(x) % 4 for x in np.concatenate(lens)} == {0, 1, 2, 3}
    assert sizes == _kind_sizes(kinds, n) and np.array_equal(got, want)


def test_pack_kind_limits(ctx):
    """16 payload kinds are taken, 17 are refused before anything is written, no regions give zeros"""
    import ctypes as C
    import torch
    from tracy_amd import capi
    n = 5
    src = torch.arange(n * 4, dtype=torch.int64, device="cuda").to(torch.uint8)
    lens = torch.tensor([4, 0, 3, 9, 1], dtype=torch.int32, device="cuda")
    want = expect([(src.cpu().numpy(), 4, lens.cpu().numpy(), 1)], n)
    packed, sizes = ctx.pack_ragged_multi([(src, 4, lens, 1)] * 16, n)
    assert sizes == [want.size] * 16 and np.array_equal(packed.cpu().numpy(), np.tile(want, 16))
    arr = (capi.RaggedSrc * 17)(*[capi.RaggedSrc(src.data_ptr(), 4, 1, lens.data_ptr(), 1) for _ in range(17)])
    out = torch.zeros(17 * n * 4, dtype=torch.uint8, device="cuda")
    kb = (C.c_uint64 * 17)(*([777] * 17))
    lib = capi.lib()
    rc = lib.tracyhip_pack_ragged_multi(ctx._h, arr, C.c_uint32(17), C.c_uint32(n), C.c_void_p(out.data_ptr()), C.c_uint64(out.numel()), kb)
    assert rc == capi.ERR_ARG
    assert list(kb) in ([777] * 17, [0] * 17) and int(out.sum()) == 0
    kb = (C.c_uint64 * 16)(*([777] * 16))
    rc = lib.tracyhip_pack_ragged_multi(ctx._h, arr, C.c_uint32(16), C.c_uint32(0), C.c_void_p(out.data_ptr()), C.c_uint64(out.numel()), kb)
    assert rc == capi.OK and list(kb) == [0] * 16 and int(out.sum()) == 0
