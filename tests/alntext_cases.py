"""Alignments for the tests of tracyhip_render_alignments (tests/test_emu_alntext.py on the host wave, tests/test_gpu_alntext.py on the device)
and an independent restatement of the three texts, written from the reference's fmindex.h:329-427 (plotAlignment), sage.h:328-339 (the
two-record FASTA) and json.h:205-215 (what traceAlignJsonOut prints behind the gapped trace) -- not from tracy_amd/host/sage_out.hpp.

An alignment is a dict: row0, row1 (bytes of one length), name0, name1 (bytes: the caller's text), pos (rs.pos), reflen
(rs.refslice.size()), forward, score.  key and linelimit belong to a job; the lists below carry them beside each alignment."""
import numpy as np

PLOT, FASTA, JSON = 0, 1, 2
FORMS = (PLOT, FASTA, JSON)
OK, DEFERRED, TOO_SMALL = 0, 1, 2
TILE = 256  # items per tile (alntext_wave.h kAlnTile; the emulator test checks it)
M32, M64 = 0xffffffff, 0xffffffffffffffff


def _i32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def _setw(n, w):
    return (b"%d" % n).rjust(w)  # (std::setw never cuts)


def expected(c, form, key=0, linelimit=60):
    r0, r1, cols = c["row0"], c["row1"], len(c["row0"])
    pos = c["pos"] & M32  # (uint32_t pos)
    if form == FASTA:
        return b">" + c["name0"] + b"\n" + r0 + b"\n>" + c["name1"] + (b" (forward)" if c["forward"] else b" (reverse)") + b"\n" + r1 + b"\n"
    if form == JSON:
        return (b",\n\"refchr\": \"" + c["name1"] + b"\",\n\"refpos\": " + b"%d" % ((pos + 1) & M32) + b",\n\"altalign\": \"" + r0 +
                b"\",\n\"refalign\": \"" + r1 + b"\",\n\"forward\": " + (b"1" if c["forward"] else b"0") + b"\n}\n")
    fald = linelimit + 14
    out = []

    def ungapped(row):  # a letter, a newline behind every fald-th; a closing newline unless the letters fill their last line
        s = row.replace(b"-", b"")
        for k in range(0, len(s), fald):
            out.append(s[k:k + fald])
            if len(s) - k >= fald:
                out.append(b"\n")
        if len(s) % fald:
            out.append(b"\n")

    rule = b"#" + b"-" * (fald - 1) + b"\n"
    out.append(c["name0"] + b"\n")
    ungapped(r0)
    out.append(c["name1"] + b"\n")
    ungapped(r1)
    out.append(b"\nAlignment score: %d\n" % c["score"] + rule + b"\n")
    ri, vi, blocks = _i32(pos + 1), 1, 0
    for s in range(0, cols, linelimit):
        a, b = r0[s:s + linelimit], r1[s:s + linelimit]
        out.append((b"Alt" + _setw(vi, 10) if key != 3 else b"Alt1" + _setw(vi, 9)) + b" " + a + b"\n")
        out.append(b" " * 14 + bytes(0x7c if x == y else 0x20 for x, y in zip(a, b)) + b"\n")
        if key == 3:
            lab = b"Alt2" + _setw(ri, 9)
        elif c["forward"]:
            lab = b"Ref" + _setw(ri, 10)
        else:  # rs.pos + rs.refslice.size() - (ri - rs.pos) + 1: uint32 - in the bracket, size_t outside
            lab = b"Ref" + _setw((pos + c["reflen"] - ((ri - pos) & M32) + 1) & M64, 10)
        out.append(lab + b" " + b + b"\n\n")
        vi += len(a) - a.count(b"-")
        ri = _i32(ri + len(b) - b.count(b"-"))
        blocks += 1
    out.append(b"\n" * (4 * (6 - blocks)) if blocks < 6 else b"")
    out.append(rule + rule + b"\n\n")
    return b"".join(out)


def is_deferred(c, form, key=0):
    """the answered domain as the issue states it"""
    cols = len(c["row0"])
    if cols > 1 << 22 or len(c["name1"]) > 65535 or (form != JSON and len(c["name0"]) > 65535):
        return True
    if c["pos"] < 0 or c["pos"] + max(c["reflen"], cols) + 1 >= 1 << 31:
        return True
    if form == PLOT and not c["forward"] and key != 3:
        return cols - c["row1"].count(b"-") > c["reflen"]
    return False


def make(cols, seed=0, gaps0=0.1, gaps1=0.1, pos=0, reflen=None, forward=1, score=100, name0=b">Alt", name1=b">Ref chr1:1-100 forward",
         row0=None, row1=None):
    rng = np.random.default_rng(1000 + seed)

    def row(g):
        a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, cols)].copy()
        a[rng.random(cols) < g] = 0x2d
        return a.tobytes()

    r0 = row(gaps0) if row0 is None else row0
    r1 = row(gaps1) if row1 is None else row1
    if row0 is None and row1 is None and cols:
        k = rng.integers(0, cols, max(cols // 2, 1))  # half of the columns match
        a, b = np.frombuffer(r0, np.uint8).copy(), np.frombuffer(r1, np.uint8)
        a[k] = b[k]
        r0 = a.tobytes()
    letters1 = len(r1) - r1.count(b"-")
    return dict(row0=r0, row1=r1, name0=name0, name1=name1, pos=pos, reflen=letters1 if reflen is None else reflen, forward=forward, score=score)


def crafted():
    """[(name, key, linelimit, alignment)]: the smallest shapes at which the bodies can go wrong"""
    out = []
    add = lambda name, key, L, c: out.append((name, key, L, c))
    for cols in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
        add("cols%d" % cols, 0, 60, make(cols, seed=cols))
    for L in (1, 7, 50, 60, 256, 65535):
        add("line%d" % L, 0, L, make(300, seed=L))
        for d in (-1, 0, 1):
            if 0 < L + d <= 1100:
                add("line%d_cols%+d" % (L, d), 0, L, make(L + d, seed=L + d))
    for blocks, cols in ((5, 45), (6, 60), (7, 61)):  # the spacer's edge
        add("blocks%d" % blocks, 0, 10, make(cols, seed=blocks))
    add("row0_gaps_only", 0, 60, make(130, row0=b"-" * 130, gaps1=0.0))
    add("row1_gaps_only", 1, 60, make(130, row1=b"-" * 130, gaps0=0.0))
    add("both_gaps_only", 0, 7, make(70, row0=b"-" * 70, row1=b"-" * 70))
    fald = 7 + 14
    for k in (0, fald - 1, fald, fald + 1, 2 * fald):  # letters of an ungapped row around its line length
        r0 = (b"-" * 3 + b"A") * k + b"-" * 5
        add("letters%d" % k, 0, 7, make(len(r0), seed=k, row0=r0, gaps1=0.3))
        add("letters%d_row1" % k, 2, 7, make(len(r0), seed=k, row1=r0, gaps0=0.0))
    # counters: linelimit 1 makes every column a block, 9 items each: block 256 starts tile 9
    add("counters_1_to_1100", 0, 1, make(1100, seed=1, gaps0=0.0, gaps1=0.0))                    # 9->10, 99->100, 999->1000 inside tiles
    add("counter_1000_at_a_tile_start", 0, 1, make(300, seed=2, gaps0=0.0, gaps1=0.0, pos=743))  # block 256: ri = 743 + 1 + 256
    add("counter_10_at_a_tile_start", 3, 1, make(300, seed=3, row0=b"-" * 247 + b"ACGTACGTA" + b"C" * 44, gaps1=0.0))  # block 256: vi = 10
    add("counter_1000_at_a_block_start", 0, 60, make(130, seed=4, gaps1=0.0, pos=939))           # block 1: ri = 939 + 1 + 60
    add("counter_100_at_a_block_start", 1, 50, make(130, seed=5, gaps1=0.0, pos=49))
    add("mirrored_120_to_1", 0, 1, make(120, seed=6, gaps1=0.0, forward=0))                      # 100->99 and 10->9
    add("mirrored_blocks", 2, 60, make(160, seed=7, gaps1=0.0, forward=0, pos=5, name1=b">Ref chr2:6-165 reversecomplement"))
    add("mirrored_with_gaps", 1, 7, make(257, seed=8, gaps1=0.4, forward=0, pos=90))
    add("mirrored_reflen_longer", 0, 50, make(99, seed=9, forward=0, reflen=1000, pos=7))
    add("mirrored_key3_is_not_mirrored", 3, 50, make(99, seed=9, forward=0, reflen=1, pos=7))
    add("pos_fills_setw10", 0, 60, make(130, seed=10, pos=1_000_000_000))
    add("pos_fills_setw10_mirrored", 0, 60, make(130, seed=11, pos=1_000_000_000, forward=0))
    add("pos_overflows_setw9", 3, 60, make(130, seed=12, pos=1_000_000_000))
    add("pos_crosses_setw9", 3, 7, make(50, seed=13, gaps1=0.0, pos=999_999_980))               # labels of 14 and of 15 bytes in one text
    add("pos_largest", 0, 60, make(100, seed=14, pos=(1 << 31) - 1 - 100 - 1 - 1))
    for sc in (0, -1, -(1 << 31), (1 << 31) - 1):
        add("score%d" % sc, 0, 60, make(65, seed=15, score=sc))
    for key in (0, 1, 2, 3):
        for fw in (0, 1):
            add("key%d_forward%d" % (key, fw), key, 60, make(257, seed=20 + 2 * key + fw, forward=fw, pos=33,
                                                           name0=b">Alt1 (Estimated allelic Fraction: 0.437)" if key else b">Alt"))
    add("empty_names", 0, 60, make(65, seed=30, name0=b"", name1=b""))
    add("names_of_300", 0, 60, make(65, seed=31, name0=b">" + b"n" * 299, name1=bytes(33 + i % 90 for i in range(300))))
    add("name_bytes", 0, 60, make(10, seed=32, name0=b"a\"b\\c\n\x80", name1=b"\x00\xff"))
    odd = b"A\"C\\G\nT\x80-\x00" * 7
    add("row_bytes", 0, 7, make(len(odd), seed=33, row0=odd, row1=odd[::-1]))
    add("name_of_65535", 0, 60, make(65, seed=34, name1=b"x" * 65535))
    add("cols_20000", 0, 256, make(20000, seed=35, gaps1=0.3, forward=0))  # 79 column tiles in front of the last anchor: two steps of their sum
    return out


def deferred():
    """[(name, key, linelimit, alignment)]: one alignment per condition under which the device does not answer"""
    return [
        ("cols_over", 0, 65535, make((1 << 22) + 1, seed=40)),
        ("name0_over", 0, 60, make(65, seed=41, name0=b"y" * 65536)),
        ("name1_over", 0, 60, make(65, seed=42, name1=b"z" * 65536)),
        ("pos_negative", 0, 60, make(65, seed=43, pos=-1)),
        ("pos_plus_reflen_over", 0, 60, make(20, seed=44, pos=(1 << 31) - 40, reflen=100)),
        ("pos_plus_cols_edge", 0, 60, make(100, seed=45, gaps1=1.0, pos=(1 << 31) - 1 - 100)),  # pos + cols + 1 = 2^31 (row 1 has no letter: no counter moves)
        ("mirrored_row1_longer", 0, 60, make(65, seed=46, gaps1=0.0, forward=0, reflen=64)),
        ("mirrored_row1_longer_late", 2, 7, make(1025, seed=47, gaps1=0.0, forward=0, reflen=1024)),
    ]


def largest():
    """the most columns the device answers (device only: the host wave would take hours)"""
    return ("cols_4194304", 2, 65535, make(1 << 22, seed=36, gaps0=0.2, gaps1=0.2, forward=0, pos=11))


def random_cases(n=200, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    lines = (1, 7, 50, 60, 256)
    for i in range(n):
        cols = int(rng.integers(0, 601))
        key, L = int(rng.integers(0, 4)), int(lines[int(rng.integers(0, len(lines)))])
        c = make(cols, seed=5000 + i, gaps0=float(rng.random()) * 0.5, gaps1=float(rng.random()) * 0.5, pos=int(rng.integers(0, 2000)) if i % 5 else int(rng.integers(0, 1 << 30)),
                 forward=int(rng.integers(0, 2)), score=int(rng.integers(-5000, 5000)), name0=b">Alt%d" % i, name1=b">Ref c:%d" % i)
        c["reflen"] += int(rng.integers(0, 3))
        out.append(("random%d" % i, key, L, c))
    return out


def jobs(items):
    """the alignments of a list grouped by (key, linelimit) in their order: {(key, linelimit): [(name, alignment)]}"""
    g = {}
    for name, key, L, c in items:
        g.setdefault((key, L), []).append((name, c))
    return g


def pack(cs):
    """alignments as the arguments of hostlib.alntext_pack / capi.PreparedAlnText"""
    return dict(rows0=[c["row0"] for c in cs], rows1=[c["row1"] for c in cs], name0=[c["name0"] for c in cs], name1=[c["name1"] for c in cs],
                ref_pos=[c["pos"] for c in cs], ref_len=[c["reflen"] for c in cs], forward=[c["forward"] for c in cs], score=[c["score"] for c in cs])


def revcomp_rule(ref):
    """reverseComplement, fmindex.h:11-25: the upper-cased reversed string is complemented into the sequence; at a letter outside ACGTN
    nothing is assigned, so that place keeps the byte the sequence had there"""
    comp = {65: 84, 67: 71, 71: 67, 84: 65, 78: 78}
    out = bytearray(ref)
    n = len(ref)
    for i in range(n):
        ch = ref[n - 1 - i]
        up = ch - 32 if 97 <= ch <= 122 else ch
        if up in comp:
            out[i] = comp[up]
    return bytes(out)
