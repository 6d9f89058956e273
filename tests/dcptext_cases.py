"""Hand-made traces for tracyhip_render_decompositions and an independent restatement of what `tracy decompose` prints from the decompose
results: the .decomp table (decompose.h:622-632), the report tail of traceAlleleAlignJsonOut (json.h:327-381) and the record lines of
the VCF.  A case is the per-trace dict of hostlib.dcptext_pack with its own max_variants / max_text and qual_cut."""
import numpy as np

DECOMP, JSON, VCF = 0, 1, 2
FORMS = (DECOMP, JSON, VCF)
OK, DEFERRED, TOO_SMALL = 0, 1, 2
TILE = 256
QC = 45
VERSION = b"0.9.1"


def base(seed=0, n=120, cols=(40, 37, 33), rows=4, nvar=0, forward=True, trims=(0, 0), maxv=4, maxt=64, **kw):
    rng = np.random.default_rng(seed)
    row = lambda m: bytes(rng.choice(list(b"ACGT-"), size=m).tolist())
    c = dict(dcp=[(int(i) - rows // 2, int(rng.integers(0, 5000))) for i in range(rows)], rows=[(row(m), row(m)) for m in cols],
             bcpos=(7 + 12 * np.arange(n)).astype(np.int32), estqual=rng.integers(0, 62, n).astype(np.uint8), variants=[],
             ref_pos=(1000 + seed, 1003 + seed), forward=forward, score=(123, -45, 6), breakpoint=n // 3, indelshift=True,
             trim_left=trims[0], trim_right=trims[1], chr1=b"chr7", chr2=b"chr7", frac1=b"0.61", frac2=b"0.39", maxv=maxv, maxt=maxt, qc=QC)
    for j in range(nvar):
        c["variants"].append(dict(pos=5000 + 3 * j, basenum=2 + j, gt=1, ref=b"A", alt=b"G"))
    c.update(kw)
    return c


def call_index(c, basenum):
    tl, tr, n = c["trim_left"] & 0xffff, c["trim_right"] & 0xffff, len(c["bcpos"])
    return ((tl + basenum - 1) if c["forward"] else n - (tr + basenum)) & 0xffffffff


def basenum_for(c, q):
    """the basenum whose call index is q"""
    tl, tr, n = c["trim_left"] & 0xffff, c["trim_right"] & 0xffff, len(c["bcpos"])
    return q + 1 - tl if c["forward"] else n - tr - q


def records(c):
    """(var_n, [(pos, basenum, gt, ref_off, ref_len, alt_off, alt_len)], text) as hostlib.dcptext_pack lays a case out"""
    if "raw_records" in c:
        text = bytes(c.get("raw_text", b"")).ljust(c["maxt"], b"\0")
        return c["raw_var_n"], [(r[0], r[1], r[2], r[4], r[5], r[6], r[7]) for r in c["raw_records"]], text
    recs, text = [], b""
    for v in c["variants"]:
        recs.append((v["pos"], v["basenum"], v["gt"], len(text), len(v["ref"]), len(text) + len(v["ref"]), len(v["alt"])))
        text += v["ref"] + v["alt"]
    return len(recs), recs, text.ljust(c["maxt"], b"\0")


def unreadable(c, form):
    """the writers would index outside an array: neither the device nor the host prints the trace"""
    if form == DECOMP:
        return False
    n = len(c["bcpos"])
    if n == 0:
        return True
    if form == JSON and (((c["trim_left"] & 0xffff) + c["breakpoint"]) & 0xffffffff) >= n:
        return True
    nv, recs, _ = records(c)
    if nv > c["maxv"]:
        return True
    return any(call_index(c, r[1]) >= n or r[3] + r[4] > c["maxt"] or r[5] + r[6] > c["maxt"] for r in recs[:nv])


def is_deferred(c, form):
    if form == DECOMP:
        return False
    if unreadable(c, form) or len(c["chr1"]) > 65535:
        return True
    if form == VCF:
        return False
    return any(len(c[k]) > 65535 for k in ("chr2", "frac1", "frac2")) or any(len(r[0]) > (1 << 22) for r in c["rows"])


def viewport(c, q):
    centre, last = int(c["bcpos"][q]) + 1, int(c["bcpos"][-1])
    return (1 if centre <= 150 else centre - 150), (centre + 150 if centre + 150 < last else last)


def vtype(ref, alt):
    if len(ref) == 1 and len(alt) == 1:
        return b"SNV"
    return b"Deletion" if len(ref) > len(alt) else b"Insertion" if len(ref) < len(alt) else b"Complex"


def expected(c, form):
    """the text of a readable case"""
    num = lambda x: b"%d" % x
    if form == DECOMP:
        return b"indel\tdecomp\n" + b"".join(num(a) + b"\t" + num(b) + b"\n" for a, b in c["dcp"])
    qc = c["qc"] & 0xffff
    nv, recs, text = records(c)
    var = []
    for pos, basenum, gt, ro, rl, ao, al in recs[:nv]:
        q = call_index(c, basenum)
        var.append(dict(pos=pos, gt=gt, ref=text[ro:ro + rl], alt=text[ao:ao + al], q=q, estq=int(c["estqual"][q]), sig=int(c["bcpos"][q]) + 1))
    if form == VCF:
        out = b""
        for v in var:
            qual = 0 if (b"n" in v["alt"] or b"N" in v["alt"]) else v["estq"]
            gt = {0: b"0/0", 1: b"0/1", 2: b"1/1"}.get(v["gt"], b"./.")
            out += b"\t".join([c["chr1"], num(v["pos"]), b".", v["ref"], v["alt"], num(qual), b"LowQual" if qual < qc else b"PASS",
                               b"TYPE=" + vtype(v["ref"], v["alt"]) + b";METHOD=EMBL.TRACYv" + VERSION + b";BASEPOS=" + num(v["q"] + 1) + b";SIGNALPOS=" +
                               num(v["sig"]), b"GT:GQ", gt + b":" + num(v["estq"])]) + b"\n"
        return out
    lo, hi = viewport(c, ((c["trim_left"] & 0xffff) + c["breakpoint"]) & 0xffffffff)
    fw = b"1" if c["forward"] else b"0"
    out = b",\n\"chartConfig\": { \"x\": { \"axis\": { \"range\": [%d, %d] }}},\n" % (lo, hi)
    for k in range(2):
        n = num(k + 1)
        out += b"\"ref" + n + b"chr\": \"" + c["chr%d" % (k + 1)] + b"\",\n\"ref" + n + b"pos\": " + num((c["ref_pos"][k] + 1) & 0xffffffff) + b",\n"
        out += b"\"alt" + n + b"align\": \"" + c["rows"][k][0] + b"\",\n\"ref" + n + b"align\": \"" + c["rows"][k][1] + b"\",\n"
        out += b"\"ref" + n + b"forward\": " + fw + b",\n\"align" + n + b"score\": " + num(c["score"][k]) + b",\n"
    out += b"\"allele1fraction\": " + c["frac1"] + b",\n\"allele1align\": \"" + c["rows"][2][0] + b"\",\n"
    out += b"\"allele2fraction\": " + c["frac2"] + b",\n\"allele2align\": \"" + c["rows"][2][1] + b"\",\n"
    out += b"\"align3score\": " + num(c["score"][2]) + b",\n\"hetindel\": " + (b"1" if c["indelshift"] else b"0") + b",\n\"decomposition\": {\n"
    out += b"\"x\": [" + b", ".join(num(a) for a, _ in c["dcp"]) + b"],\n\"y\": [" + b", ".join(num(b) for _, b in c["dcp"]) + b"]\n},\n"
    out += b"\"variants\": {\n\"columns\": [\"chr\", \"pos\", \"id\", \"ref\", \"alt\", \"qual\", \"filter\", \"type\", \"genotype\", \"basepos\", \"signalpos\"],\n"
    rows = []
    for v in var:
        gt = {0: b"hom. REF", 1: b"het.", 2: b"hom. ALT"}.get(v["gt"], b"missing")
        rows.append(b"[\"" + c["chr1"] + b"\", " + num(v["pos"]) + b", \".\", \"" + v["ref"] + b"\", \"" + v["alt"] + b"\", " + num(v["estq"]) + b", " +
                    (b"\"LowQual\", " if v["estq"] < qc else b"\"PASS\", ") + b"\"" + vtype(v["ref"], v["alt"]) + b"\", \"" + gt + b"\", " +
                    num(v["q"] + 1) + b", " + num(v["sig"]) + b"]")
    out += b"\"rows\": [\n" + b",\n".join(rows) + b"],\n\"xranges\": [\n"
    out += b",\n".join(b"[%d, %d]" % viewport(c, v["q"]) for v in var) + b"]\n}\n}\n"
    return out


def crafted():
    """(name, case): what the writer can go wrong on, every case readable and answered by the device"""
    out = []
    add = lambda name, c: out.append((name, c))
    add("plain", base(1, nvar=2))
    add("table_empty", base(2, rows=0))
    add("table_maxindel1", base(3, rows=4))
    add("table_maxindel1000", base(4, rows=2002))
    add("table_negative", base(5, dcp=[(-1000, 0), (-2147483648, 2147483647), (-1, -1), (0, -2147483648)]))
    for rows in (TILE - 2, TILE - 1, TILE, TILE + 1):  # (a list section has rows + 1 items)
        add("table_rows%d" % rows, base(6, rows=rows))
    add("variants0", base(7, nvar=0))
    add("variants1", base(8, nvar=1))
    add("variants_max", base(9, nvar=4))
    add("variants_max_two_tiles", base(10, n=700, nvar=TILE + 3, maxv=TILE + 3, maxt=1024))
    types = [(b"A", b"G"), (b"ACG", b"A"), (b"A", b"ATT"), (b"AC", b"GT")]
    c = base(11, maxv=8, maxt=64)
    c["variants"] = [dict(pos=10 + i, basenum=3 + i, gt=gt, ref=r, alt=a) for i, ((r, a), gt) in enumerate(zip(types + types, (1, 2, 1, 2, 2, 1, 2, 1)))]
    add("types_and_genotypes", c)
    c = base(12, maxv=4)
    c["variants"] = [dict(pos=-5, basenum=3, gt=0, ref=b"A", alt=b"C"), dict(pos=7, basenum=4, gt=3, ref=b"A", alt=b"C"),
                     dict(pos=2147483647, basenum=5, gt=-1, ref=b"A", alt=b"C")]
    add("genotypes_outside", c)
    c = base(13, maxv=4)
    c["estqual"][:] = 60
    c["variants"] = [dict(pos=1, basenum=3, gt=1, ref=b"A", alt=b"AN"), dict(pos=2, basenum=4, gt=1, ref=b"A", alt=b"n"),
                     dict(pos=3, basenum=5, gt=1, ref=b"N", alt=b"C")]
    add("alt_with_N", c)
    c = base(14, maxv=4)
    c["estqual"][2:5] = (QC - 1, QC, QC + 1)
    c["variants"] = [dict(pos=1 + i, basenum=3 + i, gt=1, ref=b"A", alt=b"C") for i in range(3)]
    add("qual_around_the_cut", c)
    add("qual_cut_16_bits", dict(c, qc=65536 + QC))
    for fw in (True, False):
        for trims in ((0, 0), (50, 50)):
            c = base(15, n=160, forward=fw, trims=trims, maxv=4)
            c["variants"] = [dict(pos=100 + q, basenum=basenum_for(c, q), gt=1 + (q & 1), ref=b"C", alt=b"T") for q in (trims[0], 80, 159 - trims[1])]
            add("%s_trims%d" % ("forward" if fw else "reverse", trims[0]), c)
    c = base(16, trims=(65536 + 3, 65536 + 2), forward=False, maxv=2)
    c["variants"] = [dict(pos=1, basenum=basenum_for(c, 9), gt=1, ref=b"C", alt=b"T")]
    add("trims_16_bits", c)
    add("viewport_clamps_at_1", base(17, breakpoint=3, nvar=1))                      # centre 44
    add("viewport_clamps_at_lastpeak", base(18, n=120, breakpoint=117, nvar=0))      # centre + 150 beyond the last peak
    add("viewport_inside", base(19, n=400, breakpoint=200))
    c = base(20, n=60, breakpoint=59, maxv=2)
    c["variants"] = [dict(pos=1, basenum=60, gt=1, ref=b"C", alt=b"T"), dict(pos=2, basenum=1, gt=1, ref=b"C", alt=b"T")]
    add("last_and_first_call", c)
    add("cols0", base(21, cols=(0, 0, 0)))
    add("cols1", base(22, cols=(1, 1, 1)))
    add("cols_around_a_tile", base(23, cols=(TILE - 1, TILE, TILE + 1)))
    add("cols_tile_minus_2", base(24, cols=(TILE - 2, 2 * TILE - 1, 2 * TILE)))
    add("cols_long", base(25, cols=(1500, 1499, 1233)))
    add("names_empty", base(26, nvar=1, chr1=b"", chr2=b"", frac1=b"", frac2=b""))
    add("names_quotes", base(27, nvar=2, chr1=b"ch\"r\\1", chr2=b"\\\"", frac1=b"\"0.5\"", frac2=b"nan\\"))
    add("names_longest", base(28, nvar=1, chr1=b"c" * 65535, chr2=b"d" * 65535, frac1=b"1" * 65535, frac2=b"2" * 65535))
    add("ref_pos_wraps", base(29, ref_pos=(0xffffffff, 0x7fffffff)))
    add("ref_pos_large", base(30, ref_pos=(0xfffffffe, 0x80000000), score=(-2147483648, 2147483647, 0), indelshift=False))
    c = base(31, maxv=2, maxt=12)
    c["variants"] = [dict(pos=1, basenum=3, gt=1, ref=b"ACGTAC", alt=b"A"), dict(pos=9, basenum=9, gt=2, ref=b"T", alt=b"TGCA")]  # the region is full
    add("text_region_full", c)
    return out


def deferred():
    """(name, case): every rule of the deferral list"""
    out = []
    add = lambda name, c: out.append((name, c))
    add("chr1_over", base(40, nvar=1, chr1=b"x" * 65536))
    add("chr2_over", base(41, chr2=b"x" * 65536))
    add("frac1_over", base(42, frac1=b"1" * 65536))
    add("frac2_over", base(43, frac2=b"1" * 65536))
    add("no_basecalls", base(44, n=0, breakpoint=0))
    c = base(45, maxv=2)
    c["variants"] = [dict(pos=1, basenum=len(c["bcpos"]) + 1, gt=1, ref=b"A", alt=b"C")]
    add("call_index_at_bc_len", c)
    c = base(46, maxv=2, forward=False)
    c["variants"] = [dict(pos=1, basenum=0, gt=1, ref=b"A", alt=b"C")]
    add("call_index_at_bc_len_reverse", c)
    c = base(47, maxv=2, forward=False)
    c["variants"] = [dict(pos=1, basenum=len(c["bcpos"]) + 1, gt=1, ref=b"A", alt=b"C")]  # bc_len - (0 + bc_len + 1) wraps
    add("call_index_wraps", c)
    add("breakpoint_at_bc_len", base(48, n=100, breakpoint=100))
    add("breakpoint_plus_trim_at_bc_len", base(49, n=100, breakpoint=50, trims=(50, 0)))
    add("var_n_over", base(50, maxv=2, raw_var_n=3, raw_records=[(1, 2, 1, 0, 0, 1, 1, 1)] * 2, raw_text=b"AC"))
    add("var_n_huge", base(51, maxv=2, raw_var_n=0xffffffff, raw_records=[(1, 2, 1, 0, 0, 1, 1, 1)] * 2, raw_text=b"AC"))
    add("ref_leaves_region", base(52, maxv=2, maxt=16, raw_var_n=1, raw_records=[(1, 2, 1, 0, 10, 7, 0, 1)], raw_text=b"AC"))
    add("alt_leaves_region", base(53, maxv=2, maxt=16, raw_var_n=1, raw_records=[(1, 2, 1, 0, 0, 1, 16, 1)], raw_text=b"AC"))
    add("alt_offset_wraps", base(54, maxv=2, maxt=16, raw_var_n=2, raw_records=[(1, 2, 1, 0, 0, 1, 1, 1), (1, 2, 1, 0, 0, 1, 0xffffffff, 2)], raw_text=b"AC"))
    return out


def cols_over():
    """more than 2^22 columns in the alt-vs-alt rows (its own function: four million bytes a row)"""
    c = base(60, cols=(3, 3, (1 << 22) + 1))
    return "cols_over", c
