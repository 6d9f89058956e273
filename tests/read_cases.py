"""File images for the tests of tracyhip_read_traces (tests/test_emu_read.py on the host wave, tests/test_gpu_read.py on the device): a small
ABIF composer that places every payload at a chosen byte offset -- the project's own writer cannot -- an SCF v3 writer for any 16-bit
second differences, and the named cases.  What a case must give is what hostlib.read_trace gives for the same bytes (expected())."""
import base64
import json
import os
import struct
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OK, DEFERRED, TOO_SMALL = 0, 1, 2
ABIF_TILE, SCF_TILE = 512, 256  # samples per emit tile / per step of an SCF channel (read_wave.h; the emulator test checks them)


def slot(name, number, etype, esize, payload, count=None, dsize=None, lead=0, offset=None):
    """one directory slot.  count / dsize default to what the payload has; lead: junk bytes in front of the payload in the data area (its
    byte offset mod 4); offset: the offset field as given, whatever the payload is"""
    payload = bytes(payload)
    return dict(name=name, number=number, etype=etype, esize=esize, payload=payload, count=len(payload) // esize if count is None else count,
                dsize=len(payload) if dsize is None else dsize, lead=lead, offset=offset)


def compose(slots, dir_first=False, nslots=None, tail=b""):
    """an ABIF image: 128-byte header, then the data area and the directory (dir_first: the directory, then the data area, so the last
    payload ends the file).  A payload lives in its slot iff the slot's dsize is <= 4."""
    dir_at = 128 if dir_first else None
    cursor = 128 + (28 * len(slots) if dir_first else 0)
    data = b""
    where = []
    for s in slots:
        if s["dsize"] <= 4 or s["offset"] is not None:
            where.append(None)
            continue
        data += b"\xa5" * s["lead"]
        cursor += s["lead"]
        where.append(cursor)
        data += s["payload"]
        cursor += len(s["payload"])
    if dir_at is None:
        dir_at = cursor
    d = b""
    for s, at in zip(slots, where):
        d += struct.pack(">4sihhii", s["name"], s["number"], s["etype"], s["esize"], s["count"], s["dsize"])
        if s["offset"] is not None:
            d += struct.pack(">i", s["offset"])
        elif at is None:
            d += s["payload"][:4].ljust(4, b"\0")
        else:
            d += struct.pack(">i", at)
        d += struct.pack(">i", 0)
    head = struct.pack(">4sh4sihhiiii", b"ABIF", 101, b"tdir", 1, 1023, 28, len(slots) if nslots is None else nslots, 28 * len(slots), dir_at, 0)
    head = head.ljust(128, b"\0")
    return head + (d + data if dir_first else data + d) + tail


def be16(a):
    return np.asarray(a).astype(">i2").tobytes()


def std_slots(sig, pos, pbas, pcon, p2ba=None, order=b"GATC", leads=(0, 0, 0, 0), ploc_lead=0):
    """the tags readab uses for a trace: sig [4][ns] in A, C, G, T order, written in dye order"""
    out = []
    for i in range(4):
        out.append(slot(b"DATA", 9 + i, 4, 2, be16(sig[b"ACGT".index(order[i:i + 1])]), lead=leads[i]))
    out.append(slot(b"FWO_", 1, 2, 1, order))
    out.append(slot(b"PLOC", 2, 4, 2, be16(pos), lead=ploc_lead))
    out.append(slot(b"PBAS", 2, 2, 1, pbas))
    if p2ba is not None:
        out.append(slot(b"P2BA", 1, 2, 1, p2ba))
    out.append(slot(b"PCON", 2, 2, 1, bytes(pcon)))
    return out


def rand_trace(rng, ns, nb, letters=b"ACGT"):
    sig = rng.integers(-300, 3000, size=(4, ns)).astype(np.int32)
    sig[:, 0] = [-32768, 32767, -1, 0]
    pos = np.sort(rng.choice(np.arange(ns), size=min(nb, ns), replace=False)).astype(np.int32)
    nb = len(pos)
    return sig, pos, bytes(rng.choice(list(letters), size=nb).tolist()), rng.integers(0, 62, size=nb).astype(np.uint8)


def scf3(raw, pos, version=b"3.00", lead=0):
    """an SCF v3 image from the stored second differences raw [4][ns] (any 16-bit words); lead: junk bytes in front of the samples"""
    raw = np.asarray(raw)
    ns, nb = raw.shape[1], len(pos)
    samples_at = 128 + lead
    bases_at = samples_at + 8 * ns
    head = struct.pack(">4s8I4sI", b".scf", ns, samples_at, nb, 0, 0, bases_at, 0, 0, version, 2).ljust(128, b"\0")
    return head + b"\x5a" * lead + b"".join((raw[c].astype(np.int64) & 0xFFFF).astype(">u2").tobytes() for c in range(4)) + np.asarray(pos).astype(">i4").tobytes()


def scf_of_trace(sig, pos, **kw):
    """... from the samples the reader must give back (every value of both integrations inside 16 bits or not: the words wrap)"""
    d = np.asarray(sig).astype(np.int64)
    for _ in range(2):
        d = np.diff(np.concatenate([np.zeros((4, 1), np.int64), d], axis=1), axis=1)
    return scf3(d, pos, **kw)


def scf_integrate(raw):
    """what readscf makes of the stored words raw [ns] (trace_io.hpp:205-216), and how often the carry of each pass wrapped"""
    def wrap(x):
        return (int(x) + 32768) % 65536 - 32768
    v, wraps = [wrap(x) for x in raw], []
    for _ in range(2):
        carry, n = 0, 0
        for k in range(len(v)):
            v[k] += carry
            carry = wrap(v[k])
            n += carry != v[k]
        wraps.append(n)
    return np.array(v, np.int64), wraps


def scf_crossing_words(rng, ns):
    """stored words whose first running sum (the step from sample to sample) keeps leaving 16 bits while every sample stays inside:
    steps of more than 32767 up and down.  A step v needs v - carry inside 16 bits, so it is picked among those that are."""
    raw, w, c1 = [], 0, 0
    for _ in range(ns):
        lo, hi = max(c1 - 32768, -32768 - w), min(c1 + 32767, 32767 - w)  # (never empty: both ranges are 65536 wide around 16-bit centres)
        jitter = int(rng.integers(0, 3000))
        v = max(lo, min(hi, hi - jitter if abs(hi) >= abs(lo) else lo + jitter))
        raw.append(v - c1)
        w += v
        c1 = (v + 32768) % 65536 - 32768
    return np.array(raw, np.int64)


def answered():
    """(name, image) of the files the device must answer.  The cases of tests/test_trace_io.py (abif_cases) and the golden files come
    with abif_cases_images() / golden_images()."""
    rng = np.random.default_rng(20240)
    out = []
    for r in range(4):  # channel payloads beginning at each byte offset mod 4 (the image's own offset is the runner's)
        sig, pos, pri, q = rand_trace(rng, 600, 40)
        img = compose(std_slots(sig, pos, pri, q, leads=(r, 0, 0, 0), ploc_lead=(r + 1) % 4))
        assert struct.unpack(">i", img[img.index(b"DATA") + 20:][:4])[0] % 4 == r
        out.append(("chan_mod%d" % r, img))
    for ns in (3, 63, 64, 65, ABIF_TILE - 1, ABIF_TILE, ABIF_TILE + 1, 2 * ABIF_TILE + 9):
        sig, pos, pri, q = rand_trace(rng, ns, 20)
        out.append(("abif_ns%d" % ns, compose(std_slots(sig, pos, pri, q, order=b"TCAG", leads=(1, 2, 3, 0)))))
    sig, pos, pri, q = rand_trace(rng, 50, 2)
    # two calls: PLOC (4 bytes) and PBAS (2 bytes) live in their slots, and the byte past PBAS is the slot's next byte ('G': a third call
    # as far as PBAS goes; the other lengths cut it)
    s = std_slots(sig, pos, b"AC", q)
    s[6] = slot(b"PBAS", 2, 2, 1, b"ACG", count=2, dsize=2)
    out.append(("two_calls_in_slots", compose(s)))
    sig, pos, pri, q = rand_trace(rng, 70, 9)
    s = std_slots(sig, pos, pri, q)
    s = [x for x in s if x["name"] != b"PBAS"] + [s[6]]  # PBAS's payload is the last of the data area and the file: no byte past it
    img = compose(s, dir_first=True)
    assert img.endswith(pri)
    out.append(("pbas_ends_the_file", img))
    sig, pos, pri, q = rand_trace(rng, 90, 12)
    out.append(("p2ba_absent", compose(std_slots(sig, pos, pri, q))))
    out.append(("p2ba_one_shorter", compose(std_slots(sig, pos, pri, q, p2ba=bytes(rng.choice(list(b"ACGTK"), size=11).tolist())))))
    out.append(("more_qualities_than_calls", compose(std_slots(sig, pos, pri, list(q) + [7, 8, 9], p2ba=pri[::-1]))))
    sig, pos, pri, q = rand_trace(rng, 90, 30, letters=b"ACGTNRY")
    out.append(("primaries_with_N_R_Y", compose(std_slots(sig, pos, pri[:3] + b"NRY" + pri[6:], q, p2ba=b"acgtKM" + pri[6:]))))
    # more than 64 slots: the wanted tags spread over a directory of 150, unrelated tags (and look-alikes) between them
    sig, pos, pri, q = rand_trace(rng, 130, 15)
    want = std_slots(sig, pos, pri, q, p2ba=pri)
    s = []
    for i in range(150):
        if i % 16 == 5 and want:
            s.append(want.pop(0))
        elif i % 7 == 0:
            s.append(slot(b"DATA", 1 + i % 8, 4, 2, be16(rng.integers(0, 99, 6))))  # DATA.1 .. 8: the raw channels, not wanted
        elif i % 7 == 1:
            s.append(slot(b"PBAS", 1, 2, 1, b"TTTTTTTT"))
        else:
            s.append(slot(b"CMNT", i, 18, 1, b"\x05hello"))
    s += want
    assert not [x for x in s[:64] if x["name"] == b"PCON"] and len(s) > 128
    out.append(("directory_of_150_slots", compose(s)))
    # a wanted name under an element type the reader skips (18, a Pascal string) next to the real one; and under a type it reads the
    # others by (PLOC.2 as characters): ignored too
    s = std_slots(sig, pos, pri, q)
    s.insert(0, slot(b"PBAS", 2, 18, 1, b"\x04GGGG"))
    s.insert(3, slot(b"PLOC", 2, 2, 1, b"junkjunk"))
    s.append(slot(b"DATA", 9, 5, 4, bytes(16)))
    out.append(("wanted_name_skipped_type", compose(s)))
    # SCF v3
    for ns in (3, 63, 64, 65, SCF_TILE - 1, SCF_TILE, SCF_TILE + 1, 3 * SCF_TILE + 5):
        sig, pos, _, _ = rand_trace(rng, ns, 10)
        out.append(("scf_ns%d" % ns, scf_of_trace(sig // 4, pos, lead=ns % 4)))
    # running sums that cross +-32768 in both passes while every sample stays inside int16: large steps up and down
    ns = 2 * SCF_TILE + 40
    raw = np.stack([scf_crossing_words(rng, ns) for _ in range(4)])
    img = scf3(raw, np.arange(5, 105, 10))
    for c in range(4):  # the first pass's carry wraps again and again, the samples stay inside 16 bits
        w, wraps = scf_integrate(raw[c])
        assert wraps[0] > 50 and wraps[1] == 0 and np.abs(w).max() <= 32767, c
    out.append(("scf_sums_cross_16_bits", img))
    return out


def scf_wide():
    """an SCF file whose integrated values leave int16 (the carry wraps, the value does not): answered with sample_bytes 4, DEFERRED with 2"""
    raw = np.zeros((4, 300), np.int64)
    raw[0, :] = 30000   # v = raw + wrap16(sum): reaches 30000 + 32767
    raw[1, 0] = -32768
    raw[1, 1:] = -20000
    raw[2, 290:] = 32767  # only the last step of the walk leaves the range
    raw[3, :] = 5
    w, wraps = scf_integrate(raw[0])  # the carries of both passes wrap, and the value needs more than 16 bits
    assert wraps[0] > 0 and wraps[1] > 0 and np.abs(w).max() > 32767
    assert np.abs(scf_integrate(raw[2])[0][:290]).max() <= 32767 < np.abs(scf_integrate(raw[2])[0]).max()
    return "scf_leaves_int16", scf3(raw, np.arange(0, 300, 30))


def deferred():
    """(name, image) of the files the device must defer -- exactly these; the host reader then refuses or reads them"""
    rng = np.random.default_rng(7)
    sig, pos, pri, q = rand_trace(rng, 80, 10)
    good = std_slots(sig, pos, pri, q)
    out = [("junk_bytes", b"JUNK" + bytes(200))]
    out.append(("abif_without_basecalls", compose(std_slots(sig, pos[:0], b"", q[:0]))))
    out.append(("directory_past_the_file", compose(good, nslots=len(good) + 3)))
    s = [dict(x) for x in good]
    s[2]["count"] = 5000
    s[2]["dsize"] = 10000
    out.append(("channel_past_the_file", compose(s)))
    out.append(("repeated_data9", compose(good + [good[0]])))
    s = [dict(x) for x in good]
    s[1] = slot(b"DATA", 10, 4, 2, be16(sig[0][:79]))
    out.append(("channels_of_unequal_counts", compose(s)))
    out.append(("fwo_not_a_permutation", compose(std_slots(sig, pos, pri, q, order=b"GATC")[:4] + [slot(b"FWO_", 1, 2, 1, b"GATT")] + good[5:])))
    out.append(("scf_version_2", scf_of_trace(sig, pos, version=b"2.00")))
    return out


def abif_cases_images():
    """the five files of tests/test_trace_io.py abif_cases (all four dye orders, negative samples, in-slot payloads)"""
    from test_trace_io import abif_cases
    with tempfile.TemporaryDirectory() as tmp:
        return [("abif_case%d" % i, open(p, "rb").read()) for i, p in enumerate(abif_cases(np.random.default_rng(41), tmp))]


def golden_images():
    """(name, image, the reference's stored answer) of tests/golden/trace_io.json["abif"]"""
    out = []
    for i, c in enumerate(json.load(open(os.path.join(HERE, "golden", "trace_io.json")))["abif"]):
        want = dict(format=0, signal=np.array(c["signal"], np.int32).reshape(4, -1), basecallpos=np.array(c["basecallpos"], np.int32),
                    basecalls1=base64.b64decode(c["basecalls1_b64"]), basecalls2=base64.b64decode(c["basecalls2_b64"]),
                    qual=np.array(c["qual"], np.uint8))
        out.append(("golden%d" % i, base64.b64decode(c["file_b64"]), want))
    return out


def expected(images):
    """hostlib.read_trace of every image (None: the reader refuses it)"""
    from tracy_amd import hostlib
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, img in enumerate(images):
            p = os.path.join(tmp, "f%d" % i)
            with open(p, "wb") as fh:
                fh.write(img)
            out.append(hostlib.read_trace(p))
    return out


def same(got, want):
    """a device result (hostlib.read_unpack fields) against read_trace's, field by field; returns the first field that differs or None"""
    if got["format"] != want["format"]:
        return "format"
    for k in ("signal", "basecallpos", "qual"):
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)) or np.asarray(got[k]).shape != np.asarray(want[k]).shape:
            return k
    for k in ("basecalls1", "basecalls2"):
        if bytes(got[k]) != bytes(want[k]):
            return k
    return None
