"""Crafted inputs for the SAM / FASTQ text tests (the CPU model test, the host program and the GPU tests share
them): the smallest shapes at which the kernels of csrc/sam.hip can go wrong.  A case is (refs, records)."""
from __future__ import annotations

import random
import struct

import bamutil

# csrc/sam.hip: a wave of the emit kernel takes WAVE_RECS consecutive records, a workgroup BLOCK_RECS
# (tests/test_gpu_view.py checks both against the library's counters)
WAVE_RECS, BLOCK_RECS = 4, 16
REFS = [("c", 1 << 29), ("chr2", 1 << 29), ("L" * 200, 1 << 29)]
NAMES = [n for n, _ in REFS]
SIZES = (0, 1, 63, 64, 65, 257, BLOCK_RECS + 1, WAVE_RECS + 1)
TRIMS = ((0, 0), (3, 0), (0, 4), (5, 5))


def rec(name=b"r", flag=0, refid=0, pos=100, mapq=60, cigar=(), codes=(), qual=None, mref=-1, mpos=-1, tlen=0, tags=b"") -> bytes:
    """A record from raw parts: cigar = [(length, op code)], codes = one 4-bit base code per base."""
    lseq = len(codes)
    sb = bytearray((lseq + 1) // 2)
    for i, c in enumerate(codes):
        sb[i // 2] |= (c & 15) << (0 if i & 1 else 4)
    if qual is None:
        qual = bytes((i * 7 + 3) % 94 for i in range(lseq))
    assert len(qual) == lseq
    nm = bytes(name) + b"\0"
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(nm), mapq, 4680, len(cigar), flag, lseq, mref, mpos, tlen)
    body += nm + b"".join(struct.pack("<I", (ln << 4) | op) for ln, op in cigar) + bytes(sb) + bytes(qual) + tags
    return struct.pack("<I", len(body)) + body


def codes_of(n: int, k: int = 0) -> list[int]:
    return [(i * 5 + k) % 16 for i in range(n)]


def basic(i: int) -> bytes:
    n = 30 + i % 9
    return rec(b"read%d" % i, flag=(0x41 if i % 2 else 0x10), refid=i % 2, pos=1000 + 17 * i, mapq=i % 61, cigar=[(n, 0)], codes=codes_of(n, i),
               mref=i % 2 if i % 2 else -1, mpos=1200 + i, tlen=(200 + i) * (-1 if i % 4 == 1 else 1),
               tags=tag("NM", "C", i % 200) + tag("RG", "Z", b"grp%d" % (i % 3)))


def tag(name: str, typ: str, value) -> bytes:
    h = name.encode() + typ.encode()
    if typ == "A":
        return h + bytes([value])
    if typ in "ZH":
        return h + bytes(value) + b"\0"
    if typ == "B":
        sub, vals = value
        return h + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i",
                                                                                         "I": "<I", "f": "<f"}[sub], v) for v in vals)
    if typ == "f" and isinstance(value, bytes):
        return h + value
    return h + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[typ], value)


INT_EXTREMES = {"c": (-128, -1, 0, 127), "C": (0, 9, 10, 255), "s": (-32768, -1, 0, 32767), "S": (0, 99, 100, 65535),
                "i": (-(1 << 31), -1, 0, (1 << 31) - 1), "I": (0, 999_999_999, 1_000_000_000, (1 << 32) - 1)}
FLOATS = (1.0, 0.1, 1e-5, 123456.7, 1e10, -0.0, float("inf"), float("-inf"), struct.pack("<I", 0x7FC00000), struct.pack("<I", 0xFFC00000))


def width_records() -> list[bytes]:
    out = []
    for f in (0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535):
        out.append(rec(b"f%d" % f, flag=f, codes=codes_of(5)))
    for p in (-1, 0, 8, 9, 98, 99, 998, 999, 99_999_998, 99_999_999, 999_999_998, 999_999_999, (1 << 31) - 2):
        out.append(rec(b"p%d" % (p + 1), pos=p, flag=1, mref=0, mpos=p, codes=codes_of(4)))
    for q in (0, 9, 10, 99, 100, 255):
        out.append(rec(b"q%d" % q, mapq=q, codes=codes_of(3)))
    for t in (0, 9, -9, 10, -10, 99, -100, 123456, -1234567, (1 << 31) - 1, -(1 << 31)):
        out.append(rec(b"t", flag=3, refid=1, mref=1, mpos=5, tlen=t, codes=codes_of(6)))
    return out


def ref_records() -> list[bytes]:
    c = codes_of(7)
    return [rec(b"a", refid=-1, pos=-1, codes=c), rec(b"b", refid=len(REFS), codes=c), rec(b"b2", refid=len(REFS) + 5, codes=c),
            rec(b"c", flag=0, refid=0, mref=1, mpos=77, tlen=55, codes=c),           # unpaired, mate fields set
            rec(b"d", flag=1, refid=1, mref=1, mpos=77, tlen=-55, codes=c),          # same contig
            rec(b"e", flag=1, refid=1, mref=0, mpos=0, tlen=5, codes=c),             # another contig, 1 character
            rec(b"f", flag=1, refid=0, mref=2, mpos=9, tlen=5, codes=c),             # ... 200 characters
            rec(b"g", flag=1, refid=2, mref=-1, mpos=-1, codes=c), rec(b"h", flag=1, refid=2, mref=len(REFS), mpos=3, tlen=1, codes=c),
            rec(b"i", flag=1, refid=-1, pos=-1, mref=-1, mpos=-1, codes=c),          # -1 == -1 is not "="
            rec(b"j", flag=1, refid=len(REFS), mref=len(REFS), mpos=3, codes=c)]


def cigar_records() -> list[bytes]:
    c = codes_of(9)
    out = [rec(b"none", cigar=[], codes=c), rec(b"one", cigar=[(9, 0)], codes=c), rec(b"all", cigar=[(k + 1, k) for k in range(9)], codes=c),
           rec(b"len", cigar=[(1, 0), (9, 1), (10, 2), (99, 3), (100, 4), ((1 << 28) - 1, 0), (0, 5)], codes=c)]
    rng = random.Random(5)
    out.append(rec(b"ops300", cigar=[(rng.choice((1, 9, 10, 99, 100, 12345, (1 << 28) - 1)), rng.randrange(9)) for _ in range(300)], codes=c))
    out.append(rec(b"ops64", cigar=[(k + 1, k % 9) for k in range(64)], codes=c))
    return out


SEQ_LENS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)


def seq_records(lens=SEQ_LENS + (10_000,)) -> list[bytes]:
    out = []
    for k, n in enumerate(lens):
        out.append(rec(b"s%d" % n, codes=codes_of(n, k), qual=bytes((0, 93, 0xFF, 41, 94, 222, 223, 127, 128)[i % 9] for i in range(n))))
    out.append(rec(b"even", codes=list(range(16)) * 2))             # every code in the high nibble first ...
    out.append(rec(b"odd", codes=[0] + list(range(16)) * 2))        # ... and in the low one
    for k in range(4):  # every output alignment of SEQ and QUAL: the name shifts them
        out.append(rec(b"n" * (k + 1), codes=codes_of(21, k)))
    return out


def name_records() -> list[bytes]:
    c = codes_of(8)
    return [rec(b"", codes=c), rec(b"x", codes=c), rec(bytes(33 + i % 90 for i in range(254)), codes=c)]


def tag_records() -> list[bytes]:
    c = codes_of(6)
    out = [rec(b"notags", codes=c)]
    for t, vals in INT_EXTREMES.items():
        out.append(rec(b"int_" + t.encode(), codes=c, tags=b"".join(tag("X%d" % k, t, v) for k, v in enumerate(vals))))
    out.append(rec(b"A", codes=c, tags=tag("XA", "A", 33) + tag("XB", "A", 126) + tag("XC", "A", 32)))
    out.append(rec(b"Z", codes=c, tags=tag("Z0", "Z", b"") + tag("Z1", "Z", b"a") + tag("Z2", "Z", b"abcd") + tag("H0", "H", b"1AE301") +
                   tag("Z3", "Z", bytes(33 + i % 90 for i in range(300))) + tag("H1", "H", b"")))
    out.append(rec(b"t40", codes=c, tags=b"".join(tag("T%d" % (k % 10), "iCZsA"[k % 5], (k * 1000, k, b"v%d" % k, -k, 65 + k % 26)[k % 5])
                                                     for k in range(40))))
    # a NUL behind a tag's value ends the list: what follows is not printed
    out.append(rec(b"stop", codes=c, tags=tag("NM", "i", 5) + b"\0" + tag("XX", "Z", b"hidden") + tag("XF", "f", 1.5)))
    out.append(rec(b"stopZ", codes=c, tags=tag("RG", "Z", b"g") + b"\0\0\0" + b"junk"))
    out.append(rec(b"stop1", codes=c, tags=tag("NM", "C", 5) + b"\0"))
    return out


def float_records() -> list[bytes]:
    c = codes_of(6)
    return [rec(b"f%d" % k, codes=c, tags=tag("NM", "i", k) + tag("XF", "f", v) + tag("RG", "Z", b"g")) for k, v in enumerate(FLOATS)]


def array_records() -> list[bytes]:
    c = codes_of(6)
    vals = {"c": (-128, 0, 127), "C": (0, 255), "s": (-32768, 32767), "S": (65535,), "i": (-(1 << 31), (1 << 31) - 1, 0), "I": ((1 << 32) - 1, 7),
            "f": (1.0, 0.1, -0.0, 1e10)}
    out = [rec(b"B" + s.encode(), codes=c, tags=tag("NM", "i", 1) + tag("XB", "B", (s, v)) + tag("RG", "Z", b"g")) for s, v in vals.items()]
    out.append(rec(b"Bempty", codes=c, tags=tag("XB", "B", ("s", ()))))
    return out


def unknown_records() -> list[bytes]:
    """The third record carries a tag type nothing defines."""
    return [basic(0), basic(1), rec(b"bad", codes=codes_of(5), tags=tag("NM", "i", 1) + b"XQq\x01\x02"), basic(3)]


def malformed_records() -> dict:
    c = codes_of(5)
    return {"short_int": [basic(0), rec(b"m", codes=c, tags=b"NMi\x01\x02")], "short_head": [rec(b"m", codes=c, tags=b"NM")],
            "open_string": [rec(b"m", codes=c, tags=b"RGZabc")], "bad_array": [rec(b"m", codes=c, tags=b"XBBq\x01\0\0\0\x05")],
            "short_array": [rec(b"m", codes=c, tags=b"XBBi\x02\0\0\0\x05\0\0\0")]}


def mix_records(n: int = 3000, seed: int = 11, arrays: bool = True) -> list[bytes]:
    """Drawn from every pool above; every 50th record takes the host path (arrays=False: only f tags, which the
    reference defines)."""
    pool = width_records() + ref_records() + cigar_records() + seq_records(SEQ_LENS) + name_records() + tag_records()
    pool += [basic(i) for i in range(40)]
    host = float_records() + (array_records() if arrays else [])
    rng = random.Random(seed)
    return [rng.choice(host) if i % 50 == 49 else rng.choice(pool) for i in range(n)]


def sam_cases() -> dict:
    """{name: records}; every case uses REFS."""
    out = {f"n{n}": [basic(i) for i in range(n)] for n in SIZES}
    out.update(widths=width_records(), refs=ref_records(), cigar=cigar_records(), seq=seq_records(), names=name_records(),
               tags=tag_records(), floats=float_records(), arrays=array_records(), mix=mix_records(),
               seq_short=seq_records(SEQ_LENS), mix_ref=mix_records(seed=12, arrays=False))
    return out


def fastq_records() -> list[bytes]:
    """Read lengths on both sides of begin + end + 1 for every trim window of TRIMS."""
    out = [rec(b"q%d" % n, codes=codes_of(n, n), flag=(0x10 if n % 2 else 0)) for n in (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 63, 64, 65, 70, 257)]
    return out + [rec(b"", codes=codes_of(12)), rec(b"n" * 254, codes=codes_of(40))]


def header_text(refs=REFS) -> str:
    return "@HD\tVN:1.4\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)


def pack(records):
    """(recs u8 with 16 bytes of slack, offs u64[n])"""
    recs, offs = bamutil.pack_records(records)
    return recs, offs[:-1]


def defined_by_reference(records: list[bytes]) -> bool:
    """The reference defines the text: no B array (the crafted ones are all tagged XB), every record within the
    block_size of 10,000 its reader takes (util/bam_deserializer.h:160), positions below INT32_MAX, CIGAR op codes
    0-8 (unknown tag types are not among the cases)."""
    import sam_model as M
    for r in records:
        p = M.parse(r)
        if len(r) - 4 > 10_000 or p["pos"] >= (1 << 31) - 1 or p["mpos"] >= (1 << 31) - 1 or any((op & 15) > 8 for op in p["cigar"]):
            return False
        if b"XBB" in p["tags"]:
            return False
    return True
