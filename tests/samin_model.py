"""Plain-Python model of SAM input (csrc/sam_parse.hip, csrc/sam_host.cpp): one SAM line -> the bytes of its BAM
record, and the line index of a SAM text.  Written from the rules, not from the C++:

where the reference (util/sam_reader.cpp:313-488) is defined its record is reproduced byte for byte: POS - 1 and
PNEXT - 1, TLEN as it is, fields translated independently, bin by CalculateMinimumBin (bam_serializer.h:92-116) over
[POS - 1, POS - 1 + the M/D/N/=/X lengths), `*` RNAME / RNEXT -> -1, `=` -> the read's refID, an unknown RNEXT -> -1
with a warning, an unknown RNAME -> UnknownContig, integer tags in the reference's smallest type.
Where the reference aborts or corrupts, the SAM specification: QUAL `*` -> 0xFF, SEQ `*` -> l_seq 0, lowercase
bases as uppercase (any other character N), B arrays, H strings, i values up to 2^32 - 1 as I.
Everything else raises BadLine(field)."""
from __future__ import annotations

import re
import struct

BASES = "=ACMGRSVTWYHKDBN"
CIGAR = "MIDNSHP=X"
NUM = re.compile(rb"-?[0-9]+\Z")
I32 = (-(1 << 31), (1 << 31) - 1)
B_FMT = {"c": ("<b", -128, 127), "C": ("<B", 0, 255), "s": ("<h", -32768, 32767), "S": ("<H", 0, 65535), "i": ("<i",) + I32,
         "I": ("<I", 0, (1 << 32) - 1)}


class BadLine(ValueError):
    def __init__(self, field: str):
        super().__init__(field)
        self.field = field


class UnknownContig(BadLine):
    pass


def number(b: bytes, lo: int, hi: int, field: str) -> int:
    if not NUM.match(b) or not lo <= int(b) <= hi:
        raise BadLine(field)
    return int(b)


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return (base + (beg >> shift)) & 0xFFFF
    return 0


def wrap32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def int_tag(v: int) -> bytes:
    if 0 <= v <= 255:
        return b"C" + struct.pack("<B", v)
    if -128 <= v < 0:
        return b"c" + struct.pack("<b", v)
    if 0 <= v <= 65535:
        return b"S" + struct.pack("<H", v)
    if -32768 <= v < 0:
        return b"s" + struct.pack("<h", v)
    return b"I" + struct.pack("<I", v) if v >= 0 else b"i" + struct.pack("<i", v)


def tag_bytes(t: bytes) -> tuple[bytes, bool]:
    """(the tag's bytes in the record, whether it takes the host path)"""
    if len(t) < 5 or t[2:3] != b":" or t[4:5] != b":":
        raise BadLine("tag")
    name, typ, val = t[:2], chr(t[3]), t[5:]
    if typ == "A":
        if len(val) != 1:
            raise BadLine("tag")
        return name + b"A" + val, False
    if typ == "i":
        return name + int_tag(number(val, -(1 << 31), (1 << 32) - 1, "tag integer")), False
    if typ == "f":
        try:
            return name + b"f" + struct.pack("<f", float(val)), True
        except (ValueError, OverflowError):
            raise BadLine("tag float")
    if typ in "ZH":
        return name + typ.encode() + val + b"\0", False
    if typ == "B":
        sub = chr(val[0]) if val else ""
        if sub not in B_FMT and sub != "f" or (len(val) > 1 and val[1:2] != b","):
            raise BadLine("tag")
        el = val[2:].split(b",") if len(val) > 1 else []
        out = name + b"B" + sub.encode() + struct.pack("<I", len(el))
        for e in el:
            if sub == "f":
                try:
                    out += struct.pack("<f", float(e))
                except (ValueError, OverflowError):
                    raise BadLine("tag array element")
            else:
                fmt, lo, hi = B_FMT[sub]
                out += struct.pack(fmt, number(e, lo, hi, "tag array element"))
        return out, True
    raise BadLine("tag type")


def base_code(c: int) -> int:
    k = BASES.find(chr(c).upper()) if c < 128 else -1
    return k if k >= 0 else 15


def parse_line(line: bytes, names: list[str]) -> tuple[bytes, bool, bool]:
    """(the record, RNEXT unknown, the line takes the host path)"""
    if len(line) < 10:
        raise BadLine("short")
    f = line.split(b"\t")
    if len(f) < 11:
        raise BadLine("fields")
    ids = {}
    for i, nm in enumerate(names):
        ids.setdefault(nm.encode(), i)
    if len(f[0]) > 254:
        raise BadLine("QNAME")
    flag = number(f[1], 0, 65535, "FLAG")
    refid = -1
    if f[2] != b"*":
        if f[2] not in ids:
            raise UnknownContig("RNAME")
        refid = ids[f[2]]
    pos = number(f[3], I32[0] + 1, I32[1] + 1, "POS") - 1
    mapq = number(f[4], 0, 255, "MAPQ")
    cigar = []
    if f[5] != b"*":
        if not re.match(rb"([0-9]+[MIDNSHP=X])+\Z", f[5]):
            raise BadLine("CIGAR")
        for ln, op in re.findall(rb"([0-9]+)([MIDNSHP=X])", f[5]):
            if int(ln) >= 1 << 28:
                raise BadLine("CIGAR")
            cigar.append((int(ln) << 4) | CIGAR.index(op.decode()))
        if len(cigar) > 65535:
            raise BadLine("CIGAR ops")
    warn = False
    if f[6] == b"=":
        mref = refid
    elif f[6] == b"*":
        mref = -1
    else:
        mref = ids.get(f[6], -1)
        warn = f[6] not in ids
    mpos = number(f[7], I32[0] + 1, I32[1] + 1, "PNEXT") - 1
    tlen = number(f[8], I32[0], I32[1], "TLEN")
    seq = b"" if f[9] == b"*" else f[9]
    if f[10] == b"*":
        qual = b"\xff" * len(seq)
    elif len(f[10]) != len(seq):
        raise BadLine("QUAL")
    else:
        qual = bytes((q - 33) & 0xFF for q in f[10])
    packed = bytearray((len(seq) + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= base_code(c) << (0 if i & 1 else 4)
    span = sum(op >> 4 for op in cigar if CIGAR[op & 15] in "MDN=X")
    tags, host = b"", False
    for t in f[11:]:
        tb, h = tag_bytes(t)
        tags += tb
        host |= h
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(f[0]) + 1, mapq, reg2bin(pos, wrap32(pos + span)), len(cigar), flag, len(seq), mref, mpos,
                       tlen)
    body += f[0] + b"\0" + b"".join(struct.pack("<I", op) for op in cigar) + bytes(packed) + qual + tags
    return struct.pack("<I", len(body)) + body, warn, host


def split_text(text: bytes) -> tuple[bytes, list[bytes]]:
    """(the header: the leading lines that begin with '@', the body's lines).  A last line without its newline is
    a line; a trailing newline adds none."""
    p = 0
    while text[p:p + 1] == b"@":
        e = text.find(b"\n", p)
        p = len(text) if e < 0 else e + 1
    body = text[p:]
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return text[:p], lines


def contigs(header: bytes) -> list[str]:
    out = []
    for ln in header.split(b"\n"):
        if ln.startswith(b"@SQ\t"):
            out.append(next((x[3:] for x in ln.split(b"\t")[1:] if x.startswith(b"SN:")), b"").decode())
    return out


def line_offsets(text: bytes) -> list[int]:
    """oge_sam_lines_dev's table: off[0] = the body's start, off[i + 1] = one past line i's newline."""
    header, lines = split_text(text)
    off = [len(header)]
    for ln in lines:
        off.append(off[-1] + len(ln) + 1)
    return off


def parse_text(text: bytes, names: list[str] | None = None):
    """(records, warning flags, host flags) of a whole SAM text; BadLine carries .line (1-based in the file)."""
    header, lines = split_text(text)
    if names is None:
        names = contigs(header)
    recs, warns, hosts = [], [], []
    for i, ln in enumerate(lines):
        try:
            r, w, h = parse_line(ln, names)
        except BadLine as e:
            e.line = header.count(b"\n") + i + 1
            raise
        recs.append(r)
        warns.append(w)
        hosts.append(h)
    return recs, warns, hosts
