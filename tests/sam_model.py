"""Plain-Python restatement of the two text modes of `openge view` / -F sam|fastq (csrc/sam.hip, csrc/sam_host.cpp):
the reference's SamWriter::write (util/sam_writer.cpp:90-217) and the single-stream form of FastqWriter::write
(util/fastq_writer.cpp:99-100) with Filter::trim (algorithms/filter.cpp:183-190).

Kept from the reference: the mate rule (paired and 0 <= mate refID < n_ref, else `*\t0\t0`), QUAL + 33 wrapping at
8 bits, f as printf %g, and the tag list stopping at a NUL byte behind a tag's value (sam_writer.cpp:210).
Beyond what the reference defines (pinned here only): a B array is rendered as the SAM specification says
(XX:B:c,1,-2, float elements %g), CIGAR op codes 9-15 print '?', POS + 1 is computed without wrapping, and a tag
of any other type, a tag cut short or a Z string without its NUL raises BadRecord."""
from __future__ import annotations

import math
import struct

BASES = "=ACMGRSVTWYHKDBN"
CIGAR = "MIDNSHP=X"
INT_TAGS = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
B_ELEM = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


class BadRecord(ValueError):
    pass


def fmt_g(raw: bytes) -> str:
    """printf("%g") of the float32 in `raw`."""
    (v,) = struct.unpack("<f", raw)
    if math.isnan(v):
        return "-nan" if raw[3] & 0x80 else "nan"
    return "%g" % v


def parse(rec: bytes) -> dict:
    (bs,) = struct.unpack_from("<I", rec, 0)
    refid, pos, lname, mapq, _bin, ncig, flag, lseq, mref, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    var = lname + 4 * ncig + (max(lseq, 0) + 1) // 2 + max(lseq, 0)
    if bs < 32 or lseq < 0 or lname < 1 or 32 + var > bs or bs + 4 != len(rec):
        raise BadRecord("lengths")
    p = 36
    name = rec[p:p + lname - 1]
    p += lname
    cigar = struct.unpack_from(f"<{ncig}I", rec, p)
    p += 4 * ncig
    seq = rec[p:p + (lseq + 1) // 2]
    p += (lseq + 1) // 2
    qual = rec[p:p + lseq]
    p += lseq
    return dict(refid=refid, pos=pos, mapq=mapq, flag=flag, lseq=lseq, mref=mref, mpos=mpos, tlen=tlen, name=name, cigar=cigar,
                seq=seq, qual=qual, tags=rec[p:])


def bases(seq: bytes, a: int, z: int) -> bytes:
    return "".join(BASES[(seq[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(a, z)).encode()


def quals(qual: bytes, a: int, z: int) -> bytes:
    return bytes((q + 33) & 0xFF for q in qual[a:z])


def tag_text(t: bytes) -> tuple[bytes, bool]:
    """(the tags' text with the leading tabs, whether an f or B tag was met before the list ended)"""
    out, host, i = bytearray(), False, 0
    while i < len(t):
        if len(t) - i < 3:
            raise BadRecord("tag cut short")
        name, typ = t[i:i + 2], chr(t[i + 2])
        i += 3
        out += b"\t" + name + b":"
        if typ == "A":
            if len(t) - i < 1:
                raise BadRecord("tag cut short")
            out += b"A:" + t[i:i + 1]
            i += 1
        elif typ in INT_TAGS:
            sz = struct.calcsize(INT_TAGS[typ])
            if len(t) - i < sz:
                raise BadRecord("tag cut short")
            out += b"i:%d" % struct.unpack_from(INT_TAGS[typ], t, i)
            i += sz
        elif typ == "f":
            if len(t) - i < 4:
                raise BadRecord("tag cut short")
            out += b"f:" + fmt_g(t[i:i + 4]).encode()
            host = True
            i += 4
        elif typ in "ZH":
            e = t.find(b"\0", i)
            if e < 0:
                raise BadRecord("string without NUL")
            out += typ.encode() + b":" + t[i:e]
            i = e + 1
        elif typ == "B":
            if len(t) - i < 5 or chr(t[i]) not in B_ELEM:
                raise BadRecord("array")
            sub = chr(t[i])
            (cnt,) = struct.unpack_from("<I", t, i + 1)
            sz = struct.calcsize(B_ELEM[sub])
            if cnt * sz > len(t) - i - 5:
                raise BadRecord("array cut short")
            out += b"B:" + sub.encode()
            i += 5
            for _ in range(cnt):
                out += b"," + (fmt_g(t[i:i + 4]).encode() if sub == "f" else b"%d" % struct.unpack_from(B_ELEM[sub], t, i))
                i += sz
            host = True
        else:
            raise BadRecord(f"unknown tag type {typ!r}")
        if i < len(t) and t[i] == 0:
            break
    return bytes(out), host


def needs_host(rec: bytes) -> bool:
    """The record takes the host path: an f or B tag in the part of the tag list that is printed."""
    return tag_text(parse(rec)["tags"])[1]


def sam_line(rec: bytes, names: list[str]) -> bytes:
    r = parse(rec)
    n_ref = len(names)
    out = bytearray(r["name"])
    out += b"\t%d\t" % r["flag"]
    out += names[r["refid"]].encode() if 0 <= r["refid"] < n_ref else b"*"
    out += b"\t%d\t%d\t" % (r["pos"] + 1, r["mapq"])
    out += b"".join(b"%d%c" % (op >> 4, ord(CIGAR[op & 15]) if (op & 15) < 9 else ord("?")) for op in r["cigar"]) or b"*"
    out += b"\t"
    if (r["flag"] & 1) and 0 <= r["mref"] < n_ref:
        out += b"=" if r["mref"] == r["refid"] else names[r["mref"]].encode()
        out += b"\t%d\t%d\t" % (r["mpos"] + 1, r["tlen"])
    else:
        out += b"*\t0\t0\t"
    if r["lseq"] == 0:
        out += b"*\t*"
    else:
        out += bases(r["seq"], 0, r["lseq"]) + b"\t" + quals(r["qual"], 0, r["lseq"])
    return bytes(out) + tag_text(r["tags"])[0] + b"\n"


def fastq_entry(rec: bytes, trim_begin: int = 0, trim_end: int = 0) -> bytes:
    """SEQ and QUAL are both [trim_begin, l_seq - trim_end).  The reference's SEQ is that; its QUAL under a trim
    window is not reproduced: Filter::trim (filter.cpp:188-189) cuts the qualities of the already shortened read a
    second time, leaving fewer qualities than bases or bytes from behind them, and throws on short reads."""
    r = parse(rec)
    a, z = (trim_begin, r["lseq"] - trim_end) if r["lseq"] > trim_begin + trim_end else (0, 0)
    return b"@" + r["name"] + b"\n" + bases(r["seq"], a, z) + b"\n+" + r["name"] + b"\n" + quals(r["qual"], a, z) + b"\n"


def lines(records: list[bytes], names: list[str], mode: str = "sam", trim=(0, 0)) -> list[bytes]:
    if mode == "sam":
        return [sam_line(r, names) for r in records]
    return [fastq_entry(r, *trim) for r in records]


def split_records(recs, offs) -> list[bytes]:
    """The records of an arena (recs u8, offs u64[n]) as byte strings."""
    out = []
    for o in offs:
        o = int(o)
        (bs,) = struct.unpack_from("<I", recs, o)
        out.append(bytes(recs[o:o + 4 + bs]))
    return out


def split_header(data: bytes) -> tuple[bytes, bytes]:
    """(the leading @ lines, the rest) of SAM text."""
    p = 0
    while data[p:p + 1] == b"@":
        p = data.index(b"\n", p) + 1
    return data[:p], data[p:]


def parse_region(region: str, refs: list[tuple[str, int]]) -> tuple[int, int, int]:
    """Filter::ParseRegionString (algorithms/filter.cpp:34-136) for "chr", "chr:pos" and "chr:start..stop":
    (refID, left, right) as the predicate compares them."""
    chrom, _, rest = region.partition(":")
    rid = [n for n, _ in refs].index(chrom)
    if not rest:
        return rid, 0, refs[rid][1]
    a, dots, z = rest.partition("..")
    return rid, int(a), int(z) if dots else int(a)


def filter_args(args: list[str], refs) -> dict:
    """The -n / -q / -l / -r arguments of `openge view` as filter_keep's keywords."""
    kw, it = {}, iter(args)
    for k in it:
        v = next(it)
        if k == "-n":
            kw["count"] = int(v)
        elif k == "-q":
            kw["mapq"] = int(v)
        elif k == "-r":
            kw["region"] = parse_region(v, refs)
        elif k == "-l":  # Filter::setReadLengths (filter.cpp:143-171)
            if v[0] == "+":
                kw["min_len"] = int(v[1:])
            elif v[0] == "-":
                kw["min_len"], kw["max_len"] = -(1 << 31), int(v[1:])
            elif "-" in v:
                kw["min_len"], kw["max_len"] = map(int, v.split("-"))
            else:
                kw["min_len"] = kw["max_len"] = int(v)
    return kw


# Filter::runInternal's predicate (algorithms/filter.cpp:192-249) on parsed records, for the CLI comparisons
def filter_keep(records: list[bytes], mapq=0, min_len=0, max_len=(1 << 31) - 1, trim_total=0, region=None, count=None) -> list[bytes]:
    out = []
    for rec in records:
        if count is not None and len(out) >= count:
            break
        r = parse(rec)
        ok = r["mapq"] >= mapq and min_len <= r["lseq"] <= max_len and r["lseq"] > trim_total
        if ok and region is not None:
            rid, left, right = region
            ok = r["refid"] == rid and r["pos"] + r["lseq"] >= left and r["pos"] <= right
        if ok:
            out.append(rec)
    return out
