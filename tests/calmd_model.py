"""The definition of `openge calmd` restated in Python (include/openge_hip.h): the NM and MD
tags of BAM records recomputed against a reference, as `samtools calmd` does without its options.  There is no
reference implementation to hold the device code to, so this model is the yardstick: it is written from the
definition alone, record by record and base by base, and shares nothing with csrc/calmd.hip.

    calmd(records, refs, reference) -> Result     records: [bytes], refs: [(name, length)], reference: {name: bytes}
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

ERR_ARG, ERR_LIMIT = -1, -3
MAX_BLOCK_SIZE = 10000
ALPHABET = b"=ACMGRSVTWYHKDBN"
INT_TYPES = {ord("c"): "<b", ord("C"): "<B", ord("s"): "<h", ord("S"): "<H", ord("i"): "<i", ord("I"): "<I"}
FIXED = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
B_ELEM = {ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}


class CalmdError(Exception):
    """A call that fails: the error code and the lowest record it names."""

    def __init__(self, code: int, record: int, why: str):
        super().__init__(f"record {record} {why}")
        self.code, self.record, self.why = code, record, why


@dataclass
class Result:
    records: list = field(default_factory=list)
    skipped: int = 0
    no_reference: int = 0
    nm_changed: int = 0
    md_changed: int = 0

    def counters(self) -> dict:
        return {"records": len(self.records), "skipped": self.skipped, "no_reference": self.no_reference,
                "nm_changed": self.nm_changed, "md_changed": self.md_changed, "bytes_out": sum(map(len, self.records))}

    def offsets(self) -> list:
        out, acc = [0], 0
        for r in self.records:
            acc += len(r)
            out.append(acc)
        return out


def upper(seq: bytes) -> bytes:
    """The reference as it is loaded: a..z upper-cased, every other byte as it is."""
    return bytes(c - 32 if 97 <= c <= 122 else c for c in seq)


def load_fasta(path) -> dict:
    """name -> sequence bytes, upper-cased: the name up to the first blank, CR before LF dropped, the last of a
    repeated name wins."""
    out, name, parts = {}, None, []
    data = open(path, "rb").read()
    for line in data.split(b"\n"):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line.startswith(b">"):
            if name is not None:
                out[name] = upper(b"".join(parts))
            name, parts = line[1:].split(b" ")[0].split(b"\t")[0].decode(), []
        elif name is not None:
            parts.append(line)
    if name is not None:
        out[name] = upper(b"".join(parts))
    return out


def ref_code(b: int) -> int:
    k = ALPHABET.find(bytes([b]))
    return k if k >= 0 else 15


def walk(pos: int, ops: list, codes: list, ref: bytes) -> tuple[int, bytes]:
    """The walk of the definition: ops = [(code, length)], codes = the read's 4-bit codes -> (nm, MD)."""
    x, y, u, nm, md = pos, 0, 0, 0, bytearray()
    for code, ln in ops:
        if code in (0, 7, 8):  # M = X
            for _ in range(ln):
                if x >= len(ref):
                    return nm, bytes(md + str(u).encode())
                c1, c2 = codes[y], ref_code(ref[x])
                if c1 == 0 or (c1 == c2 and c1 != 15):
                    u += 1
                else:
                    md += str(u).encode() + bytes([ref[x]])
                    u, nm = 0, nm + 1
                x, y = x + 1, y + 1
        elif code == 2:  # D
            md += str(u).encode() + b"^" + ref[x:x + ln]
            u, nm, x = 0, nm + ln, x + ln
        elif code == 1:  # I
            y, nm = y + ln, nm + ln
        elif code == 4:  # S
            y += ln
        elif code == 3:  # N
            x += ln
    return nm, bytes(md + str(u).encode())


def parse_tags(rb: bytes, p: int) -> list | None:
    """[(name, type, start, end)] of the tags from p to the record's end; None when one does not fit."""
    out, end = [], len(rb)
    while p < end:
        if p + 3 > end:
            return None
        name, typ, start = rb[p:p + 2], rb[p + 2], p
        p += 3
        if typ in FIXED:
            p += FIXED[typ]
        elif typ in (ord("Z"), ord("H")):
            z = rb.find(b"\0", p)
            if z < 0:
                return None
            p = z + 1
        elif typ == ord("B"):
            if p + 5 > end or rb[p] not in B_ELEM:
                return None
            p += 5 + struct.unpack_from("<I", rb, p + 1)[0] * B_ELEM[rb[p]]
        else:
            return None
        if p > end:
            return None
        out.append((name, typ, start, p))
    return out


SKIPPED, NO_REFERENCE, USED = "skipped", "no_reference", "used"


def one(rb: bytes, refs: list, reference: dict):
    """One record -> (status, new record, nm changed, md changed); raises (code, why) as a tuple for a fault."""
    bs = struct.unpack_from("<I", rb, 0)[0]
    assert len(rb) == 4 + bs
    refid, pos, lname, _, _, nops, flag, lseq = struct.unpack_from("<iiBBHHHI", rb, 4)
    if flag & 4 or refid < 0 or pos < 0 or nops == 0 or lseq == 0:
        return SKIPPED, rb, False, False
    if refid >= len(refs):
        raise ValueError(ERR_ARG, "has a refID of n_ref or more")
    if refs[refid][0] not in reference:
        return NO_REFERENCE, rb, False, False
    ref = reference[refs[refid][0]]
    if bs > MAX_BLOCK_SIZE:
        raise ValueError(ERR_ARG, "has a block_size above 10000")
    cig_at = 36 + lname
    seq_at = cig_at + 4 * nops
    if seq_at > len(rb):
        raise ValueError(ERR_ARG, "has a CIGAR that does not fit its block_size")
    ops = [(w & 15, w >> 4) for w in struct.unpack_from(f"<{nops}I", rb, cig_at)]
    if any(c > 8 for c, _ in ops):
        raise ValueError(ERR_ARG, "has a CIGAR op code above 8")
    tag_at = seq_at + (lseq + 1) // 2 + lseq
    tags = parse_tags(rb, tag_at) if tag_at <= len(rb) else None
    if tags is None:
        raise ValueError(ERR_ARG, "has bases, qualities or tags that do not fit its block_size")
    if sum(ln for c, ln in ops if c in (0, 1, 4, 7, 8)) != lseq:
        raise ValueError(ERR_ARG, "has CIGAR ops whose read bases do not sum to l_seq")
    codes = [(rb[seq_at + i // 2] >> 4) if i % 2 == 0 else (rb[seq_at + i // 2] & 15) for i in range(lseq)]
    nm, md = walk(pos, ops, codes, ref)
    first = {}
    for t in tags:
        first.setdefault(t[0], t)
    nm_tag, md_tag = first.get(b"NM"), first.get(b"MD")
    nm_keep = nm_tag is not None and nm_tag[1] in INT_TYPES and struct.unpack_from(INT_TYPES[nm_tag[1]], rb, nm_tag[2] + 3)[0] == nm
    md_keep = md_tag is not None and md_tag[1] == ord("Z") and rb[md_tag[2] + 3:md_tag[3] - 1] == md
    cut = sorted(t[2:] for t, keep in ((nm_tag, nm_keep), (md_tag, md_keep)) if t is not None and not keep)
    body, at = bytearray(), 4
    for a, b in cut:
        body += rb[at:a]
        at = b
    body += rb[at:]
    if not nm_keep:
        body += b"NM" + (b"C" + struct.pack("<B", nm) if nm < 256 else b"S" + struct.pack("<H", nm) if nm < 65536 else
                         b"I" + struct.pack("<I", nm & 0xFFFFFFFF))
    if not md_keep:
        body += b"MDZ" + md + b"\0"
    if nm > 0xFFFFFFFF or len(body) > MAX_BLOCK_SIZE:
        raise ValueError(ERR_LIMIT, "would exceed the largest block_size (10000) with its new tags")
    return USED, struct.pack("<I", len(body)) + bytes(body), not nm_keep, not md_keep


def calmd(records: list, refs: list, reference: dict) -> Result:
    """Every record in order; the lowest faulty record fails the call (CalmdError), and then nothing is written."""
    res = Result()
    for i, rb in enumerate(records):
        try:
            status, new, nm_c, md_c = one(rb, refs, reference)
        except ValueError as e:
            raise CalmdError(e.args[0], i, e.args[1]) from None
        res.records.append(new)
        res.skipped += status == SKIPPED
        res.no_reference += status == NO_REFERENCE
        res.nm_changed += nm_c
        res.md_changed += md_c
    return res


def tags_of(rb: bytes) -> dict:
    """name -> (type char, value) of a record's tags (the first of each name); Z values as bytes, integers as int."""
    refid, pos, lname, _, _, nops, flag, lseq = struct.unpack_from("<iiBBHHHI", rb, 4)
    out = {}
    for name, typ, a, b in parse_tags(rb, 36 + lname + 4 * nops + (lseq + 1) // 2 + lseq) or []:
        if name.decode() in out:
            continue
        v = rb[a + 3:b - 1] if typ in (ord("Z"), ord("H")) else struct.unpack_from(INT_TYPES[typ], rb, a + 3)[0] if typ in INT_TYPES else rb[a + 3:b]
        out[name.decode()] = (chr(typ), v)
    return out


def nm_md_of_record(rb: bytes, ref: bytes) -> tuple[int, bytes]:
    """(nm, MD) of the walk of one well-formed record against its contig's sequence."""
    refid, pos, lname, _, _, nops, flag, lseq = struct.unpack_from("<iiBBHHHI", rb, 4)
    cig_at = 36 + lname
    seq_at = cig_at + 4 * nops
    ops = [(w & 15, w >> 4) for w in struct.unpack_from(f"<{nops}I", rb, cig_at)]
    codes = [(rb[seq_at + i // 2] >> 4) if i % 2 == 0 else (rb[seq_at + i // 2] & 15) for i in range(lseq)]
    return walk(pos, ops, codes, ref)
