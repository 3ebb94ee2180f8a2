"""Crafted coordinate-sorted BAM files for the index tests (CPU model tests and GPU tests share them)."""
from __future__ import annotations

import struct

import bamutil

REF_LEN = 1 << 29


def header_bytes(refs: list[tuple[str, int]]) -> bytes:
    text = "@HD\tVN:1.4\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    ht = text.encode()
    body = b"BAM\1" + struct.pack("<i", len(ht)) + ht + struct.pack("<i", len(refs))
    for name, ln in refs:
        nb = name.encode() + b"\0"
        body += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    return body


def make_bam(refs, records: list[bytes], payload: int = 65280, level: int = 6) -> bytes:
    """Header and records in one stream cut into `payload`-byte BGZF blocks (plus the EOF block)."""
    return bamutil.bgzf_blocks(header_bytes(refs) + b"".join(records), level, payload)


def rec(name, refid, pos, cigar="10M", flag=0, size: int | None = None) -> bytes:
    """A record; size: its exact byte length, reached with a Z tag of filler."""
    seq = "A" * 10
    r = bamutil.make_record(name, flag, refid, pos, cigar, seq)
    if size is not None:
        pad = size - len(r) - 4
        assert pad >= 0, (size, len(r))
        r = bamutil.make_record(name, flag, refid, pos, cigar, seq, tags=b"XXZ" + b"x" * pad + b"\0")
        assert len(r) == size
    return r


def refs(n: int) -> list[tuple[str, int]]:
    return [(f"chr{i}", REF_LEN) for i in range(n)]


def bin_edges() -> tuple[list, list[bytes]]:
    """A record straddling each of the 16 Ki / 128 Ki / 1 Mi / 8 Mi / 64 Mi edges (via N and via D), pos 0,
    rend == 2^29, a 10I5S record (no reference length), a 0x4 record placed on the reference."""
    rows = [(0, "10M", 0), (5000, "10I5S", 0), (7000, "10M", 0x4)]
    for shift in (14, 17, 20, 23, 26):  # 1 << shift and 3 << shift are edges of that level and of no higher one
        rows.append(((1 << shift) - 10, "5M20N5M", 0))
        rows.append(((3 << shift) - 3, "2M7D9M", 0))
    rows.append((REF_LEN - 10, "10M", 0))
    rows.sort(key=lambda r: r[0])
    return refs(1), [rec(f"e{i}", 0, p, c, f) for i, (p, c, f) in enumerate(rows)]


def refs_and_gaps() -> tuple[list, list[bytes]]:
    """References without reads first, in the middle and last; a 300 kb gap before the first read and one in
    the middle (empty linear windows leading and inside); one record over 40 windows; unplaced reads last."""
    out = []
    for r in (1, 3):
        out += [rec(f"a{r}", r, 300_000), rec(f"b{r}", r, 300_100), rec(f"c{r}", r, 620_000, "10M638960N10M"),
                rec(f"d{r}", r, 620_500), rec(f"g{r}", r, 1_600_000, flag=0x4)]
    out += [rec("u0", -1, -1, "", 0x4), rec("u1", -1, -1, "", 0x4)]
    return refs(5), out


def empty3() -> tuple[list, list[bytes]]:
    return refs(3), []


def one_record() -> tuple[list, list[bytes]]:
    return refs(1), [rec("only", 0, 12345)]


def unmapped_only() -> tuple[list, list[bytes]]:
    return refs(2), [rec(f"u{i}", -1, -1, "", 0x4) for i in range(5)]


CRAFTED = {"bin_edges": bin_edges, "refs_and_gaps": refs_and_gaps, "empty3": empty3, "one_record": one_record,
           "unmapped_only": unmapped_only}


def over_limit() -> tuple[list, list[bytes]]:
    """rend == 2^29 + 1"""
    return refs(1), [rec("ok", 0, 100), rec("far", 0, REF_LEN - 9, "10M")]


def block_layout(payload: int, big: int | None = None) -> tuple[list, list[bytes], dict]:
    """For `payload`-byte blocks: a record ending exactly on a payload boundary, a record spanning three
    blocks (`big` bytes, default 2 * payload + 200), bin 4681 revisited within one block (the chunks merge)
    and bin 4682 revisited in a later block (they do not).  -> (refs, records, {name: record index})."""
    rf = refs(1)
    h = len(header_bytes(rf))
    big = big or 2 * payload + 200
    small = 120
    out, idx = [], {}
    # bin 4681 (window 0), bin 585 between, bin 4681 again: all three inside the first block
    out += [rec("m0", 0, 100, size=small), rec("m1", 0, 200, "10M20000N10M", size=small), rec("m2", 0, 300, size=small)]
    assert h + 3 * small < payload
    # fill so that record `edge` ends exactly where a block ends
    used = h + 3 * small
    fill = payload - used % payload
    if fill < 60:
        fill += payload
    out.append(rec("edge", 0, 400, size=fill))
    idx["edge"] = len(out) - 1
    assert (used + fill) % payload == 0
    # window 1 (bin 4682), then a record over three blocks in bin 585, then window 1 again in a later block
    out.append(rec("n0", 0, 16384 + 10, size=small))
    out.append(rec("big", 0, 16384 + 20, "10M20000N10M", size=big))
    idx["big"] = len(out) - 1
    out.append(rec("n2", 0, 16384 + 30, size=small))
    out.append(rec("tail", 0, 50_000, size=small))
    return rf, out, idx
