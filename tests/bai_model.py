"""The project's canonical BAM index (.bai), restated in plain Python.

Independent of the product: it works from a decompressed record stream plus a block table, or from the
bytes of a BGZF BAM file (zlib only).  Also a small BAI parser and an index-driven region query, so a test
can show that an image is not merely byte-equal to this model but finds the records.

Definitions (SAM v1 section 5.2 for the layout):
  voff(x)      = cstart[b] << 16 | (x - uoff[b]), b the last block with uoff[b] <= x (a position on a block
                 edge belongs to the block that starts there; x == uoff[nblk] gives cstart[nblk] << 16)
  span         rbeg = pos, rend = pos + max(1, reference length); FLAG 0x4 or no CIGAR ops: length 1
  chunk        a maximal run of consecutive records with one (refID, bin): [beg of first, end of last],
               end = voff of the next record's first byte; chunk k+1 of a bin merges into chunk k when
               (end_k >> 16) >= (beg_{k+1} >> 16), judged on the unmerged neighbours
  linear       ioffset[w] = smallest beg of a record overlapping 16 Ki window w; an empty window takes the
               next window's value; n_intv = last window + 1
  per ref      bins ascending, pseudo-bin 37450 last (first beg, last end; records without / with 0x4)
"""
from __future__ import annotations

import bisect
import struct
import zlib

PSEUDO_BIN = 37450
MAX_END = 1 << 29


class Unsorted(ValueError):
    """The record at .index breaks the coordinate order (OGE_ERR_ARG in the product)."""

    def __init__(self, index: int):
        super().__init__(f"record {index} is out of order")
        self.index = index


class Limit(ValueError):
    """The record at .index ends past 2^29 (OGE_ERR_LIMIT in the product)."""

    def __init__(self, index: int):
        super().__init__(f"record {index} ends past 2^29")
        self.index = index


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    if beg >> 14 == end >> 14:
        return 4681 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return 585 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return 73 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return 9 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return 1 + (beg >> 26)
    return 0


def reg2bins(beg: int, end: int) -> list[int]:
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(base + (beg >> shift), base + (end >> shift) + 1))
    return out


def span(rb) -> tuple[int, int, int, int]:
    """-> (refID, rbeg, rend, flag) of one record (block_size included in rb)."""
    refid, pos, lname, _mapq, _bin, ncig, flag = struct.unpack_from("<iiBBHHH", rb, 4)
    length = 0
    if not flag & 0x4 and ncig:
        for op in struct.unpack_from(f"<{ncig}I", rb, 36 + lname):
            if op & 0xF in (0, 2, 3, 7, 8):  # M D N = X
                length += op >> 4
    return refid, pos, pos + max(1, length), flag


# ------------------------------------------------------------------------------------------ BGZF
def bgzf_walk(bam: bytes) -> list[tuple[int, int, int, int]]:
    """Every block of the file: (file offset, deflate start, deflate end, ISIZE)."""
    out, p = [], 0
    while p < len(bam):
        assert bam[p:p + 4] == b"\x1f\x8b\x08\x04", "not BGZF"
        (xlen,) = struct.unpack_from("<H", bam, p + 10)
        x, xend, bsize = p + 12, p + 12 + xlen, 0
        while x + 4 <= xend:
            (slen,) = struct.unpack_from("<H", bam, x + 2)
            if bam[x:x + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", bam, x + 4)[0] + 1
            x += 4 + slen
        assert bsize, "no BC field"
        (isize,) = struct.unpack_from("<I", bam, p + bsize - 4)
        out.append((p, xend, p + bsize - 8, isize))
        p += bsize
    return out


def block_table(bam: bytes) -> tuple[list[int], list[int]]:
    """(uoff, cstart), nblk + 1 entries each: the blocks with a non-empty payload, then the payload total
    and the file offset just past the last of them."""
    uoff, cstart, tot, end = [], [], 0, 0
    for p, _d0, d1, isize in bgzf_walk(bam):
        if isize:
            uoff.append(tot)
            cstart.append(p)
            tot += isize
            end = d1 + 8
    return uoff + [tot], cstart + [end]


def inflate_all(bam: bytes) -> bytes:
    return b"".join(zlib.decompress(bam[d0:d1], -15) for _p, d0, d1, isize in bgzf_walk(bam) if isize)


def stream_layout(raw: bytes) -> tuple[int, int, list[int]]:
    """Decompressed BAM stream -> (n_ref, offset of the first record, record offsets)."""
    assert raw[:4] == b"BAM\1"
    (lt,) = struct.unpack_from("<i", raw, 4)
    p = 8 + lt
    (n_ref,) = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, p)
        p += 8 + ln
    base, offs = p, []
    while p < len(raw):
        offs.append(p)
        p += 4 + struct.unpack_from("<I", raw, p)[0]
    assert p == len(raw)
    return n_ref, base, offs


# ------------------------------------------------------------------------------------------ build
def build(recs, offs, n_ref: int, stream_base: int, uoff, cstart) -> bytes:
    """The index image of the records recs[offs[i]:] (n = len(offs); contiguous; record 0 at stream position
    stream_base) under the block table (uoff, cstart)."""
    if n_ref < 0:
        raise Limit(-1)
    recs = bytes(recs) if not isinstance(recs, (bytes, memoryview)) else recs
    uoff = [int(x) for x in uoff]
    cstart = [int(x) for x in cstart]
    offs = [int(o) for o in offs]
    n = len(offs)

    def voff(x: int) -> int:
        b = bisect.bisect_right(uoff, x) - 1
        assert b >= 0 and x <= uoff[-1], "record outside the block table"
        assert x - uoff[b] < 1 << 16
        return cstart[b] << 16 | (x - uoff[b])

    spans, begs = [], []
    prev = None
    for i, o in enumerate(offs):
        (bs,) = struct.unpack_from("<I", recs, o)
        refid, rbeg, rend, flag = span(recs[o:o + 4 + bs])
        assert -1 <= refid < n_ref and (refid < 0 or rbeg >= 0), f"record {i} is malformed"
        key = (refid & 0xFFFFFFFF, rbeg if refid >= 0 else 0)
        if prev is not None and key < prev:
            raise Unsorted(i)
        prev = key
        if refid >= 0 and rend > MAX_END:
            raise Limit(i)
        spans.append((refid, rbeg, rend, flag))
        begs.append(voff(stream_base + o - offs[0]))
    if n:
        (bs,) = struct.unpack_from("<I", recs, offs[-1])
        begs.append(voff(stream_base + offs[-1] - offs[0] + 4 + bs))

    bins = [dict() for _ in range(n_ref)]      # bin -> list of [beg, end] runs in file order
    lin = [dict() for _ in range(n_ref)]       # window -> smallest beg
    meta = [None] * n_ref                      # [first beg, last end, n without 0x4, n with 0x4]
    n_no_coor = 0
    last = None
    for i, (refid, rbeg, rend, flag) in enumerate(spans):
        if refid < 0:
            n_no_coor += 1
            last = None
            continue
        b = reg2bin(rbeg, rend)
        if last == (refid, b):
            bins[refid][b][-1][1] = begs[i + 1]
        else:
            bins[refid].setdefault(b, []).append([begs[i], begs[i + 1]])
        last = (refid, b)
        for w in range(rbeg >> 14, ((rend - 1) >> 14) + 1):
            lin[refid][w] = min(lin[refid].get(w, begs[i]), begs[i])
        if meta[refid] is None:
            meta[refid] = [begs[i], begs[i + 1], 0, 0]
        meta[refid][1] = begs[i + 1]
        meta[refid][3 if flag & 0x4 else 2] += 1

    out = [b"BAI\1", struct.pack("<i", n_ref)]
    for r in range(n_ref):
        out.append(struct.pack("<i", len(bins[r]) + (1 if meta[r] else 0)))
        for b in sorted(bins[r]):
            runs = bins[r][b]
            chunks = [list(runs[0])]
            for k in range(1, len(runs)):
                if runs[k - 1][1] >> 16 >= runs[k][0] >> 16:
                    chunks[-1][1] = runs[k][1]
                else:
                    chunks.append(list(runs[k]))
            out.append(struct.pack("<Ii", b, len(chunks)))
            out.extend(struct.pack("<QQ", *c) for c in chunks)
        if meta[r]:
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, *meta[r]))
        n_intv = max(lin[r]) + 1 if lin[r] else 0
        io = [0] * n_intv
        nxt = 0
        for w in range(n_intv - 1, -1, -1):
            nxt = lin[r].get(w, nxt)
            io[w] = nxt
        out.append(struct.pack(f"<i{n_intv}Q", n_intv, *io))
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def build_from_bam(bam: bytes) -> bytes:
    raw = inflate_all(bam)
    n_ref, base, offs = stream_layout(raw)
    uoff, cstart = block_table(bam)
    return build(raw, offs, n_ref, base, uoff, cstart)


# ------------------------------------------------------------------------------------------ parse
def parse(bai: bytes) -> dict:
    """-> {"refs": [{"bins": {bin: [(beg, end)...]} (in file order of the image), "order": [bin...],
    "pseudo": (beg, end, mapped, unmapped) | None, "ioffset": [...]}], "n_no_coor": int}"""
    assert bai[:4] == b"BAI\1", "not a BAI"
    (n_ref,) = struct.unpack_from("<i", bai, 4)
    p, refs = 8, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", bai, p)
        p += 4
        bins, order, pseudo = {}, [], None
        for _ in range(n_bin):
            b, nc = struct.unpack_from("<Ii", bai, p)
            p += 8
            ch = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(nc)]
            p += 16 * nc
            if b == PSEUDO_BIN:
                assert nc == 2 and pseudo is None
                pseudo = (*ch[0], *ch[1])
            else:
                assert b not in bins and b < PSEUDO_BIN
                bins[b] = ch
            order.append(b)
        (n_intv,) = struct.unpack_from("<i", bai, p)
        io = list(struct.unpack_from(f"<{n_intv}Q", bai, p + 4))
        p += 4 + 8 * n_intv
        refs.append({"bins": bins, "order": order, "pseudo": pseudo, "ioffset": io})
    (nnc,) = struct.unpack_from("<Q", bai, p)
    assert p + 8 == len(bai), "trailing bytes"
    return {"refs": refs, "n_no_coor": nnc}


def check_invariants(bai: bytes) -> None:
    """Bins ascend with the pseudo-bin last; a bin's chunks are ordered and do not overlap; the linear
    index never decreases."""
    for ref in parse(bai)["refs"]:
        order = ref["order"]
        assert order == sorted(order)
        assert (ref["pseudo"] is not None) == bool(ref["bins"]) == bool(ref["ioffset"])
        for ch in ref["bins"].values():
            assert ch
            for k, (beg, end) in enumerate(ch):
                assert beg < end
                if k:
                    assert ch[k - 1][1] <= beg and ch[k - 1][1] >> 16 < beg >> 16
        io = ref["ioffset"]
        assert all(a <= b for a, b in zip(io, io[1:]))


# ------------------------------------------------------------------------------------------ query
class Reader:
    """Records of a BGZF BAM between two virtual offsets, decoded with zlib block by block."""

    def __init__(self, bam: bytes):
        self.bam = bam
        self.cache = {}

    def block(self, coff: int) -> tuple[bytes, int]:
        """-> (payload, file offset of the next block)"""
        if coff not in self.cache:
            bam = self.bam
            (xlen,) = struct.unpack_from("<H", bam, coff + 10)
            x, xend, bsize = coff + 12, coff + 12 + xlen, 0
            while x + 4 <= xend:
                (slen,) = struct.unpack_from("<H", bam, x + 2)
                if bam[x:x + 2] == b"BC" and slen == 2:
                    bsize = struct.unpack_from("<H", bam, x + 4)[0] + 1
                x += 4 + slen
            self.cache[coff] = (zlib.decompress(bam[xend:coff + bsize - 8], -15), coff + bsize)
        return self.cache[coff]

    def records(self, vbeg: int, vend: int):
        """Yield (voff, record bytes) for the records that start in [vbeg, vend)."""
        coff, u = vbeg >> 16, vbeg & 0xFFFF

        def take(k: int) -> bytes:
            nonlocal coff, u
            got = b""
            while len(got) < k:
                data, nxt = self.block(coff)
                if u >= len(data):
                    coff, u = nxt, 0
                    continue
                piece = data[u:u + k - len(got)]
                got += piece
                u += len(piece)
            return got

        while True:
            while coff < len(self.bam) and u >= len(self.block(coff)[0]):  # a block edge belongs to the next block
                coff, u = self.block(coff)[1], 0
            here = coff << 16 | u
            if here >= vend or coff >= len(self.bam):
                return
            head = take(4)
            yield here, head + take(struct.unpack("<I", head)[0])


def query(bai, bam: bytes, ref: int, beg: int, end: int, reader: "Reader | None" = None) -> list[bytes]:
    """The records of reference `ref` overlapping [beg, end), found through the index alone: the chunks of
    reg2bins(beg, end), cut at the linear index entry of beg's window; in file order.  bai: the image, or
    parse(image) when many regions are asked of one index (then pass one Reader(bam) too)."""
    r = (bai if isinstance(bai, dict) else parse(bai))["refs"][ref]
    io = r["ioffset"]
    if beg >> 14 >= len(io) or end <= beg:
        return []
    floor = io[beg >> 14]
    rd = reader or Reader(bam)
    # a merged chunk also covers the records of other bins that lie between its runs, so the ranges of
    # different bins can overlap: read their union, as every BAI reader does
    ranges = sorted((max(cb, floor), ce) for b in reg2bins(beg, end) for cb, ce in r["bins"].get(b, ()) if ce > floor)
    hits, done = [], 0
    for cb, ce in ranges:
        cb = max(cb, done)
        if cb >= ce:
            continue
        for _vo, rb in rd.records(cb, ce):
            refid, rbeg, rend, _ = span(rb)
            if refid == ref and rbeg < end and rend > beg:
                hits.append(rb)
        done = ce
    return hits


def brute(bam: bytes, ref: int, beg: int, end: int, _cache={}) -> list[bytes]:
    """The same by scanning every record of the file."""
    key = (id(bam), len(bam))
    if _cache.get("key") != key:
        raw = inflate_all(bam)
        _n, _b, offs = stream_layout(raw)
        rows = []
        for o in offs:
            rb = raw[o:o + 4 + struct.unpack_from("<I", raw, o)[0]]
            rows.append((*span(rb)[:3], rb))
        _cache.update(key=key, rows=rows, bam=bam)
    return [rb for refid, rbeg, rend, rb in _cache["rows"] if refid == ref and rbeg < end and rend > beg]
