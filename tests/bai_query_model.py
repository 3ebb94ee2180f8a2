"""The index query of oge_bai_query[_dev], restated in plain Python on top of bai_model.parse / reg2bins.

Region (ref_id, left_pos, right_pos) asks for the reference positions [max(0, left_pos - widen),
min(right_pos + 1, 2^29)) of ref_id: every chunk of the bins of that interval, cut at the linear index entry of
the interval's first 16 Ki window.  The result is the union of all those half-open virtual-offset intervals:
overlapping and touching ones joined, empty ones dropped, ascending.
"""
from __future__ import annotations

import struct

import bai_model as M

MAX_END = 1 << 29
# the largest l_seq the device record walk admits lies below its block_size cap (inflate.hip: 32..10000)
WIDEN = 10000


def union(ranges) -> list[tuple[int, int]]:
    out = []
    for b, e in sorted(r for r in ranges if r[1] > r[0]):
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return [tuple(r) for r in out]


def raw_ranges(parsed: dict, regions, widen: int = 0) -> list[tuple[int, int]]:
    out = []
    refs = parsed["refs"]
    for ref, left, right in regions:
        qb, qe = max(0, left - widen), min(right + 1, MAX_END)
        if not 0 <= ref < len(refs) or qb >= qe:
            continue
        io = refs[ref]["ioffset"]
        if qb >> 14 >= len(io):
            continue
        floor = io[qb >> 14]
        for b in M.reg2bins(qb, qe):
            for cb, ce in refs[ref]["bins"].get(b, ()):
                cb = max(cb, floor)
                out.append((cb, max(ce, cb)))
    return out


def merged_ranges(bai, regions, widen: int = 0) -> list[tuple[int, int]]:
    parsed = bai if isinstance(bai, dict) else M.parse(bai)
    return union(raw_ranges(parsed, regions, widen))


def serialise(parsed: dict, reverse_bins: bool = False, n_no_coor: bool = True) -> bytes:
    """A parsed image back into bytes; reverse_bins: every reference's bins in descending order, the pseudo-bin
    first -- as valid a BAI as the ascending one."""
    out = [b"BAI\1", struct.pack("<i", len(parsed["refs"]))]
    for r in parsed["refs"]:
        bins = [(b, list(ch)) for b, ch in r["bins"].items()]
        if r["pseudo"] is not None:
            p = r["pseudo"]
            bins.append((M.PSEUDO_BIN, [(p[0], p[1]), (p[2], p[3])]))
        if reverse_bins:
            bins.reverse()
        out.append(struct.pack("<i", len(bins)))
        for b, ch in bins:
            out.append(struct.pack("<Ii", b, len(ch)))
            out.extend(struct.pack("<QQ", *c) for c in ch)
        out.append(struct.pack(f"<i{len(r['ioffset'])}Q", len(r["ioffset"]), *r["ioffset"]))
    if n_no_coor:
        out.append(struct.pack("<Q", parsed["n_no_coor"]))
    return b"".join(out)


def with_empty_ref(parsed: dict, at: int) -> tuple[dict, callable]:
    """The image with a reference without records inserted at index `at`; -> (parsed, map of old ref ids)."""
    refs = list(parsed["refs"])
    refs.insert(at, {"bins": {}, "order": [], "pseudo": None, "ioffset": []})
    return {"refs": refs, "n_no_coor": parsed["n_no_coor"]}, (lambda r: r + 1 if r >= at else r)
