"""The region-list predicate of `view / mergesort -L` (oge_filter_regions_dev), restated in plain Python.

A region is (ref_id, left_pos, right_pos) with the meaning of the oge_filter_opts fields.  A record passes a
region when
    refID == ref_id and pos + l_seq >= left_pos and pos <= right_pos
with pos + l_seq in 32-bit wrapping arithmetic, as the single-region Filter computes it.  A record passes a
list when it passes at least one of its regions; the other Filter settings (mapq, lengths, trim, count limit)
apply as they do with one region.
"""
from __future__ import annotations

import struct

INT32_MAX = (1 << 31) - 1


def wrap32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def core(rb: bytes) -> tuple[int, int, int, int]:
    """-> (refID, pos, mapq, l_seq) of one record (block_size included in rb)."""
    refid, pos, _lname, mapq = struct.unpack_from("<iiBB", rb, 4)
    (lseq,) = struct.unpack_from("<i", rb, 20)
    return refid, pos, mapq, lseq


def in_region(refid: int, pos: int, lseq: int, region) -> bool:
    ref, left, right = region
    return refid == ref and wrap32(pos + lseq) >= left and pos <= right


def keep_regions(records: list[bytes], regions, mapq_min: int = 0, min_len: int = 0, max_len: int = INT32_MAX,
                 trim_total: int = 0, count_limit: int = INT32_MAX) -> list[int]:
    """Indices of the records the filter keeps, in input order: a plain loop over the regions per record."""
    out = []
    for i, rb in enumerate(records):
        if len(out) >= count_limit:
            break
        refid, pos, mapq, lseq = core(rb)
        if not (mapq >= mapq_min and min_len <= lseq <= max_len and lseq > trim_total):
            continue
        if any(in_region(refid, pos, lseq, r) for r in regions):
            out.append(i)
    return out


def sorted_running_max(regions) -> tuple[list, list]:
    """What the device keeps of a list: the regions' (ref_id as unsigned, left_pos) in ascending order, and beside
    each the largest right_pos among the regions of its ref_id up to it."""
    order = sorted(regions, key=lambda r: (r[0] & 0xFFFFFFFF, r[1]))
    keys, rmax = [], []
    for ref, left, right in order:
        best = max(right, rmax[-1][1]) if keys and keys[-1][0] == ref & 0xFFFFFFFF else right
        keys.append((ref & 0xFFFFFFFF, left))
        rmax.append((ref & 0xFFFFFFFF, best))
    return keys, rmax


def in_regions_by_search(refid: int, pos: int, lseq: int, keys, rmax) -> bool:
    """One binary search per record: the regions of refID with left_pos <= pos + l_seq are a prefix of that
    refID's sorted regions, and one of them has right_pos >= pos exactly when their largest right_pos has."""
    import bisect

    k = bisect.bisect_right(keys, (refid & 0xFFFFFFFF, wrap32(pos + lseq)))
    return k > 0 and rmax[k - 1][0] == refid & 0xFFFFFFFF and rmax[k - 1][1] >= pos
