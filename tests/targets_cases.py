"""Crafted record sets for `openge targets` (csrc/targets.hip): the smallest shapes at which its kernels can go wrong.

Every case is (records, refs).  Geometry the shapes aim at: 64 lanes per wave, 256 threads per workgroup, 1024
records per tile of the event pass (counter targets_tile_records: one append atomic), 1024 sorted events per tile of
the running maximum (targets_merge_tile), the 4096-key tile of the radix sort."""
from __future__ import annotations

import random
import struct

import bamutil

REFS = [("chrA", 100000), ("chrB", 50000), ("chrC", 3000)]
TILE_RECORDS, MERGE_TILE, SORT_TILE = 1024, 1024, 4096
GAPS = (0, 1, 10)
MAX_INTERVALS = (500, 100000)


def header_text(refs=REFS) -> str:
    return "@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)


def rec(refid: int, pos: int, cigar: str = "", i: int = 0, flag: int = 0, mapq: int = 60, mref: int = -1) -> bytes:
    return bamutil.make_record(f"r{i}", flag, refid, pos, cigar, "ACGT", None, mapq, mref, -1 if mref < 0 else pos)


def recs_of(elements) -> list[bytes]:
    """[(refid, pos, cigar) or (refid, pos, cigar, {flag, mapq, mref})] -> records, numbered"""
    return [rec(e[0], e[1], e[2], i, **(e[3] if len(e) > 3 else {})) for i, e in enumerate(elements)]


def indels(n: int) -> str:
    """a CIGAR of 2 n + 1 ops with n interior indels, insertions and deletions by turns"""
    return "2M" + "".join(f"{1 + k % 3}{'ID'[k % 2]}2M" for k in range(n))


def wide(n: int = 70) -> str:
    """n ops, M and I by turns, M at both ends"""
    assert n % 2 == 0
    return "".join(f"{1 + k % 3}{'MI'[k % 2]}" for k in range(n - 2)) + "2M3M"


def chain(n: int, start: int = 1000, refid: int = 0):
    """n deletions of 5, each overlapping the next: one interval of 3 n + 2 bases"""
    return [(refid, start + 3 * k, "5M5D5M") for k in range(n)]


def cases() -> dict:
    out = {}
    out["empty"] = ([], REFS)
    out["no_events"] = (recs_of([(0, 10 * k, "30M") for k in range(70)] + [(1, 5, ""), (2, 7, "4S")]), REFS)
    out["one_event"] = (recs_of([(0, 100, "10M2D10M")]), REFS)
    # events in the last record of a wave, a workgroup's row and a tile, and in the first of the next
    plain = [(0, 7 * k, "20M") for k in range(TILE_RECORDS + 70)]
    for at in (63, 64, 255, 256, TILE_RECORDS - 1, TILE_RECORDS):
        plain[at] = (1, 40 * at, "10M3D10M" if at % 2 else "10M2I10M")
    out["tile_edge"] = (recs_of(plain), REFS)
    out["sixty_indels"] = (recs_of([(0, 50, "30M"), (0, 100, indels(60)), (1, 9, "10M1I10M")]), REFS)
    # every read carries 60 events: the arena is 60 times the records, over more than one tile
    out["all_sixty"] = (recs_of([(k % 2, 11 * k, indels(60)) for k in range(TILE_RECORDS + 40)]), REFS)
    out["seventy_ops"] = (recs_of([(0, 200, wide(70)), (0, 5000, wide(70)), (1, 10, "20M")]), REFS)
    # the read filter: every line but the marked ones gives nothing
    ev = "10M2D10M"
    out["filters"] = (recs_of([(0, 100, ev, dict(flag=0x4)), (0, 300, ev, dict(flag=0x100)), (0, 500, ev, dict(flag=0x200)),
                               (0, 700, ev, dict(flag=0x400)), (0, 900, ev, dict(mapq=0)), (0, 1100, ev, dict(mapq=255)),
                               (0, 1300, ev, dict(flag=0x1, mref=1)),          # a bad mate
                               (0, 1500, ev, dict(flag=0x1 | 0x8, mref=1)),    # kept: the mate is unmapped
                               (0, 1700, ev, dict(flag=0x1, mref=0)),          # kept: the mate on the same contig
                               (0, 1900, ev, dict(mref=1)),                    # kept: not paired
                               (-1, 2100, ev), (0, -1, ev), (-1, -1, ev),
                               (0, 2300, ev, dict(flag=0x10 | 0x800, mapq=1)),  # kept: other bits, MAPQ 1
                               (0, 2500, ev, dict(mapq=254))]), REFS)           # kept
    out["edge_indels"] = (recs_of([(0, 100, "2I10M"), (0, 200, "10M2D"), (0, 300, "5S2I10M"), (0, 400, "5H5S10M2I3S"),
                                   (0, 500, "10M2I10M5S"), (0, 600, "3D10M2I"), (0, 700, "2I"), (0, 800, "5S")]), REFS)
    out["n_and_p"] = (recs_of([(0, 100, "10M100N5M2D5M"), (0, 1000, "5M2P5M1I5M"), (0, 2000, "5M10N5M"), (0, 3000, "5M3N2D4P1I5M")]), REFS)
    out["eq_x"] = (recs_of([(0, 100, "5=2I5X"), (0, 300, "5X3D5="), (0, 500, "10M2I3D10M"), (0, 700, "4S5=1D5=4S"), (0, 900, "5S2D5=1I5X")]),
                   REFS)
    # A [100,400] encloses B [110,111], C [300,301] and D [390,395]; E [401,402] is apart at gap 0 and joins at gap 1
    out["enclose"] = (recs_of([(0, 90, "10M300D10M"), (0, 100, "10M1I10M"), (0, 290, "10M1I10M"), (0, 380, "10M5D10M"),
                               (0, 391, "10M1I10M")]), REFS)
    out["copies3000"] = (recs_of([(1, 777, "10M4D10M")] * 3000), REFS)
    out["chain5000"] = (recs_of(chain(5000)), REFS)
    out["width_499_500"] = (recs_of([(0, 1000, "10M499D10M"), (0, 5000, "10M500D10M"), (0, 9000, "10M501D10M"), (1, 100, "10M1D10M")]), REFS)
    # contig 0 ends with a stop of 90000, contig 1 begins with an event at 5
    out["contigs3"] = (recs_of([(0, 10, "10M1I10M"), (0, 89590, "10M400D10M"), (1, 0, "5M1I5M"), (1, 49000, "10M2D10M"), (2, 0, "1M1D1M"),
                                (2, 2000, "10M2I10M")]), REFS)
    # anchored on the last base of chrC: the stop is clipped, start = stop; a deletion running out of chrC
    out["clip_end"] = (recs_of([(2, 2990, "10M2I5M"), (1, 49900, "50M200D5M")]), REFS)
    big = [("big", 2147483647), ("small", 1000)]
    out["widths"] = (recs_of([(0, 10 ** w - 6, "5M1I5M") for w in range(1, 10)] + [(1, 94, "5M1I5M"), (0, 2147483600, "5M1I5M")]), big)
    mixed = (chain(1500, 1000) + chain(1500, 1002, 1) + [(1, 777, "10M4D10M")] * 700 + [(0, 60000 + 13 * k, indels(k % 7)) for k in range(900)] +
             [(0, 90, "10M300D10M"), (0, 100, "10M1I10M"), (0, 391, "10M1I10M"), (0, 89590, "10M400D10M"), (1, 0, "5M1I5M"),
              (2, 2990, "10M2I5M"), (0, 30000, ev, dict(flag=0x400)), (0, 30100, wide(70))])
    out["mixed"] = (recs_of(mixed), REFS)
    shuffled = list(mixed)
    random.Random(11).shuffle(shuffled)
    out["mixed_shuffled"] = (recs_of(shuffled), REFS)
    return out


def patched(rb: bytes, n_cigar: int | None = None, op0: int | None = None) -> bytes:
    """rb with its op count or its first op overwritten"""
    b = bytearray(rb)
    if n_cigar is not None:
        struct.pack_into("<H", b, 16, n_cigar)
    if op0 is not None:
        struct.pack_into("<I", b, 36 + b[12], op0)
    return bytes(b)


def error_cases() -> dict:
    """name -> (records, refs, the record the error names, its kind as targets_model.BAD numbers them)"""
    good = [(0, 10 * k, "10M2D10M") for k in range(300)]
    out = {}
    r = recs_of(good + [(3, 5, "10M")] + good[:5] + [(7, 5, "10M")])
    out["refid"] = (r, REFS, 300, 0)
    r = recs_of(good)
    r[257] = patched(r[257], n_cigar=4000)
    out["cigar_size"] = (r, REFS, 257, 1)
    r = recs_of(good)
    r[70] = patched(r[70], op0=(10 << 4) | 9)
    r[290] = patched(r[290], n_cigar=4000)
    out["op_code"] = (r, REFS, 70, 2)
    # the same faults in reads the filter drops: no error
    r = recs_of(good[:5] + [(3, 5, "10M", dict(flag=0x4)), (0, 5, "10M", dict(mapq=0))])
    r[6] = patched(r[6], op0=(10 << 4) | 12)
    out["filtered_faults"] = (r, REFS, None, None)
    return out
