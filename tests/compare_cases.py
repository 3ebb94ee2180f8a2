"""Crafted record sets for `openge compare` (csrc/compare.hip): the smallest shapes at which its kernels can go wrong.

Every case is (records of file 0, records of the other file, region strings or None); all of them are defined by
the reference (op codes 0-8, contigs of the dictionary, records far below its reader's block_size limit), so the
recipe tests/golden/make_compare_goldens.py records the reference's text for each.

Geometry the shapes aim at: 64 lanes per wave, 256 threads per workgroup, 1024 records per key tile
(compare_tile_records), 16 ops up to which one lane hashes a CIGAR alone (compare_wide_ops), the 4096-key tile of
the radix sort."""
from __future__ import annotations

import random

import bamutil

REFS = [("chrA", 100000), ("chrB", 50000), ("chrC", 3000)]
TILE_RECORDS, WIDE_OPS = 1024, 16
TYPES = "MIDNSHP=X"


def header_text(refs=REFS) -> str:
    return "@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)


def rec(refid: int, pos: int, cigar: str = "", i: int = 0) -> bytes:
    return bamutil.make_record(f"r{i}", 0, refid, pos, cigar, "ACGT")


def recs_of(elements) -> list[bytes]:
    """[(refid, pos, cigar, multiplicity)] -> records, numbered"""
    out = []
    for refid, pos, cigar, mult in elements:
        for _ in range(mult):
            out.append(rec(refid, pos, cigar, len(out)))
    return out


def pack(records: list[bytes]):
    """(recs u8 with 16 bytes of slack, offs u64[n])"""
    recs, offs = bamutil.pack_records(records)
    return recs, offs[:-1]


def wide(last: str, n: int = 70) -> str:
    """n ops that differ from wide(other) only in the last one"""
    return "".join(f"{1 + k % 3}{'MI'[k % 2]}" for k in range(n - 1)) + last


def _ladder(n_pos: int, start: int = 0, refid: int = 0):
    """Positions with multiplicities 1..7 in file 0 and 1..5 in the other, three CIGARs: runs of 2..12 equal items
    over every wave, workgroup and tile edge of the sorted union"""
    cig = ("30M", "10M2I18M", "10M2D20M")
    a = [(refid, start + 3 * p, cig[p % 3], p % 7 + 1) for p in range(n_pos)]
    b = [(refid, start + 3 * p, cig[(p + (p % 11 == 0)) % 3], (p * 3) % 5 + 1) for p in range(n_pos)]
    return a, b


def cases() -> dict:
    out = {}
    la, lb = _ladder(40)
    out["equal"] = (recs_of(la), recs_of(la), None)
    out["empty_ref"] = ([], recs_of(la), None)
    out["empty_other"] = (recs_of(la), [], None)
    out["both_empty"] = ([], [], None)
    out["mult_3v5"] = (recs_of([(0, 100, "50M", 3)]), recs_of([(0, 100, "50M", 5)]), None)
    out["mult_5v3"] = (recs_of([(0, 100, "50M", 5)]), recs_of([(0, 100, "50M", 3)]), None)
    # 200 reads at one position, three CIGARs of one op count: only the hash (or the ops) tells them apart.  The
    # first two share the low 4 bits of compare.hip's hash, the third does not: at debug_hash_bits = 4 the run of
    # the first two is hard and the third is a run of its own.
    pile = ("10M5I10M", "10M3D10M", "11M4I10M")
    out["pile200"] = (recs_of([(0, 500, pile[0], 70), (0, 500, pile[1], 70), (0, 500, pile[2], 60)]),
                      recs_of([(0, 500, pile[0], 60), (0, 500, pile[1], 75), (0, 500, pile[2], 65)]), None)
    # 40 CIGARs of one op count at one position: more than the 16 values of a 4-bit hash, so some of them collide
    # there whatever the hash function is
    many = [f"{10 + k // 4}M{1 + k % 4}I20M" for k in range(40)]
    out["pile40"] = (recs_of([(0, 800, c, 2) for c in many]), recs_of([(0, 800, c, k % 3 + 1) for k, c in enumerate(many)]), None)
    # 70 ops (more than a wave's lanes), different in the last op alone, next to narrow CIGARs at the same place
    out["wide70"] = (recs_of([(0, 7, wide("5M"), 2), (0, 7, wide("6M"), 1), (0, 7, "9M", 1), (0, 7, wide("5M", 17), 1)]),
                     recs_of([(0, 7, wide("5M"), 1), (0, 7, wide("6M"), 2), (0, 7, wide("5S"), 1), (0, 7, wide("5M", 16), 1)]), None)
    # one length, every type: the order of the printed diff is the type CHARACTER's
    out["types"] = (recs_of([(0, 9, "10M", 1), (0, 9, "10=", 2), (0, 9, "10X", 1)] + [(1, 4, f"5{t}", 1) for t in "MDS"]),
                    recs_of([(0, 9, "10M", 2), (0, 9, "10=", 1), (0, 9, "10X", 1)] + [(1, 4, f"5{t}", 1) for t in TYPES]), None)
    out["no_ops"] = (recs_of([(0, 3, "", 2), (0, 3, "1M", 1), (0, 4, "", 1)]), recs_of([(0, 3, "", 3), (0, 4, "", 1), (1, 0, "", 1)]), None)
    # refID -1 and pos -1 belong to no region
    out["unplaced"] = (recs_of([(-1, -1, "", 3), (0, -1, "4M", 1), (-1, 50, "4M", 1), (0, 0, "4M", 1)]),
                       recs_of([(-1, -1, "", 1), (0, -1, "4M", 2), (0, 0, "4M", 1), (1, 0, "4M", 1)]), None)
    edge = [(0, 99, "8M", 1), (0, 100, "8M", 1), (0, 200, "8M", 1), (0, 201, "8M", 1), (1, 100, "8M", 1), (1, 150, "8M", 1)]
    out["bounds"] = (recs_of(edge[:3]), recs_of(edge), ["chrA:100..200", "chrA:100", "chrA:201", "chrB", "chrA:0..99"])
    out["overlap"] = (recs_of(la), recs_of(lb), ["chrA:0..60", "chrA:30..90", "chrA"])
    out["contigs"] = (recs_of(la + _ladder(20, 5, 1)[0] + [(2, 2999, "4M", 1)]), recs_of(lb + _ladder(20, 5, 1)[1] + [(2, 0, "4M", 1)]),
                      ["chrB", "chrA", "chrC:2999", "chrC"])
    # a run of equal items across lane 64 / thread 256 / record 1024 / key 4096 of the sorted union
    for edge_at in (64, 256, 1024, 4096):
        singles = [(0, p, "20M", 1) for p in range(edge_at // 2 - 3)]
        run = [(0, 50000, "20M", 9)]
        out[f"straddle{edge_at}"] = (recs_of(singles + run), recs_of(singles + [(0, 50000, "20M", 4)]), None)
    big_a, big_b = _ladder(1250)  # about 5000 records a side
    out["ladder"] = (recs_of(big_a), recs_of(big_b), None)
    rnd = random.Random(7)
    ua, ub = recs_of(big_a + _ladder(100, 11, 1)[0]), recs_of(big_b + _ladder(100, 11, 1)[1])
    rnd.shuffle(ua)
    rnd.shuffle(ub)
    out["unsorted"] = (ua, ub, ["chrA:300..2000", "chrB"])
    return out


def hard_cases() -> tuple[str, ...]:
    """cases where one (position, op count) holds two CIGARs: hard runs once the hash is narrowed to 0 bits"""
    return ("pile200", "pile40", "wide70", "types")
