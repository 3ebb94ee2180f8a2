"""Crafted inputs for the stats / count / coverage tests (CPU model tests and GPU tests share them): the smallest
shapes at which each kernel of csrc/qc.hip can go wrong.  A case is (refs, records); `bam_bytes` makes the file."""
from __future__ import annotations

import random
import struct

import numpy as np

import bamutil

# csrc/qc.hip: a wave walks WAVE_RECS consecutive records in steps of STEP, a workgroup BLOCK_RECS; lengths below
# LEN_TAB go through the LDS table; a coverage tile is COV_TILE records, its LDS window COV_WIN bins
# (tests/test_gpu_qc.py checks these against the library's counters)
STEP, WAVE_RECS, BLOCK_RECS, LEN_TAB, COV_TILE, COV_WIN = 64, 1024, 4096, 4096, 1024, 4096
EDGES = (STEP, WAVE_RECS, BLOCK_RECS)
FLAG_BITS = (0x1, 0x2, 0x4, 0x8, 0x10, 0x40, 0x80, 0x200, 0x400)
REFS1 = [("chr1", 1 << 29)]
REFS6 = [(f"chr{j}", 1 << 29) for j in range(1, 7)]


def rec(i, refid, pos, flag=0, lseq=10, tlen=0, mref=-1, mpos=-1) -> bytes:
    """bamutil.make_record's bytes for a read of `lseq` bases '=' with no CIGAR, built without a per-base loop."""
    nm = f"r{i}".encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(nm), 60, 4680, 0, flag, lseq, mref, mpos, tlen)
    body += nm + bytes((lseq + 1) // 2) + bytes([30]) * lseq
    return struct.pack("<I", len(body)) + body


def header_text(refs) -> str:
    return "@HD\tVN:1.4\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)


def bam_bytes(refs, records, tmp_path) -> bytes:
    p = tmp_path / "qc_case.bam"
    bamutil.write_bam_py(p, header_text(refs), refs, records)
    return p.read_bytes()


def pack(records):
    """(recs u8 with 16 bytes of slack, offs u64[n])"""
    recs, offs = bamutil.pack_records(records)
    return recs, offs[:-1]


# ------------------------------------------------------------------------------------------------ flags and sizes
def flag_seq(n: int, seed: int = 5) -> list[int]:
    """All 512 combinations of the nine bits first (shuffled), then bits drawn with a probability of their own
    each, so that no two of the twelve counters agree."""
    rng = random.Random(seed)
    combos = [sum(b for k, b in enumerate(FLAG_BITS) if c >> k & 1) for c in range(512)]
    rng.shuffle(combos)
    prob = (0.83, 0.61, 0.07, 0.13, 0.42, 0.55, 0.38, 0.03, 0.19)
    out = combos[:n]
    while len(out) < n:
        out.append(sum(b for b, p in zip(FLAG_BITS, prob) if rng.random() < p))
    return out


def sized(n: int):
    """n sorted reads on one contig with cycling flags, lengths 10..16 and insert sizes of both signs."""
    fl = flag_seq(n)
    return REFS1, [rec(i, 0, 100 + 3 * i, fl[i], 10 + i % 7, (i * 37 % 1000) * (-1 if i % 3 == 0 else 1)) for i in range(n)]


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, BLOCK_RECS + 1)
FLAGS_N = 512 + 1500


# ------------------------------------------------------------------------------------------------ sorted
def keyed(keys):
    return [rec(i, r, p) for i, (r, p) in enumerate(keys)]


def _asc(n, rid=0):
    return [(rid, 100 + i) for i in range(n)]


def sorted_cases() -> dict:
    """{name: (keys, expected Sorted)}; keys are (refID, pos)."""
    out = {}
    for e in EDGES:
        n = e + 70
        for c in (e - 1, e, e + 1, e + 2):  # the violating triple (c-2, c-1, c) at every alignment across the edge
            k = _asc(n)
            k[c] = (0, 0)
            out[f"triple_e{e}_c{c - e:+d}"] = (k, False)
        for s in (e - 2, e - 1, e):  # a run start on the edge: 100, 50, 60 is sorted, 100, 150, 60 is not
            k = _asc(s) + [(1, 100), (1, 50)] + [(1, 60 + i) for i in range(n - s - 2)]
            out[f"runstart_e{e}_s{s - e:+d}"] = (k, True)
            k = _asc(s) + [(1, 100), (1, 150)] + [(1, 60 + i) for i in range(n - s - 2)]
            out[f"runstart_bad_e{e}_s{s - e:+d}"] = (k, False)
        k = _asc(e, rid=1) + _asc(70, rid=0)  # a refID decrease exactly on the edge
        out[f"rid_down_e{e}"] = (k, False)
    # the middle considered record a whole workgroup back: a workgroup of unplaced records in between
    gap = [(-1, -1)] * (BLOCK_RECS + 2)
    for c0, good in ((0, False), (5000, True)):
        k = _asc(BLOCK_RECS - 2) + gap + [(0, c0)] + [(0, 6000 + i) for i in range(30)]
        out[f"block_back_{'ok' if good else 'bad'}"] = (k, good)
    # ... and both predecessors behind unplaced stretches of their own
    k = _asc(WAVE_RECS - 1) + [(-1, -1)] * WAVE_RECS + [(0, 5000)] + [(-1, -1)] * (BLOCK_RECS + 7) + [(0, 4999)]
    out["two_gaps_bad"] = (k, False)
    k = [(-1, -1)] * (BLOCK_RECS + 3) + [(2, 100), (2, 50), (2, 60)]  # the file's first considered record is exempt
    out["leading_gap_ok"] = (k, True)
    # pos -1 with a valid refID is not considered (and raises no refID)
    out["pos_minus1_ok"] = ([(0, 100), (0, 150), (5, -1), (0, -1), (0, 160), (1, 0)], True)
    out["pos_minus1_bad"] = ([(0, 100), (0, 150), (0, -1), (0, 140)], False)
    out["three_ok"] = ([(0, 100), (0, 50), (0, 60)], True)
    out["three_bad"] = ([(0, 100), (0, 150), (0, 60)], False)
    out["only_unplaced"] = ([(-1, -1)] * 70, True)
    return out


# ------------------------------------------------------------------------------------------------ lengths
def length_cases() -> dict:
    big = 70_000
    return {
        "len_0_1": (REFS1, [rec(i, 0, 100 + i, lseq=l) for i, l in enumerate((0, 1, 1, 0, 1))]),
        "len_3000": (REFS1, [rec(i, 0, 100 + i, lseq=i % 3000) for i in range(3300)]),
        "len_big": (REFS1, [rec(i, 0, 100 + i, lseq=l)
                            for i, l in enumerate((50, big, LEN_TAB - 1, LEN_TAB, 5000, 50, LEN_TAB, 5000, 5000, LEN_TAB + 1))]),
    }


# ------------------------------------------------------------------------------------------------ inserts
def insert_recs(tlens, noise: bool = True):
    """First mates with the given tlen (signs alternate), with second mates, unpaired reads and tlen 0 mixed in."""
    out, i = [], 0
    for k, t in enumerate(tlens):
        out.append(rec(i, 0, 100 + i, 0x41, tlen=t if t == -(1 << 31) else (-t if k % 2 else t)))
        i += 1
        if noise:
            out.append(rec(i, 0, 100 + i, 0x81, tlen=7))       # second mate
            out.append(rec(i + 1, 0, 101 + i, 0x40, tlen=9))   # first-mate bit without the paired bit
            out.append(rec(i + 2, 0, 102 + i, 0x41, tlen=0))   # tlen 0
            i += 3
    return REFS1, out


def insert_cases() -> dict:
    out = {f"ins_n{m}": insert_recs([300, 100, 200, 400][:m]) for m in range(5)}
    out["ins_n0"] = (REFS1, insert_recs([300])[1][1:])  # no qualifying read among second mates, unpaired reads and tlen 0
    out["ins_equal"] = insert_recs([250] * 9)
    out["ins_ties"] = insert_recs([100, 200, 200, 200, 300, 200])
    for v in (1 << 10, 1 << 11, 1 << 21, 1 << 22):  # the radix digits' edges (10 | 11 | 11 bits from the bottom)
        out[f"ins_edge{v}_odd"] = insert_recs([v + 1, v - 1, v])
        out[f"ins_edge{v}_lo"] = insert_recs([v, v - 1])
        out[f"ins_edge{v}_hi"] = insert_recs([v + 1, v, 3, (1 << 31) - 1])
    out["ins_small"] = insert_recs([1, 2, 1, 3])
    out["ins_max"] = insert_recs([(1 << 31) - 2, (1 << 31) - 1, -(1 << 31), 5, -(1 << 31)])
    rng = random.Random(11)
    out["ins_many"] = insert_recs([rng.choice((rng.randint(1, 700), rng.randint(1, (1 << 31) - 1))) for _ in range(3001)], noise=False)
    return out


def stats_cases() -> dict:
    """Every crafted stats input: {name: (refs, records)}."""
    out = {f"n{n}": sized(n) for n in SIZES}
    out["flags512"] = sized(FLAGS_N)
    out.update({f"sorted_{k}": (REFS6, keyed(v[0])) for k, v in sorted_cases().items()})
    out.update(length_cases())
    out.update(insert_cases())
    return out


# ------------------------------------------------------------------------------------------------ coverage
BINSIZES = (1, 7, 100, 10_000_000, 1 << 30)


def coverage_cases() -> dict:
    """{name: (refs, records, defined)}; defined: the reference defines the result (it can read every record, and
    every counted position lies in its contig's bins) at every bin size."""
    out = {}
    basic = [rec(0, 0, 0, lseq=10), rec(1, 0, 989, lseq=10),       # pos 0; the last counted position is 999
             rec(2, 0, 500, lseq=0), rec(3, 0, 510, flag=0x4),      # one position; a placed unmapped read
             rec(4, -1, -1, flag=0x4), rec(5, 0, -1), rec(6, -1, 77),  # skipped
             rec(7, 0, 93, lseq=14), rec(8, 0, 100, lseq=99)]
    out["basic"] = ([("c", 1000)], basic, True)
    out["past_end"] = ([("c", 1000), ("d", 50)], basic + [rec(9, 0, 995, lseq=10), rec(10, 1, 49, lseq=3), rec(11, 0, 2000, lseq=5),
                                                          rec(12, 1, -5, lseq=9)], False)
    out["contention"] = ([("c", 100_000)], [rec(i, 0, 4321, lseq=100) for i in range(5000)], True)
    out["long70k"] = ([("c", 200_000)], [rec(0, 0, 10, lseq=50), rec(1, 0, 1000, lseq=70_000), rec(2, 0, 1500, lseq=90),
                                         rec(3, 0, 150_000, lseq=200)], False)  # the reference's reader refuses the record
    rng = random.Random(3)
    refs = [("a", 600_000), ("b", 600_000), ("c", 300_000)]  # at bin size 100 more bins than one window
    out["unsorted_wide"] = (refs, [rec(i, (r := rng.randrange(3)), rng.randrange(refs[r][1] - 300), lseq=rng.randint(0, 250))
                                   for i in range(2 * COV_TILE + 77)], True)
    # sorted reads with one wide tile: most tiles take the window, one falls back
    srt = sorted((rng.randrange(0, 40_000) for _ in range(3 * COV_TILE)))
    recs = [rec(i, 0, p, lseq=100) for i, p in enumerate(srt)]
    recs[COV_TILE + 5] = rec(COV_TILE + 5, 1, 590_000, lseq=100)
    out["sorted_window"] = (refs, recs, True)
    out["name_order"] = ([("chrB", 3000), ("chrA", 2000), ("chrC", 700)],
                         [rec(0, 0, 5, lseq=100), rec(1, 1, 1500, lseq=100), rec(2, 0, 2899, lseq=100), rec(3, 1, 0, lseq=30)], True)
    out["n_ref0"] = ([], [rec(0, -1, -1, flag=0x4), rec(1, -1, -1, flag=0x4)], True)
    return out
