"""Crafted record sets for the duplicate-set pass (csrc/dupsets.hip): the smallest shapes at which its kernels can go
wrong.  Every case is (header text, records, distances).  Geometry the shapes aim at: 64 lanes per wave (counter
dupsets_wave_cap), 256 threads per workgroup, BLOCK_CAP members of a set in one workgroup's LDS (counter
dupsets_block_cap; one member more goes to the host).

A pair is two records of one name and read group; a set is the pairs placed at one (pos1, pos2).  Sets are laid out
at ascending positions, so the sorted order of the sets of one library, contig and orientation is the order in which
a case creates them: that is what puts a given set across a wave's 64-lane edge."""
from __future__ import annotations

import random

import bamutil
from dupmetrics_cases import REFS, header_text, rg

WAVE_CAP, BLOCK_CAP = 64, 1024
HEADER = header_text([("a1", "libA"), ("a2", "libA"), ("b1", "libB")])


def name7(tile, x, y, k) -> str:
    return f"M{k}:7:FC:1:{tile}:{x}:{y}"


def name5(tile, x, y, k) -> str:
    return f"M{k}:3:{tile}:{x}:{y}"


def pair(name: str, pos1: int, pos2: int, rgid: bytes = b"a1", ref1: int = 0, ref2: int = 0, rev1: bool = False, rev2: bool = True,
         left_is_first: bool = True) -> list[bytes]:
    """The two ends of one pair, the left one first: 4M reads at (ref1, pos1) and (ref2, pos2).  left_is_first: the
    left end has FLAG 0x40, else 0x80."""
    tags = rg(rgid) if rgid is not None else b""
    f1 = 0x1 | (0x10 if rev1 else 0) | (0x20 if rev2 else 0) | (0x40 if left_is_first else 0x80)
    f2 = 0x1 | (0x10 if rev2 else 0) | (0x20 if rev1 else 0) | (0x80 if left_is_first else 0x40)
    return [bamutil.make_record(name, f1, ref1, pos1, "4M", "ACGT", None, 30, ref2, pos2, 0, tags),
            bamutil.make_record(name, f2, ref2, pos2, "4M", "ACGT", None, 30, ref1, pos1, 0, tags)]


class Builder:
    """Sets at ascending positions; every pair gets a name of its own."""

    def __init__(self):
        self.records: list[bytes] = []
        self.k = 0
        self.pos = 100

    def add_set(self, locs, **kw):
        """locs: one (tile, x, y), or None for a name without a location, per pair of the set"""
        self.pos += 10
        for j, loc in enumerate(locs):
            self.k += 1
            if loc is None:
                nm = f"plain{self.k}"
            elif (self.k + j) % 3 == 0:
                nm = name5(*loc, self.k)
            else:
                nm = name7(*loc, self.k)
            self.records += pair(nm, self.pos, self.pos + 300, **kw)
        return self


def spread(n: int, k0: int = 0):
    """n locations on two tiles, some of them within 100 of one another in chains of assorted lengths"""
    return [((k0 + k) % 2 + 1, ((k0 + k) * 37) % 1500, ((k0 + k) * 91) % 700) for k in range(n)]


def sized_case(sizes) -> tuple[str, list[bytes], tuple]:
    b = Builder()
    for s in sizes:
        b.add_set(spread(s, b.k))
    return HEADER, b.records, (100,)


def chain_orders() -> tuple[str, list[bytes], tuple]:
    """A-B-C with A and C 2 D apart, in all six orders: 2 optical duplicates each.  At D + 1 the same; at D - 1 none."""
    import itertools
    b = Builder()
    pts = [(5, 1000, 1000), (5, 1100, 1000), (5, 1200, 1000)]
    for order in itertools.permutations(pts):
        b.add_set(list(order))
    return HEADER, b.records, (100, 101, 99)


def cases() -> dict:
    out = {}
    out["n0"] = (HEADER, [], (100,))
    out["no_pairs"] = (HEADER, [bamutil.make_record(f"M{i}:7:FC:1:1:{i}:{i}", 0, 0, 100 + i % 3, "4M", "ACGT", None, 30, -1, -1, 0, rg(b"a1"))
                                for i in range(70)], (100,))
    # 1, 2, 63, 64, 65 pairs in a set: a lane, a wave less one, a wave, a wave and one (the workgroup tier)
    out["sizes_small"] = sized_case((1, 2, 63, 64, 65, 1, 3))
    out["block_m1"] = sized_case((2, BLOCK_CAP - 1, 2))
    out["block"] = sized_case((BLOCK_CAP, 5))
    out["block_p1"] = sized_case((3, BLOCK_CAP + 1, 2))   # the host tier
    # 20 sets of 3 fill lanes 0..59; the set of 7 would lie in lanes 60..66: it is taken whole in the second round
    out["straddle"] = sized_case((3,) * 20 + (7,) + (2,) * 30 + (64,) + (5,) * 3)
    # runs of two-pair sets that end one short of, at and one past a wave's and a workgroup's edge; a set of 3 in front
    # moves every later edge into the middle of a set
    for n in (31, 32, 33, 127, 128, 129):
        b = Builder()
        for k in range(n):
            b.add_set([(1, 500, 500), (1, 500 + (k % 3) * 60, 520)])  # dx 0, 60, 120: close, close, not close at 100
        out[f"twos{n}"] = (HEADER, b.records, (100,))
        b = Builder().add_set([(1, 1, 1), (1, 2, 2), (2, 1, 1)])
        for k in range(n):
            b.add_set([(1, 500, 500), (1, 500 + (k % 3) * 60, 520)])
        out[f"three_twos{n}"] = (HEADER, b.records, (100,))
    out["chain"] = chain_orders()
    close = [(1, 100, 100), (1, 110, 110)]
    b = Builder()
    b.add_set(close, rgid=b"a1")
    b.pos -= 10
    b.add_set(close, rgid=b"b1")            # the same coordinates in two libraries: two sets
    b.add_set(close + close, rgid=b"a1")
    b.pos -= 10
    b.add_set(close, rgid=b"a2")            # two read groups of one library in one set: never close to one another
    b.add_set([(1, 100, 100), (2, 100, 100), (1, 100, 300), (300, 100, 100)])   # different tiles, far apart in y
    b.add_set(close, rgid=None)             # no RG tag: read group -1, the unknown library
    b.pos -= 10
    b.add_set(close, rgid=b"nobody")        # an unlisted value: the same set, also read group -1
    out["libs_rgs_tiles"] = (HEADER, b.records, (100,))
    b = Builder()
    b.add_set(close)                                        # FR, both lefts first: 1
    b.pos -= 10
    b.add_set(close[:1], left_is_first=False)               # the same FR set, a left end that is second: its own part
    b.add_set(close, rev2=False)                            # FF
    b.pos -= 10
    b.add_set(close[:1], rev2=False, left_is_first=False)   # the same FF set: not divided, all three close
    b.add_set(close, rev1=True, rev2=True)                  # RR
    b.pos -= 10
    b.add_set(close[1:], rev1=True, rev2=True, left_is_first=False)
    b.add_set(close, rev1=True, rev2=False)                 # RF
    b.pos -= 10
    b.add_set(close[:1], rev1=True, rev2=False, left_is_first=False)
    b.add_set(close + close, ref2=1)                        # mates on two contigs
    b.add_set(close, ref1=1, ref2=1)
    out["orientations_contigs"] = (HEADER, b.records, (100,))
    b = Builder()
    b.add_set([(1, 50, 50), (1, 50, 50), (1, 50, 51), (1, 51, 50), (1, 50, 50)])   # D = 0: equal locations only
    b.add_set([(1, -50, 50), (1, 40, 50), (1, -50, -40)])                          # negative coordinates
    out["d0"] = (HEADER, b.records, (0, 1, 90))
    b = Builder()
    b.add_set([(1, 10, 10), None, (1, 20, 20), None, None])
    b.add_set([None, None])
    b.add_set([None])
    b.add_set([(1, 10, 10)])
    # field counts 4, 5, 6, 7, 8; junk behind the digits; an empty field; a sign; a name longer than the summary's slot
    names = ["a:1:10:10", "a:1:10:10:10", "a:b:1:10:10:10", "a:b:c:d:1:10:10", "a:b:c:d:e:1:10:10", "q:w:1:12#0/1:12abc", "e:r:1::14",
             "t:y:1:-3:9", "t:y:1:-:9", "x" * 30 + ":u:1:15:15"]
    b.pos += 10
    for nm in names:
        b.records += pair(nm, b.pos, b.pos + 300)
    out["names"] = (HEADER, b.records, (100,))
    mixed = sized_case((5, 1, 70, 2, 2, 9, 64, 3))
    out["mixed"] = mixed
    # the same pairs in another record order: every first end, then every second end, each in an order of its own
    rnd = random.Random(5)
    firsts, seconds = mixed[1][0::2], mixed[1][1::2]
    rnd.shuffle(firsts)
    rnd.shuffle(seconds)
    out["mixed_shuffled"] = (HEADER, firsts + seconds, (100,))
    return out
