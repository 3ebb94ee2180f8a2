"""Python restatement of the duplicate-set pass (csrc/dupsets.hip, oge_dup_sets_text of host_capi.cpp; DESIGN.md
section 27; include/openge_hip.h states the same definition).  The yardstick of the tests: nothing here calls the
library.

Pairs and sets are the dedup's: they are taken from tests/dupcheck.py (expected_dups(..., debug=...): pr1, pr2, pgid),
which restates the pairing and the chunks independently of the product.  Everything else -- the location of a pair,
the division of FR / RF sets, "close", the components, the histograms, the text -- is defined here."""
from __future__ import annotations

import math
import struct

import numpy as np

import dupmetrics_model as DM

BINS = 1024
FIELDS = ("pairs", "sets", "located", "optical")
HIST_COLUMNS = ("all_sets", "optical_sets", "non_optical_sets")


# ------------------------------------------------------------------------------------------- the location
def number(b: bytes) -> int:
    """An optional '-', then decimal digits up to the first other byte; no digit gives 0.  (Held in int32 by the
    product: more than 9 digits are outside the definition.)"""
    k, neg = 0, False
    if b[:1] == b"-":
        k, neg = 1, True
    v = 0
    while k < len(b) and 0x30 <= b[k] <= 0x39:
        v = v * 10 + b[k] - 0x30
        k += 1
    return -v if neg else v


def location(name: bytes) -> tuple[int, int, int] | None:
    """(tile, x, y): the last three of exactly 5 or exactly 7 ':'-separated fields; None for any other count."""
    f = name.split(b":")
    if len(f) not in (5, 7):
        return None
    return number(f[-3]), number(f[-2]), number(f[-1])


def read_name(rb: bytes) -> bytes:
    return bytes(rb[36:36 + rb[12]]).split(b"\0")[0]


def rg_ids(header_text: str) -> list[bytes]:
    """The ids of the @RG lines in header order: the read-group index is the first position of a value in it."""
    out = []
    for line in header_text.splitlines():
        if line.startswith("@RG\t"):
            f = dict(x.split(":", 1) for x in line.split("\t")[1:] if len(x) >= 3)
            out.append(f.get("ID", "").encode())
    return out


def rg_index(rb: bytes, ids: list[bytes]) -> int:
    v = DM.rg_value(rb)
    return ids.index(v) if v and v in ids else -1


# ------------------------------------------------------------------------------------------- one set
def close(a, b, D: int) -> bool:
    """a, b: (rg, tile, x, y) of two located pairs of one part"""
    return a[0] == b[0] and a[1] == b[1] and abs(a[2] - b[2]) <= D and abs(a[3] - b[3]) <= D


def components(members: list[tuple[int, int, int, int]], D: int) -> int:
    """connected components of "close" among located members, by union-find over all pairs of members"""
    n = len(members)
    if n < 2:
        return n
    a = np.array(members, dtype=np.int64)
    adj = ((a[:, None, 0] == a[None, :, 0]) & (a[:, None, 1] == a[None, :, 1]) & (np.abs(a[:, None, 2] - a[None, :, 2]) <= D) &
           (np.abs(a[:, None, 3] - a[None, :, 3]) <= D))
    par = list(range(n))

    def find(v):
        while par[v] != v:
            par[v] = par[par[v]]
            v = par[v]
        return v

    for i, j in zip(*np.nonzero(np.triu(adj, 1))):
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            par[ri] = rj
    return sum(1 for v in range(n) if find(v) == v)


def set_optical(members, divided: bool, D: int) -> tuple[int, int]:
    """members: [(first: bool, location (rg, tile, x, y) or None)] -> (located, optical duplicates).  A divided set
    (FR or RF) is counted in two parts, by `first`."""
    located = optical = 0
    for part in ((True, False) if divided else (None,)):
        locs = [loc for first, loc in members if loc is not None and (part is None or first == part)]
        located += len(locs)
        optical += len(locs) - components(locs, D)
    return located, optical


# ------------------------------------------------------------------------------------------- a record set
def pairs_and_sets(recs: np.ndarray, offs: np.ndarray, header_text: str):
    """-> [(read-1 record index, read-2 record index, set id)] from tests/dupcheck.py"""
    import torch

    import dupcheck
    if len(offs) == 0:
        return []
    dbg: dict = {}
    dupcheck.expected_dups(torch.from_numpy(np.ascontiguousarray(recs)), torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()),
                           header_text, dbg)
    if "pr1" not in dbg:
        return []
    return list(zip(dbg["pr1"].tolist(), dbg["pr2"].tolist(), dbg["pgid"].tolist()))


def compute(recs: np.ndarray, offs: np.ndarray, header_text: str, D: int, ignore_rg: bool = False):
    """-> (per library [pairs, sets, located, optical] by the library ids of dupmetrics_model.lib_table, the three
    histograms as lists of BINS).  `located` counts the pairs with a location in sets of two or more pairs."""
    rg_lib, unknown, names = DM.lib_table(header_text)
    ids = rg_ids(header_text)
    per_lib = [[0] * 4 for _ in names]
    hist = [[0] * BINS for _ in range(3)]
    sets: dict[int, list[tuple[int, int]]] = {}
    for r1, r2, g in pairs_and_sets(recs, offs, header_text):
        sets.setdefault(g, []).append((r1, r2))

    def rec(i):
        o = int(offs[i])
        return bytes(recs[o:o + 4 + struct.unpack_from("<I", recs, o)[0]])

    for members in sets.values():
        first = rec(members[0][0])
        lib = DM.library_of(first, rg_lib, unknown)
        s = len(members)
        located = o = 0
        if s >= 2:
            flag1, flag2 = struct.unpack_from("<H", first, 18)[0], struct.unpack_from("<H", rec(members[0][1]), 18)[0]
            divided = bool((flag1 ^ flag2) & 0x10)  # FR or RF: the two ends on different strands
            ms = []
            for r1, _ in members:
                rb = rec(r1)
                loc = location(read_name(rb))
                ms.append((bool(struct.unpack_from("<H", rb, 18)[0] & 0x40), None if loc is None else ((-1 if ignore_rg else rg_index(rb, ids)),) + loc))
            located, o = set_optical(ms, divided, D)
        per_lib[lib][0] += s
        per_lib[lib][1] += 1
        per_lib[lib][2] += located
        per_lib[lib][3] += o
        hist[0][min(s, BINS - 1)] += 1
        hist[2][min(s - o, BINS - 1)] += 1
        if o > 0:
            hist[1][min(o + 1, BINS - 1)] += 1
    return per_lib, hist


# ------------------------------------------------------------------------------------------- the text
def text(row_list, hist, command_line: str) -> bytes:
    """row_list: [(name, the six counters of dupmetrics_model, [pairs, sets, located, optical])].  Section 26's layout
    with the optical column filled; the estimate and the ROI from (READ_PAIRS_EXAMINED - optical, READ_PAIRS_EXAMINED -
    READ_PAIR_DUPLICATES); the histogram block always."""
    body = ("## htsjdk.samtools.metrics.StringHeader\n" + f"# {command_line}\n" + "\n" + "## METRICS CLASS\tpicard.sam.DuplicationMetrics\n" +
            "\t".join(DM.COLUMNS) + "\n").encode()
    ordered = sorted(row_list, key=lambda r: r[0].encode())
    last = None
    for nm, c6, c4 in ordered:
        d = DM.derived(c6)
        n, dups, opt = d["pairs"], d["pair_dups"], c4[3]
        size = DM.estimate_library_size(n - opt, n - dups) if opt <= n and dups <= n else None
        body += nm.encode() + ("\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%s\n" % (
            d["unpaired"], n, d["secondary"], d["unmapped"], d["unpaired_dups"], dups, opt, d["percent"], "" if size is None else str(size))).encode()
        last = (n - opt, n - dups, size)
    body += b"\n"
    roi = len(ordered) == 1 and bool(last[2])
    top = max([k for k in range(1, BINS) if hist[0][k] or hist[1][k] or hist[2][k]] or [0])
    if roi:
        top = max(top, 100)
    body += ("## HISTOGRAM\tjava.lang.Double\nBIN" + ("\tCoverageMult" if roi else "") + "\t" + "\t".join(HIST_COLUMNS) + "\n").encode()
    for k in range(1, top + 1):
        line = "%d.0" % k
        if roi:
            n, c, L = float(last[0]), float(last[1]), float(last[2])
            line += "\t%.6f" % (L * (1 - math.exp(-(float(k) * n) / L)) / c)
        body += (line + "\t%d\t%d\t%d\n" % (hist[0][k], hist[1][k], hist[2][k])).encode()
    return body + b"\n"


def text_of_records(recs, offs, header_text: str, D: int, command_line: str) -> bytes:
    """The whole file of a record set: section 26's counts of the records' flags, this model's sets."""
    rg_lib, unknown, names = DM.lib_table(header_text)
    counts = DM.count(DM.records_of_arena(recs, offs), rg_lib, unknown, len(names))
    per_lib, hist = compute(recs, offs, header_text, D)
    rows = [(nm, counts[k], per_lib[k]) for k, nm in enumerate(names) if nm]
    if not names[unknown] and (any(counts[unknown]) or any(per_lib[unknown])):
        rows.append((DM.UNKNOWN, counts[unknown], per_lib[unknown]))
    return text(rows, hist, command_line)
