"""Python restatement of the duplication metrics (csrc/dupmetrics.hip, host_capi.cpp; DESIGN.md section 26;
include/openge_hip.h states the same definition).  The yardstick of the tests: nothing here calls the library.

A record contributes its final FLAG and the library its RG tag resolves to; the counters are sums of reads, so the
counts of any partition of a record set add up."""
from __future__ import annotations

import math
import struct

COUNTERS = ("unpaired_examined", "pair_reads_examined", "secondary", "unmapped", "unpaired_dups", "pair_read_dups")
UNKNOWN = "Unknown Library"
COLUMNS = ("LIBRARY", "UNPAIRED_READS_EXAMINED", "READ_PAIRS_EXAMINED", "SECONDARY_OR_SUPPLEMENTARY_RDS", "UNMAPPED_READS",
           "UNPAIRED_READ_DUPLICATES", "READ_PAIR_DUPLICATES", "READ_PAIR_OPTICAL_DUPLICATES", "PERCENT_DUPLICATION",
           "ESTIMATED_LIBRARY_SIZE")
MIN_BLOCK, MAX_BLOCK = 32, 10000  # the block sizes the record walks admit; any other record has no tags to walk


# ------------------------------------------------------------------------------------------- one record
def rg_value(rb: bytes) -> bytes | None:
    """The RG value as FindTag finds it: the first tag named RG, of whatever type byte, gives the bytes up to the
    next NUL or the record's end; None when the walk ends without one."""
    (bs,) = struct.unpack_from("<I", rb, 0)
    if bs < MIN_BLOCK or bs > MAX_BLOCK:
        return None
    tend = 4 + bs
    lname, ncig, lseq = rb[12], struct.unpack_from("<H", rb, 16)[0], struct.unpack_from("<I", rb, 20)[0]
    p = 36 + lname + 4 * ncig + (lseq + 1) // 2 + lseq
    while p + 3 <= tend:
        t0, t1, ty = rb[p], rb[p + 1], rb[p + 2]
        p += 3
        if t0 == 0x52 and t1 == 0x47:  # "RG"
            s = p
            while s < tend and rb[s]:
                s += 1
            return bytes(rb[p:s])
        if ty == 0:
            return None
        c = chr(ty)
        if c in "AcC":
            p += 1
        elif c in "sS":
            p += 2
        elif c in "fiI":
            p += 4
        elif c in "ZH":
            while p < tend and rb[p]:
                p += 1
            p += 1
        elif c == "B":
            if p + 5 > tend:
                return None
            sub, (cnt,) = chr(rb[p]), struct.unpack_from("<i", rb, p + 1)
            p += 5
            size = 1 if sub in "cC" else 2 if sub in "sS" else 4 if sub in "fiI" else 0
            if not size or cnt < 0:
                return None
            p += cnt * size
        else:
            return None
        if p >= tend or rb[p] == 0:
            return None
    return None


def library_of(rb: bytes, rg_lib: dict[bytes, int], unknown_lib: int) -> int:
    """rg_lib: read-group id -> library id.  No tag, an empty value or an unlisted value: unknown_lib."""
    v = rg_value(rb)
    return rg_lib.get(v, unknown_lib) if v else unknown_lib


def record_class(flag: int, refid: int) -> str:
    """The first rule that applies (buildSortedReadEndLists, algorithms/mark_duplicates.cpp:202-209)."""
    if flag & 0x4 or refid == -1:
        return "unmapped"
    if flag & 0x100:
        return "secondary"
    if flag & 0x1 and not flag & 0x8:
        return "pair"
    return "unpaired"


def record_counters(flag: int, refid: int) -> list[str]:
    """The one or two counters a record adds 1 to."""
    cls = record_class(flag, refid)
    out = [{"unmapped": "unmapped", "secondary": "secondary", "pair": "pair_reads_examined", "unpaired": "unpaired_examined"}[cls]]
    if flag & 0x400 and cls in ("pair", "unpaired"):
        out.append("pair_read_dups" if cls == "pair" else "unpaired_dups")
    return out


# ------------------------------------------------------------------------------------------- the table
def lib_table(header_text: str) -> tuple[dict[bytes, int], int, list[str]]:
    """(read-group id -> library id, unknown_lib, names by id) as LibTable (csrc/lib_table.h) numbers them: ids
    from 1 in the order the names first appear; an @RG without an LB, or with an empty one, is in "Unknown Library";
    unknown_lib is that name's id when an @RG has it, else the next free id, whose name here is ""."""
    ids: dict[str, int] = {}
    rg_lib: dict[bytes, int] = {}
    for line in header_text.splitlines():
        if not line.startswith("@RG\t"):
            continue
        f = dict(x.split(":", 1) for x in line.split("\t")[1:] if len(x) >= 3)
        lb = f.get("LB", "") or UNKNOWN
        ids.setdefault(lb, len(ids) + 1)
        rg_lib.setdefault(f.get("ID", "").encode(), ids[lb])  # the first read group of an id wins, as the table walk does
    unknown = ids.get(UNKNOWN, len(ids) + 1)
    names = [""] * (max(list(ids.values()) + [unknown]) + 1)
    for nm, k in ids.items():
        names[k] = nm
    return rg_lib, unknown, names


def count(records, rg_lib: dict[bytes, int], unknown_lib: int, n_lib: int | None = None) -> list[list[int]]:
    """records: an iterable of record bytes -> n_lib rows of the six counters, indexed by library id"""
    if n_lib is None:
        n_lib = 1 + max(list(rg_lib.values()) + [unknown_lib])
    out = [[0] * 6 for _ in range(n_lib)]
    for rb in records:
        flag, refid = struct.unpack_from("<H", rb, 18)[0], struct.unpack_from("<i", rb, 4)[0]
        lib = library_of(rb, rg_lib, unknown_lib)
        for c in record_counters(flag, refid):
            out[lib][COUNTERS.index(c)] += 1
    return out


def records_of_arena(recs, offs):
    for o in offs:
        o = int(o)
        (bs,) = struct.unpack_from("<I", recs, o)
        yield bytes(recs[o:o + 4 + bs])


def rows(names: list[str], unknown_lib: int, counts: list[list[int]]) -> list[tuple[str, list[int]]]:
    """One row for every library an @RG names; one more "Unknown Library" row when none does and at least one
    record resolved to it.  In id order (text() sorts)."""
    out = [(nm, counts[k]) for k, nm in enumerate(names) if nm]
    if not names[unknown_lib] and any(counts[unknown_lib]):
        out.append((UNKNOWN, counts[unknown_lib]))
    return out


# ------------------------------------------------------------------------------------------- derived values
def estimate_library_size(pairs: int, unique_pairs: int) -> int | None:
    """Picard's estimateLibrarySize, in double, in exactly this order of operations; None: no estimate."""
    n, c = float(pairs), float(unique_pairs)
    if not (pairs > 0 and pairs - unique_pairs > 0):
        return None

    def f(x: float) -> float:
        if x == 0:  # c == 0: 0 / 0 in IEEE arithmetic; every comparison with it is false, the result is 0
            return math.nan
        return c / x - 1 + math.exp(-n / x)

    m, M = 1.0, 100.0
    while f(M * c) > 0:
        M *= 10
    for _ in range(40):
        r = (m + M) / 2
        u = f(r * c)
        if u == 0:
            break
        if u > 0:
            m = r
        else:
            M = r
    return int(c * (m + M) / 2)


def f_at(pairs: int, unique_pairs: int, x: float) -> float:
    return float(unique_pairs) / x - 1 + math.exp(-float(pairs) / x)


def derived(c6: list[int]) -> dict:
    ue, pe, sec, unm, ud, pd = c6
    n, dups = pe // 2, pd // 2
    den = ue + pe
    size = estimate_library_size(n, n - dups) if dups <= n else None
    return dict(unpaired=ue, pairs=n, secondary=sec, unmapped=unm, unpaired_dups=ud, pair_dups=dups, optical=0,
                percent=(ud + pd) / den if den else 0.0, size=size)


def roi(pairs: int, unique_pairs: int, size: int) -> list[float]:
    L, n, c = float(size), float(pairs), float(unique_pairs)
    return [L * (1 - math.exp(-(x * n) / L)) / c for x in (float(k) for k in range(1, 101))]


# ------------------------------------------------------------------------------------------- the text
def text(row_list: list[tuple[str, list[int]]], command_line: str) -> bytes:
    """Picard's layout; rows sorted by name in byte order; the histogram only with exactly one row that has an
    estimate."""
    out = ["## htsjdk.samtools.metrics.StringHeader\n", f"# {command_line}\n", "\n", "## METRICS CLASS\tpicard.sam.DuplicationMetrics\n",
           "\t".join(COLUMNS) + "\n"]
    ordered = sorted(row_list, key=lambda r: r[0].encode())
    ds = [derived(c6) for _, c6 in ordered]
    body = b"".join(s.encode() for s in out)
    for (nm, _), d in zip(ordered, ds):
        body += nm.encode() + ("\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%s\n" % (
            d["unpaired"], d["pairs"], d["secondary"], d["unmapped"], d["unpaired_dups"], d["pair_dups"], d["optical"], d["percent"],
            "" if d["size"] is None else str(d["size"]))).encode()
    body += b"\n"
    if len(ds) == 1 and ds[0]["size"]:  # an estimate of 0 (no unique pair) has no histogram
        d = ds[0]
        body += b"## HISTOGRAM\tjava.lang.Double\nBIN\tVALUE\n"
        for k, v in enumerate(roi(d["pairs"], d["pairs"] - d["pair_dups"], d["size"]), 1):
            body += ("%d.0\t%.6f\n" % (k, v)).encode()
        body += b"\n"
    return body


def parse(data: bytes) -> tuple[str, list[dict], list[tuple[float, float]]]:
    """A metrics file -> (command line, rows as {column: text}, histogram).  What a report tool does: the line
    after "## METRICS CLASS" names the columns."""
    lines = data.decode().split("\n")
    assert lines[0] == "## htsjdk.samtools.metrics.StringHeader" and lines[1].startswith("# ") and lines[2] == ""
    assert lines[3] == "## METRICS CLASS\tpicard.sam.DuplicationMetrics"
    cols = lines[4].split("\t")
    k, out = 5, []
    while lines[k] != "":
        out.append(dict(zip(cols, lines[k].split("\t"))))
        assert len(lines[k].split("\t")) == len(cols)
        k += 1
    k += 1
    hist = []
    if k < len(lines) and lines[k].startswith("## HISTOGRAM"):
        assert lines[k] == "## HISTOGRAM\tjava.lang.Double" and lines[k + 1] == "BIN\tVALUE"
        k += 2
        while lines[k] != "":
            a, b = lines[k].split("\t")
            hist.append((float(a), float(b)))
            k += 1
        k += 1
    assert lines[k:] == [""], lines[k:]
    return lines[1][2:], out, hist


def same_rows(got: list[dict], want: list[dict]) -> bool:
    """Integers exactly, PERCENT_DUPLICATION at 1e-6 absolute: one unit of the last printed digit."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        for col in COLUMNS:
            if col == "PERCENT_DUPLICATION":
                if abs(float(g[col]) - float(w[col])) > 1e-6:
                    return False
            elif g[col] != w[col]:
                return False
    return True
