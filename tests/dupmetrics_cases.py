"""Crafted record sets for the duplication metrics (csrc/dupmetrics.hip): the smallest shapes at which its kernel can go
wrong.  Every case is (header text, records).  Geometry the shapes aim at: 64 lanes per wave, 256 threads per
workgroup, TILE records per tile (counter dupmetrics_tile_records), LDS_LIBS libraries in the workgroup's LDS table
(counter dupmetrics_lds_libs; one library more takes the kernel that adds its per-wave sums to the table in HBM)."""
from __future__ import annotations

import struct

import bamutil

REFS = [("chrA", 100000), ("chrB", 50000)]
TILE, LDS_LIBS = 1024, 64
FLAG_BITS = (0x1, 0x4, 0x8, 0x10, 0x100, 0x400, 0x800)
# every class with and without 0x400, and bits without a meaning of their own
FLAG_CYCLE = (0x0, 0x400, 0x1, 0x401, 0x9, 0x409, 0x4, 0x404, 0x100, 0x500, 0x800, 0xC01, 0x10, 0x411, 0x63, 0x463)


def header_text(rgs, refs=REFS) -> str:
    """rgs: [(id, LB or None)]"""
    return ("@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs) +
            "".join(f"@RG\tID:{i}" + (f"\tLB:{lb}" if lb is not None else "") + "\tSM:s\n" for i, lb in rgs))


def rg(value: bytes, type_byte: bytes = b"Z", nul: bool = True) -> bytes:
    return b"RG" + type_byte + value + (b"\0" if nul else b"")


def rec(i: int, flag: int = 0, tags: bytes = b"", refid: int = 0) -> bytes:
    mapped_mate = bool(flag & 0x1) and not flag & 0x8
    return bamutil.make_record(f"r{i}", flag, refid, -1 if refid < 0 else 100 + i % 9000, "" if refid < 0 else "4M", "ACGT", None, 30,
                               refid if mapped_mate else -1, (100 + i % 9000) if mapped_mate and refid >= 0 else -1, 0, tags)


# one tag of every scalar type and of every B subtype, with array counts 0, 1 and 3
SCALARS = (b"XAAq" + b"Xcc\xff" + b"XCC\x07" + b"Xss" + struct.pack("<h", -2) + b"XSS" + struct.pack("<H", 9) + b"Xii" + struct.pack("<i", -5) +
           b"XII" + struct.pack("<I", 77) + b"Xff" + struct.pack("<f", 1.5) + b"XZZtext\0" + b"XHH1AE3\0")
ARRAYS = b"".join(b"Y" + t + b"B" + t + struct.pack("<i", cnt) + bytes(size * cnt)
                  for (t, size), cnt in zip(((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4)), (3, 0, 1, 3, 0, 1, 3)))


def sized_cases() -> dict:
    """n = 0, 1, 63, 64, 65, T - 1, T, T + 1 and 2 T + 1 records: the last record of a wave and of a tile and the first
    of the next are the only records of their library; the rest are of one more."""
    edge = {63: "w_last", 64: "w_first", TILE - 1: "t_last", TILE: "t_first", 2 * TILE - 1: "t2_last", 2 * TILE: "t2_first"}
    rgs = [("bulk", "libBulk")] + [(nm, "lib_" + nm) for nm in edge.values()]
    out = {}
    for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out[f"n{n}"] = (header_text(rgs), [rec(i, FLAG_CYCLE[i % len(FLAG_CYCLE)], rg(edge.get(i, "bulk").encode())) for i in range(n)])
    return out


def flag_table() -> tuple[str, list[bytes]]:
    """all 128 combinations of FLAG_BITS x refID {-1, 0}: 256 records over three libraries"""
    rgs = [("a", "libA"), ("b", "libB"), ("c", "libC")]
    records = []
    for refid in (-1, 0):
        for m in range(128):
            flag = sum(b for k, b in enumerate(FLAG_BITS) if m >> k & 1)
            records.append(rec(len(records), flag, rg(rgs[(m + (refid + 1) * 2) % 3][0].encode()), refid))
    return header_text(rgs), records


def contention() -> tuple[str, list[bytes]]:
    """3 T records of one library and one class: every lane of every wave adds to one key, and with 0x400 to two"""
    return header_text([("only", "libOnly")]), [rec(i, 0x401, rg(b"only")) for i in range(3 * TILE)]


ID15, ID16, ID40 = "f" * 15, "s" * 16, "l" * 40


def rg_shapes() -> tuple[str, list[bytes]]:
    rgs = [("g1", "libA"), ("g2", "libA"),            # two read groups with one LB
           ("g3", None),                               # no LB: Unknown Library
           ("g4", "Unknown Library"),                  # an LB spelled like it: the same library
           (ID15, "lib15"), (ID16, "lib16"), (ID40, "lib40"),
           ("g1", "libDouble"),                        # a second @RG of one id: the first one counts
           ("g", "libShort"), ("g12", "libLong")]      # ids that are prefixes of one another
    shapes = [
        b"",                                            # no tags
        rg(b"g1"),                                      # RG first
        SCALARS + ARRAYS + rg(b"g2"),                   # RG after one tag of every type
        ARRAYS + SCALARS + rg(b"g3"),
        rg(b"g1", b"A"), rg(b"g2", b"i"), rg(b"g4", b"B"), rg(b"g1", b"\0"), rg(b"g2", b"?"),   # a type byte other than Z
        rg(b""),                                        # an empty value
        rg(b"nobody"), rg(b"g1x"), rg(b"G1"),           # unlisted values
        rg(ID15.encode()), rg(ID16.encode()), rg(ID40.encode()),
        rg(ID15.encode()[:-1]), rg(ID16.encode() + b"s"), rg(ID40.encode()[:-1] + b"L"),   # one byte off at every length
        rg(b"g"), rg(b"g12"),
        rg(b"g3"), rg(b"g4"),
        b"XX?" + b"abcd" + rg(b"g1"),                   # an unknown type byte in front of RG: the walk ends
        b"XX\0" + rg(b"g1"),                            # a type byte of 0 in front
        b"XZZabc\0" + b"\0\0\0" + rg(b"g1"),            # the next tag starts with a NUL
        rg(b"g1", nul=False), rg(ID15.encode(), nul=False), rg(ID16.encode(), nul=False),   # the value ends at the record's end
        b"XZZopen",                                     # a Z value that runs to the record's end, no RG
        b"YBBc" + struct.pack("<i", 1000) + b"ab",      # a B array that runs past the record's end
        b"YBBc" + struct.pack("<i", -8) + rg(b"g1"),    # a negative count
        b"YBBZ" + struct.pack("<i", 1) + b"a" + rg(b"g1"),   # an unknown subtype
        b"YBB" + b"c\1\0",                              # a B header that does not fit
        b"YBBc" + struct.pack("<i", 2) + b"ab" + rg(b"g2"),  # an array that ends where RG begins
        rg(b"g2") + rg(b"g1"),                          # two RG tags: the first one
        b"XZZRGZg1\0" + rg(b"g2"),                      # "RGZg1" inside a string value is no tag
        b"RG",                                          # two bytes: no tag
        b"RGZ",                                         # a tag without a value byte: empty
    ]
    records = []
    for k, tags in enumerate(shapes):
        for flag in (0x0, 0x401, 0x104, 0x409):
            records.append(rec(len(records), flag, tags, -1 if flag == 0x104 and k % 2 else 0))
    return header_text(rgs), records


def lib_count_cases() -> dict:
    """1, 2, LDS_LIBS and LDS_LIBS + 1 libraries named by the header, every one hit; with the id for "Unknown Library"
    the table has two entries more"""
    out = {}
    for n_lib in (1, 2, LDS_LIBS - 2, LDS_LIBS - 1, LDS_LIBS, LDS_LIBS + 1):
        rgs = [(f"rg{k}", f"lib{k:03d}") for k in range(n_lib)]
        records = [rec(i, FLAG_CYCLE[(i // n_lib) % len(FLAG_CYCLE)], rg(f"rg{i % n_lib}".encode()) if i % (n_lib + 1) else b"")
                   for i in range(3 * n_lib + 70)]
        out[f"libs{n_lib}"] = (header_text(rgs), records)
    return out


def cases() -> dict:
    out = dict(sized_cases())
    out["flag_table"] = flag_table()
    out["contention"] = contention()
    out["rg_shapes"] = rg_shapes()
    out["no_rg_lines"] = (header_text([]), [rec(i, FLAG_CYCLE[i % 16], rg(b"g1") if i % 2 else b"") for i in range(40)])
    out.update(lib_count_cases())
    return out


def bam_body(header: str, refs, records) -> bytes:
    ht = header.encode()
    body = b"BAM\1" + struct.pack("<i", len(ht)) + ht + struct.pack("<i", len(refs))
    for name, ln in refs:
        nb = name.encode() + b"\0"
        body += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    return body + b"".join(records)
