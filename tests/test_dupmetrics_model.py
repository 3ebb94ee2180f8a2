"""CPU: the duplication-metrics model (tests/dupmetrics_model.py) against hand-worked values, and the crafted cases
(tests/dupmetrics_cases.py) against what they say they build."""
import struct

import bamutil
import dupmetrics_cases as K
import dupmetrics_model as M


def test_class_table_over_every_flag_combination():
    """All 128 combinations of {0x1, 0x4, 0x8, 0x10, 0x100, 0x400, 0x800} x refID {-1, 0}: the first rule that
    applies wins; 0x10 and 0x800 change nothing; 0x400 adds a duplicate count only to pair and unpaired."""
    seen = set()
    for refid in (-1, 0):
        for m in range(128):
            flag = sum(b for k, b in enumerate(K.FLAG_BITS) if m >> k & 1)
            cls = M.record_class(flag, refid)
            if flag & 0x4 or refid == -1:
                want = "unmapped"
            elif flag & 0x100:
                want = "secondary"
            elif (flag & 0x9) == 0x1:
                want = "pair"
            else:
                want = "unpaired"
            assert cls == want, (hex(flag), refid)
            assert M.record_class(flag ^ 0x10, refid) == cls and M.record_class(flag ^ 0x800, refid) == cls
            got = M.record_counters(flag, refid)
            first = {"unmapped": "unmapped", "secondary": "secondary", "pair": "pair_reads_examined", "unpaired": "unpaired_examined"}[cls]
            dup = [] if not flag & 0x400 or cls in ("unmapped", "secondary") else ["pair_read_dups" if cls == "pair" else "unpaired_dups"]
            assert got == [first] + dup, (hex(flag), refid, got)
            seen.add((cls, bool(dup)))
    assert len(seen) == 6  # four classes, two of them with and without the duplicate count


def test_halving_of_odd_pair_counts():
    d = M.derived([3, 7, 0, 0, 1, 3])
    assert (d["pairs"], d["pair_dups"]) == (3, 1)
    assert d["percent"] == (1 + 3) / (3 + 7)  # the reads, not the halved pairs
    assert M.derived([0, 0, 5, 5, 0, 0])["percent"] == 0.0 and M.derived([0, 1, 0, 0, 0, 1])["size"] is None


def test_rg_value_hand_cases():
    r = lambda tags: K.rec(0, 0, tags)
    assert M.rg_value(r(b"")) is None
    assert M.rg_value(r(K.rg(b"g1"))) == b"g1"
    assert M.rg_value(r(K.SCALARS + K.ARRAYS + K.rg(b"g2"))) == b"g2"
    assert M.rg_value(r(K.rg(b"g1", b"\0"))) == b"g1"  # RG is looked at before the type byte
    assert M.rg_value(r(K.rg(b""))) == b"" and M.rg_value(r(b"RGZ")) == b"" and M.rg_value(r(b"RG")) is None
    assert M.rg_value(r(b"XX?abcd" + K.rg(b"g1"))) is None and M.rg_value(r(b"XX\0" + K.rg(b"g1"))) is None
    assert M.rg_value(r(K.rg(b"abc", nul=False))) == b"abc"
    assert M.rg_value(r(b"XZZabc\0\0\0\0" + K.rg(b"g1"))) is None
    assert M.rg_value(r(b"YBBc" + struct.pack("<i", -8) + K.rg(b"g1"))) is None
    assert M.rg_value(r(b"YBBc" + struct.pack("<i", 2) + b"ab" + K.rg(b"g2"))) == b"g2"
    assert M.rg_value(r(K.rg(b"g2") + K.rg(b"g1"))) == b"g2"
    assert M.rg_value(r(b"XZZRGZg1\0" + K.rg(b"g2"))) == b"g2"


def test_lib_table_numbers_as_the_modules_do():
    rg_lib, unknown, names = M.lib_table(K.rg_shapes()[0])
    assert names[1:5] == ["libA", "Unknown Library", "lib15", "lib16"] and unknown == 2
    assert rg_lib[b"g1"] == 1 and rg_lib[b"g2"] == 1 and rg_lib[b"g3"] == 2 and rg_lib[b"g4"] == 2  # the first g1 counts
    assert names[names.index("libDouble")] == "libDouble" and b"g1" in rg_lib and rg_lib[b"g1"] != names.index("libDouble")
    rg_lib, unknown, names = M.lib_table(K.header_text([("a", "x"), ("b", "y")]))
    assert (unknown, names) == (3, ["", "x", "y", ""])
    assert M.lib_table(K.header_text([])) == ({}, 1, ["", ""])


def test_rows_and_unknown_library():
    names = ["", "x", "y", ""]
    zero = [0] * 6
    assert M.rows(names, 3, [zero, zero, [1, 0, 0, 0, 0, 0], zero]) == [("x", zero), ("y", [1, 0, 0, 0, 0, 0])]
    assert M.rows(names, 3, [zero, zero, zero, [0, 0, 0, 2, 0, 0]])[-1] == ("Unknown Library", [0, 0, 0, 2, 0, 0])
    assert M.rows(["", ""], 1, [zero, zero]) == []


def test_cases_build_what_they_say():
    cases = K.cases()
    for n in (0, 1, 63, 64, 65, K.TILE - 1, K.TILE, K.TILE + 1, 2 * K.TILE + 1):
        header, records = cases[f"n{n}"]
        assert len(records) == n
        rg_lib, unknown, names = M.lib_table(header)
        c = M.count(records, rg_lib, unknown)
        for at, nm in ((63, "lib_w_last"), (64, "lib_w_first"), (K.TILE - 1, "lib_t_last"), (K.TILE, "lib_t_first"),
                       (2 * K.TILE - 1, "lib_t2_last"), (2 * K.TILE, "lib_t2_first")):
            assert sum(c[names.index(nm)][:4]) == (1 if at < n else 0), (n, nm)  # the only record of its library
    header, records = cases["flag_table"]
    assert len(records) == 256 and len({(bamutil.fields(r)["flag"], bamutil.fields(r)["refid"]) for r in records}) == 256
    c = M.count(records, *M.lib_table(header)[:2])
    assert all(all(v > 0 for v in row) for row in c[1:4])  # every counter of every library is hit
    header, records = cases["contention"]
    assert M.count(records, *M.lib_table(header)[:2])[1] == [0, 3 * K.TILE, 0, 0, 0, 3 * K.TILE]
    for n_lib in (1, 2, K.LDS_LIBS - 2, K.LDS_LIBS - 1, K.LDS_LIBS, K.LDS_LIBS + 1):
        header, records = cases[f"libs{n_lib}"]
        rg_lib, unknown, names = M.lib_table(header)
        assert len(names) == n_lib + 2 and unknown == n_lib + 1
        c = M.count(records, rg_lib, unknown)
        assert all(sum(row[:4]) > 0 for row in c[1:])  # every library, the unknown one too
    # the table sizes on both sides of the LDS limit are among them
    assert {len(M.lib_table(cases[f"libs{k}"][0])[2]) for k in (K.LDS_LIBS - 2, K.LDS_LIBS - 1)} == {K.LDS_LIBS, K.LDS_LIBS + 1}
    header, records = cases["rg_shapes"]
    rg_lib, unknown, names = M.lib_table(header)
    c = M.count(records, rg_lib, unknown)
    for nm in ("libA", "Unknown Library", "lib15", "lib16", "lib40", "libShort", "libLong"):
        assert sum(c[names.index(nm)][:4]) > 0, nm
    assert sum(c[names.index("libDouble")]) == 0


def test_text_layout_and_parse_round_trip():
    one = [("libA", [10, 2000, 3, 4, 1, 200])]
    t = M.text(one, "openge dedup --metrics m.txt in.bam")
    cl, rows, hist = M.parse(t)
    assert cl == "openge dedup --metrics m.txt in.bam" and len(rows) == 1 and len(hist) == 100
    d = M.derived(one[0][1])
    assert rows[0]["LIBRARY"] == "libA" and rows[0]["READ_PAIRS_EXAMINED"] == "1000" and rows[0]["READ_PAIR_DUPLICATES"] == "100"
    assert rows[0]["ESTIMATED_LIBRARY_SIZE"] == str(d["size"]) and d["size"] > 900
    assert rows[0]["PERCENT_DUPLICATION"] == "%.6f" % (201 / 2010)
    # ROI at 1x is 1 but for the estimate's cut to an integer: L moves by less than 1, L (1 - exp(-n / L)) / c by less than 1 / c
    assert [h[0] for h in hist] == [float(k) for k in range(1, 101)] and abs(hist[0][1] - 1.0) < 1 / 900
    assert all(a[1] <= b[1] for a, b in zip(hist, hist[1:])) and hist[0][1] < hist[1][1] < hist[99][1]  # it saturates at L / c
    two = M.text(one + [("Zeta", [0] * 6)], "x")
    assert b"HISTOGRAM" not in two and [r["ESTIMATED_LIBRARY_SIZE"] for r in M.parse(two)[1]] == ["", str(d["size"])]  # "Z" < "l"
    assert b"HISTOGRAM" not in M.text([("libA", [5, 0, 0, 0, 1, 0])], "x")  # no pairs: no estimate
    # byte order, not locale order: upper case before lower case, "_" between them
    order = [r["LIBRARY"] for r in M.parse(M.text([(n, [0] * 6) for n in ("b", "B", "a", "_", "Z", "é")], "x"))[1]]
    assert order == ["B", "Z", "_", "a", "b", "é"]
    assert M.same_rows(rows, rows) and not M.same_rows(rows, [dict(rows[0], UNMAPPED_READS="5")])
