"""Crafted SAM texts for the SAM input tests (the CPU model test, the host program and the GPU tests share them): the
smallest shapes at which the kernels of csrc/sam_parse.hip can go wrong.  A case is a whole SAM text (header and
lines); an error case adds the 1-based line of the file that must be named and the model's field."""
from __future__ import annotations

import functools

# csrc/sam_parse.hip: a wave takes WAVE_LINES consecutive lines, a workgroup BLOCK_LINES (tests/test_gpu_samin.py
# checks both against the library's counters); a lane chunk is 64 characters, a line-index tile 4096 bytes
WAVE_LINES, BLOCK_LINES = 4, 16
REFS = [("c", 1 << 29), ("chr2", 1 << 29), ("L" * 200, 1 << 29)]
SEQ = "ACGTNMRSVWYHKDB="


def header(refs=REFS, extra: str = "") -> bytes:
    return ("@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs) + extra).encode()


def seq_of(n: int, k: int = 0) -> str:
    return "".join(SEQ[(i * 5 + k) % 15] for i in range(n))  # no '=': the reference's writer and reader both know it, keep it rare


def qual_of(n: int, k: int = 0) -> str:
    return "".join(chr(33 + (i * 7 + k) % 94) for i in range(n))


def line(name="r", flag=0, rname="c", pos=100, mapq=60, cigar="*", rnext="*", pnext=0, tlen=0, seq=None, qual=None, tags=()) -> bytes:
    if seq is None:
        seq = seq_of(8)
    if qual is None:
        qual = qual_of(len(seq)) if seq != "*" else "*"
    f = [name, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual, *tags]
    return "\t".join(f).encode()


def basic(i: int) -> bytes:
    n = 30 + i % 9
    return line(f"read{i}", flag=0x41 if i % 2 else 0x10, rname=REFS[i % 2][0], pos=1000 + 17 * i, mapq=i % 61, cigar=f"{n}M",
                rnext="=" if i % 2 else "*", pnext=1200 + i, tlen=(200 + i) * (-1 if i % 4 == 1 else 1), seq=seq_of(n, i), qual=qual_of(n, i),
                tags=(f"NM:i:{i % 200}", f"RG:Z:grp{i % 3}"))


def text(lines: list[bytes], refs=REFS, newline_at_end=True) -> bytes:
    return header(refs) + b"\n".join(lines) + (b"\n" if lines and newline_at_end else b"")


def padded(total: int, k: int = 0) -> bytes:
    """A line of exactly `total` characters: the slack goes into a Z tag."""
    base = line(f"p{total}", pos=7 + k, cigar="8M", tags=("NM:i:1",))
    assert total >= len(base) + 6
    return base + b"\tXZ:Z:" + b"z" * (total - len(base) - 6)


def straddle_lines() -> list[bytes]:
    """A tab at the characters 62..65 and 126..129 of the line, and fields that straddle the chunk edges."""
    out = []
    for at in (62, 63, 64, 65, 126, 127, 128, 129):
        # the name ends right before the tab at `at`
        out.append(line("n" * at, flag=99, rname="chr2", pos=123456, cigar="4M4S", rnext="=", pnext=99, tlen=-50, tags=("AS:i:-7",)))
        assert out[-1][at:at + 1] == b"\t"
    for at in (60, 61, 62, 63):  # FLAG, POS and the CIGAR across the edge
        out.append(line("m" * at, flag=65535, rname="c", pos=2147483647, mapq=255, cigar="1M2I3D4N5S6H7P8=9X", seq=seq_of(25), tags=("XA:A:q",)))
    return out


def cigar_of(nops: int) -> tuple[str, int]:
    ops = "MIDNSHP=X"
    s = "".join(f"{1 + (i * 37) % 1200}{ops[i % 9]}" for i in range(nops))
    return s, 0


INT_EDGES = (0, 255, 256, -1, -128, -129, 65535, 65536, -32768, -32769, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, -(1 << 31), 127, 128, 32767, 32768)


@functools.lru_cache(maxsize=None)
def cases() -> dict[str, bytes]:
    c: dict[str, bytes] = {}
    c["header_only"] = header()
    c["empty_text"] = b""
    c["no_header"] = b"\n".join([line("a", rname="*"), line("b", rname="*", rnext="*")]) + b"\n"
    for n in (1, WAVE_LINES - 1, WAVE_LINES, WAVE_LINES + 1, BLOCK_LINES - 1, BLOCK_LINES, BLOCK_LINES + 1, 3 * BLOCK_LINES + 5):
        c[f"basic_{n}"] = text([basic(i) for i in range(n)])
    c["no_trailing_newline"] = text([basic(i) for i in range(6)], newline_at_end=False)
    c["one_line_no_newline"] = text([basic(3)], newline_at_end=False)
    c["line_lengths"] = text([padded(n) for n in (63, 64, 65, 127, 128, 129, 255, 256, 257)] + [padded(10300), padded(4096), padded(70)])
    c["tile_edges"] = text([padded(4096 - len(header()) % 4096 + d, d) for d in (-1, 0, 1, 2, 3)] + [padded(4095), padded(4097), padded(8191)])
    c["straddle"] = text(straddle_lines())
    c["names"] = text([line("x"), line("y" * 254), line("q" * 253), line("ab")])
    c["seq_lengths"] = text([line(f"s{n}", seq=seq_of(n, n) if n else "*", qual=qual_of(n) if n else "*") for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 500, 501)])
    c["seq_cases"] = text([line("low", seq="acgtnmrsvwyhkdb=", qual=qual_of(16)), line("odd", seq="XZ.U*", qual="IIIII"),
                           line("qstar", seq="ACGTA", qual="*"), line("both", seq="*", qual="*"), line("q1", seq="A", qual="*"),
                           line("qmax", seq="ACG", qual="!~J")])
    widths = [0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999,
              1000000000, 2147483647, 2147483648]
    c["pos_widths"] = text([line(f"p{p}", flag=1, pos=p, rnext="=", pnext=p, cigar="5M", seq=seq_of(5)) for p in widths] +
                           [line("neg", pos=-5, pnext=-2147483647), line("zeros", pos="000123", tlen="-0007", mapq="007", flag="0099")])
    c["tlen_widths"] = text([line(f"t{t}", flag=3, rname="chr2", rnext="chr2", pnext=5, tlen=t) for t in
                             [0, 9, -9, 10, -10, 99, -100, 1234, -12345, 123456, -1234567, 12345678, -123456789, 1234567890, 2147483647, -2147483648]])
    c["bins"] = text([line(f"b{p}_{ln}", pos=p, cigar=f"{ln}M" if ln else "*") for p, ln in
                      [(0, 0), (0, 5), (1, 1), (16384, 1), (16384, 2), (16385, 16384), (131072, 1), (131073, 200000), (1 << 20, 1 << 20), (1 << 23, 1 << 23),
                       (1 << 26, 1 << 26), (1 << 29, 1), ((1 << 29) - 10, 20), (2147483647, 268435455)]] +
                     [line("mixed", pos=16380, cigar="3M2X1=1N1P1H5S4I2D")])
    c["cigars"] = text([line(f"c{n}", cigar=cigar_of(n)[0] if n else "*", pos=1000) for n in (0, 1, 2, 63, 64, 65, 99, 100, 120, 128, 129, 300)] +
                       [line("long", cigar="268435455M"), line("zeros", cigar="0M00012S")])
    c["int_tags"] = text([line(f"i{k}", tags=(f"X{chr(65 + k % 26)}:i:{v}",)) for k, v in enumerate(INT_EDGES)] +
                         [line("many", tags=tuple(f"Y{chr(65 + k)}:i:{v}" for k, v in enumerate(INT_EDGES))), line("z", tags=("ZZ:i:-0", "ZY:i:0000255", "ZX:i:0000256"))])
    c["str_tags"] = text([line("a", tags=("XA:A:!", "XB:A:~", "XC:A: ")), line("z", tags=("RG:Z:grp 1 with spaces", "CO:Z:", "XE:Z:x")),
                          line("h", tags=("XH:H:1AE301", "XI:H:")), line("zl", tags=("XL:Z:" + "w" * 700, "NM:i:3", "XM:Z:" + "v" * 63, "XN:Z:" + "u" * 64)),
                          line("colon", tags=("XZ:Z:a:b:c\\t", "X1:Z:::"))])
    c["host_tags"] = text([line("f1", tags=("XF:f:1.5",)), basic(1), line("f2", tags=("NM:i:1", "XF:f:-3.25e-3", "RG:Z:g")),
                           line("b1", tags=("XB:B:c,1,-2,127,-128",)), line("b2", tags=("XB:B:C,0,255", "XS:B:s,-32768,32767", "XT:B:S,65535")),
                           line("b3", tags=("XI:B:i,-2147483648,2147483647", "XJ:B:I,4294967295,0", "XK:B:f,1.5,-0.25,1e10")),
                           line("b0", tags=("XE:B:c", "XZ:Z:after")), basic(2), line("bl", tags=("XL:B:S," + ",".join(str(i) for i in range(200)),)), basic(4)])
    c["rnext"] = text([line("eq", flag=1, rname="chr2", rnext="=", pnext=10), line("star", flag=1, rname="chr2", rnext="*", pnext=77),
                       line("other", flag=1, rname="c", rnext="L" * 200, pnext=5), line("unk", flag=1, rname="c", rnext="nowhere", pnext=9),
                       line("unmapped_eq", rname="*", pos=0, rnext="=", pnext=0), line("last", rname="L" * 200, rnext="c"), line("unk2", rnext="C")])
    c["one_contig"] = text([line("a", rname="only", rnext="="), line("b", rname="*")], refs=[("only", 1000)])
    many = [(f"ctg{i}_{(i * 7919) % 1000}", 1000 + i) for i in range(3000)]
    c["many_contigs"] = text([line(f"m{i}", flag=1, rname=many[i][0], rnext=many[(i * 31 + 7) % 3000][0], pnext=3) for i in (0, 1, 2, 1499, 2998, 2999)] +
                             [line("u", flag=1, rname=many[5][0], rnext="ctg5")], refs=many)
    c["cr"] = text([line("a", tags=("XZ:Z:x\r",)), line("b", seq="ACGT", qual="III\r")])
    mix = []
    for i in range(150):
        k = i % 10
        mix.append(basic(i) if k < 6 else padded(64 + i, i) if k == 6 else line(f"f{i}", tags=("XF:f:0.5",)) if k == 7 else
                   line(f"c{i}", cigar=cigar_of(1 + i % 70)[0]) if k == 8 else line(f"s{i}", seq=seq_of(100 + i), tags=(f"XI:i:{-i * 1000}",)))
    c["mix"] = text(mix)
    return c


# what the reference's reader defines (util/sam_reader.cpp): no f, B or H tag, no `*` SEQ / QUAL, no lowercase or
# unknown base, fewer than 100 CIGAR ops, lines below 10,240 characters, integers inside int32 and every error-free
# line at least 10 characters, and a newline behind the last line (it cuts the last character of a line that has none)
REFERENCE_DEFINED = ["basic_1", "basic_3", "basic_4", "basic_5", "basic_15", "basic_16", "basic_17", "basic_53", "straddle", "names", "tlen_widths", "rnext", "one_contig", "many_contigs"]


def reference_subset() -> dict[str, bytes]:
    """Cases, or the part of a case, that the reference defines (tests/golden/make_samin_goldens.py)."""
    c = cases()
    out = {k: c[k] for k in REFERENCE_DEFINED}
    out["line_lengths"] = text([padded(n) for n in (63, 64, 65, 127, 128, 129, 255, 256, 257, 4096, 10200)])  # its fgets buffer ends a line near 10,239
    out["seq_lengths"] = text([line(f"s{n}", seq=seq_of(n, n), qual=qual_of(n)) for n in (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 500, 501)])
    out["pos_widths"] = text([line(f"p{p}", flag=1, pos=p, rnext="=", pnext=p, cigar="5M", seq=seq_of(5)) for p in
                              [0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000,
                               999999999, 1000000000, 2147483647]])
    out["bins"] = text([line(f"b{p}_{ln}", pos=p, cigar=f"{ln}M" if ln else "*") for p, ln in
                        [(0, 0), (0, 5), (1, 1), (16384, 1), (16384, 2), (16385, 16384), (131072, 1), (131073, 200000), (1 << 20, 1 << 20), (1 << 23, 1 << 23),
                         (1 << 26, 1 << 26), (1 << 29, 1), ((1 << 29) - 10, 20)]] + [line("mixed", pos=16380, cigar="3M2X1=1N1P1H5S4I2D")])
    out["cigars"] = text([line(f"c{n}", cigar=cigar_of(n)[0] if n else "*", pos=1000) for n in (0, 1, 2, 63, 64, 65, 99)])
    out["int_tags"] = text([line(f"i{k}", tags=(f"X{chr(65 + k % 26)}:i:{v}",)) for k, v in enumerate(INT_EDGES) if -(1 << 31) <= v < 1 << 31])
    out["str_tags"] = text([line("a", tags=("XA:A:!", "XB:A:~", "XC:A: ")), line("z", tags=("RG:Z:grp 1 with spaces", "CO:Z:", "XE:Z:x")),
                            line("zl", tags=("XL:Z:" + "w" * 700, "NM:i:3", "XM:Z:" + "v" * 63, "XN:Z:" + "u" * 64))])
    return out


@functools.lru_cache(maxsize=None)
def error_cases() -> dict[str, tuple[bytes, int, str]]:
    """name -> (text, the 1-based line of the file that fails, the model's field), each error as the first, a middle
    and the last line of a body longer than a workgroup's lines."""
    bad = {
        "fields10": (b"\t".join(line("x").split(b"\t")[:10]), "fields"),
        "short": (b"a\tb\tc\td", "short"),
        "empty_line": (b"", "short"),
        "flag_text": (line("x", flag="1x"), "FLAG"),
        "flag_range": (line("x", flag=65536), "FLAG"),
        "flag_neg": (line("x", flag=-1), "FLAG"),
        "flag_empty": (line("x", flag=""), "FLAG"),
        "flag_plus": (line("x", flag="+4"), "FLAG"),
        "mapq_range": (line("x", mapq=256), "MAPQ"),
        "pos_range": (line("x", pos=2147483649), "POS"),
        "pos_low": (line("x", pos=-2147483648), "POS"),
        "pos_huge": (line("x", pos="9" * 30), "POS"),
        "pos_minus": (line("x", pos="-"), "POS"),
        "pnext_range": (line("x", pnext=2147483649), "PNEXT"),
        "tlen_range": (line("x", tlen=2147483648), "TLEN"),
        "tlen_text": (line("x", tlen="1e3"), "TLEN"),
        "name255": (line("n" * 255), "QNAME"),
        "qual_len": (line("x", seq="ACGT", qual="III"), "QUAL"),
        "qual_len_star_seq": (line("x", seq="*", qual="II"), "QUAL"),
        "tag_shape": (line("x", tags=("NM:i:1", "XYZ:i:1")), "tag"),
        "tag_short": (line("x", tags=("NM:i",)), "tag"),
        "tag_empty": (line("x", tags=("",)), "tag"),
        "tag_a_long": (line("x", tags=("XA:A:ab",)), "tag"),
        "tag_type": (line("x", tags=("XQ:q:1",)), "tag type"),
        "tag_type_c": (line("x", tags=("XQ:c:1",)), "tag type"),
        "tag_int_range": (line("x", tags=("XI:i:4294967296",)), "tag integer"),
        "tag_int_low": (line("x", tags=("XI:i:-2147483649",)), "tag integer"),
        "tag_int_text": (line("x", tags=("XI:i:12a",)), "tag integer"),
        "tag_b_sub": (line("x", tags=("XB:B:q,1",)), "tag"),
        "cigar_letter": (line("x", cigar="5M3Q"), "CIGAR"),
        "cigar_no_len": (line("x", cigar="M"), "CIGAR"),
        "cigar_tail": (line("x", cigar="5M3"), "CIGAR"),
        "cigar_big": (line("x", cigar="268435456M"), "CIGAR"),
        "cigar_empty": (line("x", cigar=""), "CIGAR"),
        "cigar_ops": (line("x", cigar="1M1I" * 32768), "CIGAR ops"),
        "rname_unknown": (line("x", rname="nowhere"), "RNAME"),
    }
    out = {}
    n = BLOCK_LINES + 3
    hl = header().count(b"\n")
    for name, (ln, field) in bad.items():
        for where, at in (("first", 0), ("middle", n // 2), ("last", n - 1)):  # the last line has no newline behind it
            lines = [basic(i) for i in range(n)]
            lines[at] = ln
            # (an empty last line exists only with its newline: without one it is the trailing newline of the line before)
            out[f"{name}_{where}"] = (text(lines, newline_at_end=where != "last" or not ln), hl + at + 1, field)
    # two bad lines: the lower one is named
    lines = [basic(i) for i in range(n)]
    lines[n - 2] = bad["flag_text"][0]
    lines[5] = bad["mapq_range"][0]
    out["two_bad"] = (text(lines), hl + 6, "MAPQ")
    return out
