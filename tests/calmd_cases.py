"""Crafted inputs for `openge calmd` (tests/calmd_model.py is the definition): the smallest shapes at which the
device code can go wrong.  Every case is (records, refs, reference dict), built with bamutil.make_record from
fixed seeds.

    rows()         name -> (record, declared MD, declared NM): directed reads whose tags are written down here from
                   the construction (reference slices and the positions that were mutated), not taken from the model
    cases()        name -> (records, refs, reference): the rows as one set, the record counts 0, 1, 63, 64, 65 and
                   1025 (scan and grid edges; one wave takes a record, a workgroup four), pass-through records, tag
                   states, the block_size limit
    error_cases()  name -> (records, refs, reference, code, lowest bad record)
"""
from __future__ import annotations

import random
import struct

import bamutil
import calmd_model as M

CL = 3000
_rnd = random.Random(2801)
R = "".join(_rnd.choice("ACGT") for _ in range(CL))  # chr1
# chr2 as the FASTA holds it: N, lowercase, IUPAC codes and two bytes that are no letters, then plain bases
R2_RAW = "ACGTNacgtRYKM*-" + "".join(_rnd.choice("ACGT") for _ in range(185))
RAW = {"chr1": R, "chr2": R2_RAW}                       # the FASTA's content; chrM is in the header only
REFERENCE = {k: M.upper(v.encode()) for k, v in RAW.items()}
REFS = [("chr1", CL), ("chr2", len(R2_RAW)), ("chrM", 100)]
R2 = REFERENCE["chr2"].decode()
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def write_fasta(path, raw: dict = RAW, width: int = 60) -> str:
    with open(path, "w") as f:
        for name, seq in raw.items():
            f.write(f">{name} crafted for calmd\n")
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + "\n")
    return str(path)


def header_text(refs=REFS) -> str:
    return "@HD\tVN:1.4\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)


def rd(pos: int, n: int, wrong=()) -> str:
    """n bases of chr1 from pos on, the ones at the relative positions `wrong` replaced by another base."""
    s = list(R[pos:pos + n])
    for i in wrong:
        s[i] = OTHER[s[i]]
    return "".join(s)


def rec(name, pos, cigar, seq, tags=b"", contig=0, flag=0) -> bytes:
    return bamutil.make_record(name, flag, contig, pos, cigar, seq, tags=tags)


def nm_tag(v: int, typ: str = "C") -> bytes:
    return b"NM" + typ.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ], v)


def md_tag(s: str) -> bytes:
    return b"MDZ" + s.encode() + b"\0"


def rows() -> dict:
    out = {}

    def row(name, pos, cigar, seq, md, nm, **kw):
        assert name not in out
        out[name] = (rec(name, pos, cigar, seq, **kw), md.encode(), nm)

    # ---- read lengths and chunk edges (a wave takes 64 bases of an M op at a time)
    row("len1", 10, "1M", rd(10, 1), "1", 0)
    row("len1_wrong", 10, "1M", rd(10, 1, [0]), f"0{R[10]}0", 1)
    for n in (63, 64, 65, 128, 129):
        row(f"len{n}", 200, f"{n}M", rd(200, n), str(n), 0)
        row(f"len{n}_last_wrong", 200, f"{n}M", rd(200, n, [n - 1]), f"{n - 1}{R[200 + n - 1]}0", 1)
    row("run_carried_over_chunk", 300, "100M", rd(300, 100, [70]), f"70{R[370]}29", 1)
    row("run_carried_over_ops", 300, "40M3I40M", rd(300, 40) + "GGG" + rd(340, 40, [30]), f"70{R[370]}9", 4)
    row("lanes_0_and_63", 400, "128M", rd(400, 128, [0, 63, 64, 127]), f"0{R[400]}62{R[463]}0{R[464]}62{R[527]}0", 4)
    row("wrong65", 500, "70M", rd(500, 70, range(65)), "".join(f"0{R[500 + i]}" for i in range(65)) + "5", 65)
    w = [9, 20, 120, 221]  # runs of 9, 10, 99, 100 and 1000 matches: every decimal width a read can reach
    row("run_widths", 600, "1222M", rd(600, 1222, w), f"9{R[609]}10{R[620]}99{R[720]}100{R[821]}1000", 4)
    # ---- CIGAR shapes
    row("d_first_of_chunk", 700, "64M2D10M", rd(700, 64) + rd(766, 10), f"64^{R[764:766]}10", 2)
    row("d_after_wrong", 700, "10M2D5M", rd(700, 10, [9]) + rd(712, 5), f"9{R[709]}0^{R[710:712]}5", 3)
    row("wrong_after_d", 700, "3M2D3M", rd(700, 3) + rd(705, 3, [0]), f"3^{R[703:705]}0{R[705]}2", 3)
    row("d_d", 800, "5M1D2D5M", rd(800, 5) + rd(808, 5), f"5^{R[805]}0^{R[806:808]}5", 3)
    row("i_d", 800, "5M2I1D5M", rd(800, 5) + "TT" + rd(806, 5), f"5^{R[805]}5", 3)
    row("ins_only", 800, "3M1I3M", rd(800, 3) + "A" + rd(803, 3), "6", 1)
    row("eq_x", 900, "5=1X4=", rd(900, 10, [5]), f"5{R[905]}4", 1)
    row("x_that_matches", 900, "5=1X4=", rd(900, 10), "10", 0)
    row("n_skip", 900, "5M100N5M", rd(900, 5) + rd(1005, 5), "10", 0)
    row("clips", 1000, "3H2S10M3S1H", "GG" + rd(1000, 10) + "TTT", "10", 0)
    row("clips_wrong_ends", 1000, "2S10M3S", "GG" + rd(1000, 10, [0, 9]) + "TTT", f"0{R[1000]}8{R[1009]}0", 2)
    row("pad", 1000, "5M2P5M", rd(1000, 10), "10", 0)
    row("ops70", 1100, "2M1I" * 35, "".join(rd(1100 + 2 * k, 2) + "C" for k in range(35)), "70", 35)
    row("ops130_wrong", 1100, "1M1I" * 65, "".join(rd(1100 + k, 1, [0] if k == 64 else []) + "C" for k in range(65)),
        f"64{R[1164]}0", 66)
    # ---- bases: = N and IUPAC in the read; N, lowercase, IUPAC and non-letters in the reference (chr2)
    assert R2[:15] == "ACGTNACGTRYKM*-"
    row("chr2_all_kinds", 0, "15M", "ACGTNACGTRYKMAA", "4N8*0-0", 3, contig=1)
    row("read_all_eq", 0, "15M", "=" * 15, "15", 0, contig=1)
    row("read_iupac_on_acgt", 0, "4M", "RCGT", "0A3", 1, contig=1)
    row("read_n_on_acgt", 0, "4M", "ANGT", "1C2", 1, contig=1)
    row("read_acgt_on_iupac", 9, "4M", "AYGM", "0R1K1", 2, contig=1)
    # ---- reference edges (chr1 has CL bases)
    row("off_end_in_m", CL - 5, "10M", rd(CL - 5, 5) + "AAAAA", "5", 0)
    row("off_end_in_m_wrong", CL - 5, "10M", rd(CL - 5, 5, [2]) + "AAAAA", f"2{R[CL - 3]}2", 1)
    row("off_end_then_ins", CL - 5, "10M2I3M", rd(CL - 5, 5) + "A" * 10, "5", 0)
    row("ins_then_off_end", CL - 5, "2M2I8M", rd(CL - 5, 2) + "GG" + rd(CL - 3, 3) + "AAAAA", "5", 2)
    row("off_end_in_d", CL - 10, "5M10D5M", rd(CL - 10, 5) + "AAAAA", f"5^{R[CL - 5:]}0", 10)
    row("d_past_end_then_ins", CL - 10, "5M10D2I", rd(CL - 10, 5) + "AA", f"5^{R[CL - 5:]}0", 12)
    row("starts_past_end", CL + 7, "5M", "ACGTA", "0", 0)
    # ---- NM values at the edges of the appended tag's types
    row("nm255", 1300, "5M255I5M", rd(1300, 5) + "A" * 255 + rd(1305, 5), "10", 255)
    row("nm256", 1300, "5M256I5M", rd(1300, 5) + "A" * 256 + rd(1305, 5), "10", 256)
    row("nm65535", CL - 10, "5M65535D", rd(CL - 10, 5), f"5^{R[CL - 5:]}0", 65535)
    row("nm65536", CL - 10, "5M65536D", rd(CL - 10, 5), f"5^{R[CL - 5:]}0", 65536)
    return out


# ---- tag states: one read, nm = 1, MD = 4x5
T_POS = 1500
T_SEQ = rd(T_POS, 10, [4])
T_MD = f"4{R[T_POS + 4]}5"
B_ARRAY = b"XBBs" + struct.pack("<I", 3) + struct.pack("<3h", -1, 2, 3)
F_TAG = b"XFf" + struct.pack("<f", 1.5)
RG = b"RGZrg1\0"


def tag_states() -> dict:
    """name -> (record, nm changed, md changed)"""
    t = {}
    for typ in "cCsSiI":
        t[f"nm_equal_{typ}"] = (RG + nm_tag(1, typ) + md_tag(T_MD), False, False)
    t["nm_different"] = (nm_tag(7) + RG + md_tag(T_MD), True, False)
    t["nm_negative"] = (nm_tag(-1, "c") + md_tag(T_MD), True, False)
    t["nm_as_z"] = (b"NMZ1\0" + md_tag(T_MD), True, False)
    t["nm_as_b"] = (b"NMBC" + struct.pack("<I", 1) + b"\1" + md_tag(T_MD), True, False)
    t["md_different"] = (nm_tag(1) + md_tag("10") + RG, False, True)
    t["md_prefix"] = (nm_tag(1) + md_tag(T_MD[:-1]), False, True)
    t["md_longer"] = (nm_tag(1) + md_tag(T_MD + "0"), False, True)
    t["md_as_a"] = (nm_tag(1) + b"MDAx", False, True)
    t["b_and_f_before_nm"] = (B_ARRAY + F_TAG + nm_tag(3) + md_tag("9"), True, True)
    t["nm_last"] = (RG + md_tag(T_MD) + nm_tag(2), True, False)
    t["md_before_nm"] = (md_tag("3A6") + RG + nm_tag(0, "i"), True, True)
    t["md_after_nm_both_wrong"] = (nm_tag(9, "S") + RG + md_tag("1"), True, True)
    t["second_nm_ignored"] = (nm_tag(1) + nm_tag(5) + md_tag(T_MD) + md_tag("1"), False, False)
    t["no_tags"] = (b"", True, True)
    t["other_tags_only"] = (RG + B_ARRAY + b"UQi" + struct.pack("<i", 30), True, True)
    return {k: (rec(k, T_POS, "10M", T_SEQ, tags=v[0]), v[1], v[2]) for k, v in t.items()}


def pass_through() -> dict:
    """name -> (record, the counter it is counted in)"""
    tags = nm_tag(9) + md_tag("1")
    return {
        "unmapped_flag": (rec("u", 100, "10M", rd(100, 10), tags, flag=4), "skipped"),
        "no_refid": (rec("r", 100, "10M", rd(100, 10), tags, contig=-1), "skipped"),
        "no_pos": (rec("p", -1, "10M", rd(100, 10), tags), "skipped"),
        "no_cigar": (rec("c", 100, "", rd(100, 10), tags), "skipped"),
        "no_seq": (rec("s", 100, "10M", "", tags), "skipped"),
        "contig_not_in_fasta": (rec("m", 5, "10M", "ACGTACGTAC", tags, contig=2), "no_reference"),
    }


def limit_record(over: int) -> bytes:
    """A read whose block_size is 10000 + over after the update (NM:C and MD:Z are appended)."""
    md = "10"
    base = rec("limit", 1600, "10M", rd(1600, 10))
    fill = M.MAX_BLOCK_SIZE + over - (len(base) - 4) - 4 - (3 + len(md) + 1) - 4  # the filler's own XZZ and NUL
    return rec("limit", 1600, "10M", rd(1600, 10), tags=b"XZZ" + b"a" * fill + b"\0")


def generated(n: int, seed: int) -> list:
    """n reads of chr1 with random shapes, mismatches (= and N among them) and tag states; a sixth of them carry
    the tags the model gives them, so they stay as they are."""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        n_ops = rnd.choice((1, 1, 2, 3, 5))
        ops, seq, x = [], [], rnd.randrange(0, CL - 700)
        pos = x
        if rnd.random() < 0.2:
            k = rnd.randrange(1, 6)
            ops.append(f"{k}S")
            seq.append("".join(rnd.choice("ACGT") for _ in range(k)))
        for j in range(n_ops):
            k = rnd.choice((1, 7, 30, 63, 64, 65, 100, 129))
            s = list(R[x:x + k])
            for q in range(k):
                if rnd.random() < 0.04:
                    s[q] = rnd.choice("ACGTN=")
            ops.append(f"{k}{rnd.choice('MMM=X')}")
            seq.append("".join(s))
            x += k
            if j + 1 < n_ops:
                kind, g = rnd.choice("IDNP"), rnd.randrange(1, 12)
                ops.append(f"{g}{kind}")
                if kind == "I":
                    seq.append("".join(rnd.choice("ACGT") for _ in range(g)))
                elif kind in "DN":
                    x += g
        seq = "".join(seq)
        nm, md = M.walk(pos, [(bamutil.CIG[c[-1]], int(c[:-1])) for c in ops], _codes(seq), REFERENCE["chr1"])
        state = rnd.randrange(6)
        tags = (b"", RG, nm_tag(nm, "i") + md_tag(md.decode()), RG + md_tag(md.decode()) + nm_tag((nm + 1) & 0x7F),
                nm_tag(nm & 0xFF, "C") + RG + md_tag("1"), B_ARRAY + nm_tag(0, "S"))[state]
        out.append(rec(f"g{i}", pos, "".join(ops), seq, tags=tags))
    return out


def _codes(seq: str) -> list:
    return [M.ALPHABET.index(ch.encode()) for ch in seq]


def cases() -> dict:
    c = {}
    c["rows"] = ([r for r, _, _ in rows().values()], REFS, REFERENCE)
    c["tag_states"] = ([r for r, _, _ in tag_states().values()], REFS, REFERENCE)
    c["pass_through"] = ([r for r, _ in pass_through().values()] + [rec("used", T_POS, "10M", T_SEQ)], REFS, REFERENCE)
    c["limit_exact"] = ([rec("a", T_POS, "10M", T_SEQ), limit_record(0)], REFS, REFERENCE)
    for n in (0, 1, 63, 64, 65, 1025):
        c[f"n{n}"] = (generated(n, 7000 + n), REFS, REFERENCE)
    return c


def _patch(rb: bytes, at: int, fmt: str, v) -> bytes:
    b = bytearray(rb)
    struct.pack_into(fmt, b, at, v)
    return bytes(b)


def bad_records() -> dict:
    """name -> a used record with one fault (its length is that of the well-formed record it was made from)"""
    good = rec("bad", T_POS, "10M", T_SEQ, tags=RG)
    cig_at = 36 + len("bad") + 1
    return {
        "refid_past_n_ref": _patch(good, 4, "<i", len(REFS)),
        # a wrong MD of 66,000 bytes: without it the record would fit again
        "block_size_above_10000": rec("bad", T_POS, "10M", T_SEQ, tags=md_tag("1" * 66000)),
        "op_code_9": _patch(good, cig_at, "<I", 10 << 4 | 9),
        "cigar_past_block": _patch(good, 16, "<H", 3000),
        "seq_past_block": _patch(_patch(good, 20, "<I", 5000), cig_at, "<I", 5000 << 4),
        "tag_without_nul": rec("bad", T_POS, "10M", T_SEQ, tags=b"RGZrg1"),
        "tag_cut": rec("bad", T_POS, "10M", T_SEQ, tags=RG + b"XY"),
        "tag_value_cut": rec("bad", T_POS, "10M", T_SEQ, tags=RG + b"XYi\0\0"),
        "tag_unknown_type": rec("bad", T_POS, "10M", T_SEQ, tags=b"XY?\0" + RG),
        "b_array_past_block": rec("bad", T_POS, "10M", T_SEQ, tags=b"XBBi" + struct.pack("<I", 100) + b"\0" * 8),
        "b_array_unknown_subtype": rec("bad", T_POS, "10M", T_SEQ, tags=b"XBBq" + struct.pack("<I", 1) + b"\0"),
        "query_length": _patch(good, cig_at, "<I", 9 << 4),
    }


def error_cases() -> dict:
    """Every fault as the lowest of two bad records (the other one of another kind), between good ones; the record
    that is one byte over the limit; a limit record behind an argument fault and in front of one."""
    bad = bad_records()
    names = list(bad)
    good = [rec(f"ok{i}", T_POS + i, "10M", rd(T_POS + i, 10)) for i in range(3)]
    skip = pass_through()["unmapped_flag"][0]
    out = {}
    for k, name in enumerate(names):
        other = bad[names[(k + 1) % len(names)]]
        out[name] = ([good[0], skip, bad[name], good[1], other, good[2]], REFS, REFERENCE, M.ERR_ARG, 2)
    out["limit_one_over"] = ([good[0], limit_record(1), good[1]], REFS, REFERENCE, M.ERR_LIMIT, 1)
    out["limit_before_arg"] = ([limit_record(1), bad["op_code_9"]], REFS, REFERENCE, M.ERR_LIMIT, 0)
    out["arg_before_limit"] = ([good[0], bad["query_length"], limit_record(1)], REFS, REFERENCE, M.ERR_ARG, 1)
    # 70 records so that the faults sit in different workgroups and waves
    out["fault_in_a_later_wave"] = (good * 22 + [bad["tag_cut"]] + good + [bad["op_code_9"]], REFS, REFERENCE, M.ERR_ARG, 66)
    return out
