"""Crafted local-realignment cases: the read shapes, caps and edges the seeded generator never emits.

Every case is a function of a fixed seed.  build_case(name, dir) writes ref.fa / ref.fa.fai (60/61 line
geometry), targets.intervals and reads.bam and returns a Built with the paths and the case's declared routing:
the number of work intervals (intervals with at least one read to clean) and how many of them phase B on the
device hands back to the host, by the rules in the header of realign_prep.hip (a read of more than 8 cigar
operations, a left-aligned cigar of more than 4, more than 2048 consensus candidates in the interval).

Conventions: 3 kb contigs, 60-base reads, quality 30; every read at a site is first of a proper pair whose
mate lies 400 bp away outside every interval; MAPQ 60, RG:Z:rg1; records coordinate-sorted (stable: reads at
one position keep their creation order, which is then the interval's toClean order).
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from pathlib import Path

import bamutil

CL = 3000
RL = 60
TAGS = b"RGZrg1\0"
REGULAR = set("ACGTacgt*")


@dataclass
class Built:
    name: str
    fasta: str
    intervals: str
    bam: str
    work: int                 # work intervals
    host: int                 # ... of which the device hands back to the host
    golden: bool = True       # a reference golden exists (tests/golden/rl_craft/<name>.json)
    host_pairs: int = -1      # mixed: scan pairs of the host intervals (kept consensuses x altReads)
    host_intervals: list = field(default_factory=list)  # mixed: the interval lines of the host intervals


class Case:
    def __init__(self, seed: int, n_contigs: int = 1):
        self.rnd = random.Random(seed)
        self.refs = ["".join(self.rnd.choice("ACGT") for _ in range(CL)) for _ in range(n_contigs)]
        self.recs: list[tuple[int, int, bytes]] = []
        self.ivs: list[str] = []
        self.n = 0

    def name_of(self, c: int) -> str:
        return f"chr{c + 1}"

    def set_ref(self, c: int, at: int, s: str) -> None:
        self.refs[c] = self.refs[c][:at] + s + self.refs[c][at + len(s):]
        assert len(self.refs[c]) == CL

    def interval(self, c: int, site: int) -> str:
        """The 51-base interval around a site (1-based, clamped to the contig)."""
        ln = f"{self.name_of(c)}:{max(site - 24, 1)}-{min(site + 26, CL)}\n"
        self.ivs.append(ln)
        return ln

    def add(self, tag: str, c: int, pos: int, cigar: str, seq: str, fx: int = 0, qual=None) -> None:
        """A first-of-pair read and its 60M mate 400 bp away (towards the contig's middle)."""
        name = f"{tag}{self.n}"
        self.n += 1
        ref = self.refs[c]
        far = pos + 400 if pos + 400 + RL <= CL else pos - 400
        tlen = far + RL - pos if far > pos else -(pos + RL - far)
        f1 = 0x1 | 0x2 | 0x40 | (0x20 if far > pos else 0x10) | fx
        f2 = 0x1 | 0x2 | 0x80 | (0x10 if far > pos else 0x20) | fx
        self.recs.append((c, pos, bamutil.make_record(name, f1, c, pos, cigar, seq, qual, 60, c, far, tlen, TAGS)))
        self.recs.append((c, far, bamutil.make_record(name, f2, c, far, f"{RL}M", ref[far:far + RL].upper().replace("N", "A"),
                                                      None, 60, c, pos, -tlen, TAGS)))

    # sample haplotypes: n bases from reference position t on, with a deletion of L at p / an insertion at p
    def hap_del(self, c: int, t: int, p: int, L: int, n: int = RL) -> str:
        ref = self.refs[c] + "A" * 200
        s = ref[t:p] + ref[p + L:] if t < p else ref[t + L:]
        return s[:n].upper()

    def hap_ins(self, c: int, t: int, p: int, ins: str, n: int = RL) -> str:
        ref = self.refs[c] + "A" * 200
        assert t <= p
        return (ref[t:p] + ins + ref[p:])[:n].upper()

    def mismatches(self, c: int, pos: int, bases: str) -> int:
        """Mismatches of the unclipped bases laid on the reference at pos, cigar ignored (regular bases only)."""
        ref = self.refs[c].upper()
        return sum(1 for i, b in enumerate(bases)
                   if pos + i < CL and b in REGULAR and ref[pos + i] in REGULAR and b != ref[pos + i])

    def write(self, d) -> tuple[str, str, str]:
        d = Path(d)
        d.mkdir(parents=True, exist_ok=True)
        fa, iv, bam = d / "ref.fa", d / "targets.intervals", d / "reads.bam"
        with open(fa, "w") as f, open(str(fa) + ".fai", "w") as fi:
            off = 0
            for c, ref in enumerate(self.refs):
                hdr = f">{self.name_of(c)}\n"
                f.write(hdr)
                off += len(hdr)
                fi.write(f"{self.name_of(c)}\t{CL}\t{off}\t60\t61\n")
                for i in range(0, CL, 60):
                    f.write(ref[i:i + 60] + "\n")
                off += CL + CL // 60
        iv.write_text("".join(self.ivs))
        hdr = "@HD\tVN:1.4\tSO:coordinate\n" + "".join(f"@SQ\tSN:{self.name_of(c)}\tLN:{CL}\n" for c in range(len(self.refs)))
        hdr += "@RG\tID:rg1\tLB:lib1\tSM:s\tPL:illumina\n"
        recs = sorted(self.recs, key=lambda r: (r[0], r[1]))  # stable
        bamutil.write_bam_py(bam, hdr, [(self.name_of(c), CL) for c in range(len(self.refs))], [r[2] for r in recs])
        return str(fa), str(iv), str(bam)


def _site_reads(k: Case, c: int, p: int, L: int, starts, shapes: str = "gu", ins: str | None = None, tag: str = "") -> None:
    """Plain support for a site: gapped ('g') and ungapped ('u') reads of the haplotype, by turns."""
    for i, t in enumerate(starts):
        a = p - t
        sh = shapes[i % len(shapes)]
        if ins is None:
            s = k.hap_del(c, t, p, L)
            k.add(tag + sh, c, t, f"{a}M{L}D{RL - a}M" if sh == "g" else f"{RL}M", s)
        else:
            s = k.hap_ins(c, t, p, ins)
            b = RL - a - len(ins)
            k.add(tag + sh, c, t, f"{a}M{len(ins)}I{b}M" if sh == "g" and b > 0 else f"{RL}M", s)


NINE_OPS = "2S{a8}M1I2M1D3M3D{b5}M5S"   # one more than the device takes
EIGHT_OPS = "{a6}M1I2M1D3M3D{b5}M5S"    # the most it takes


def _nine_op_read(k: Case, c: int, p: int, t: int) -> None:
    a = p - t
    b = RL - a
    cig = NINE_OPS.format(a8=a - 8, b5=b - 5)
    assert sum(ch.isalpha() for ch in cig) == 9
    k.add("nine", c, t + 2, cig, k.hap_del(c, t, p, 3))


def _five_op_read(k: Case, c: int, t: int) -> None:
    """4S20M1I1D1I33M: two blocks, two insertions around a deletion; its unclipped cigar has 5 operations and
    differs from the record's, so the left-aligned cigar is a new one of more than 4."""
    ref = k.refs[c]
    seq = "ACGT" + ref[t:t + 20] + "G" + "T" + ref[t + 21:t + 21 + 33]
    seq = seq[:50] + ("A" if seq[50] != "A" else "C") + seq[51:]
    assert len(seq) == 59
    k.add("two", c, t, "4S20M1I1D1I33M", seq)


def clips(seed=101):
    k = Case(seed)
    p, L = 1000, 3
    k.interval(0, p)
    for i, t in enumerate(range(p - 50, p - 8, 3)):
        a, b = p - t, RL - (p - t)
        s = k.hap_del(0, t, p, L)
        sh = i % 8
        if sh == 0: k.add("g", 0, t, f"{a}M{L}D{b}M", s)
        elif sh == 1: k.add("u", 0, t, f"{RL}M", s)
        elif sh == 2: k.add("tc", 0, t, f"{a}M{L}D{b - 5}M5S", s)
        elif sh == 3: k.add("hc", 0, t, f"3H{a}M{L}D{b}M2H", s)
        elif sh == 4: k.add("lc", 0, t + 4, f"4S{a - 4}M{L}D{b}M", s)
        elif sh == 5: k.add("dup", 0, t, f"{a}M{L}D{b}M", s, 0x400)
        elif sh == 6: k.add("bc", 0, t + 4, f"4S{a - 4}M{L}D{b - 5}M5S", s)
        else: k.add("alt", 0, t, f"{a + 3}M{L}D{b - 3}M", s)
    a = 30  # a read of 8 operations: not two blocks, no consensus, but still the device's
    k.add("eight", 0, p - a, EIGHT_OPS.format(a6=a - 6, b5=RL - a - 5), k.hap_del(0, p - a, p, L))
    return k, 1, 0


def early_indel(seed=102):
    k = Case(seed)
    p, q, L, ins = 1000, 2000, 3, "GT"
    k.interval(0, p)
    k.interval(0, q)
    _site_reads(k, 0, p, L, range(p - 48, p - 10, 4))
    k.add("early", 0, p - 2, f"2M{L}D{RL - 2}M", k.hap_del(0, p - 2, p, L))
    k.add("late", 0, p - 56, f"56M{L}D4M", k.hap_del(0, p - 56, p, L))
    _site_reads(k, 0, q, 0, range(q - 48, q - 10, 4), ins=ins)
    k.add("early", 0, q - 1, "1M2I57M", k.hap_ins(0, q - 1, q, ins))
    k.add("late", 0, q - 54, "54M2I4M", k.hap_ins(0, q - 54, q, ins))
    return k, 2, 0


def homopolymer(seed=103):
    k = Case(seed)
    # deletions of 2 at the right end of a 14-base run (990..1003); reads from inside the run: the deletion
    # slides to the read's first base
    k.set_ref(0, 989, "C" + "A" * 14 + "G")
    k.interval(0, 1000)
    p = 1002
    for t in (988, 989, 991, 992, 993, 994, 996):
        s = k.hap_del(0, t, p, 2)
        k.add("h", 0, t, f"{p - t}M2D{RL - (p - t)}M", s[:40] + ("A" if s[40] != "A" else "C") + s[41:])
    for t in (950, 955, 960):
        k.add("w", 0, t, f"{p - t}M2D{RL - (p - t)}M", k.hap_del(0, t, p, 2))
        k.add("v", 0, t + 1, f"{RL}M", k.hap_del(0, t + 1, p, 2))
    # insertions of 2 at the right end of a run (1990..2003)
    k.set_ref(0, 1989, "C" + "T" * 14 + "G")
    k.interval(0, 2000)
    q = 2004
    for t in (1988, 1989, 1992, 1994, 1997):
        s = k.hap_ins(0, t, q, "TT")
        k.add("hi", 0, t, f"{q - t}M2I{RL - 2 - (q - t)}M", s[:45] + ("A" if s[45] != "A" else "C") + s[46:])
    for t in (1950, 1955, 1960):
        k.add("wi", 0, t, f"{q - t}M2I{RL - 2 - (q - t)}M", k.hap_ins(0, t, q, "TT"))
        k.add("vi", 0, t + 1, f"{RL}M", k.hap_ins(0, t + 1, q, "TT"))
    return k, 2, 0


def _contig_edge(seed, p, starts=None):
    k = Case(seed, 2)
    k.interval(0, p)
    k.interval(1, p)
    starts = starts or [t for t in range(max(p - RL + 8, 0), p - 6, 3)]
    _site_reads(k, 0, p, 3, starts)
    _site_reads(k, 1, p, 0, starts, ins="".join(k.rnd.choice("ACGT") for _ in range(4)))
    return k, 2, 0


def contig_start(seed=104):
    return _contig_edge(seed, 35)


def contig_end(seed=105):
    # most reads end inside the contig (so the site is realigned); the last four, gapped and ungapped by turns,
    # run past the contig end (each base out there costs 99 on either alignment)
    p = CL - 20
    k, w, h = _contig_edge(seed, p, list(range(p - 58, p - 42)) + [p - 41, p - 34, p - 30, p - 18])
    assert sum(pos + RL > CL for _, pos, _ in k.recs) >= 3
    return k, w, h


def irregular_insert(seed=106):
    k = Case(seed)
    p = 1000
    # lower-case and N reference bases inside the window (946..1056)
    k.set_ref(0, 960, k.refs[0][960:972].lower())
    k.set_ref(0, 1030, "NN")
    k.set_ref(0, 1040, k.refs[0][1040:1046].lower())
    k.interval(0, p)
    for i, t in enumerate(range(960, 990, 4)):
        a = p - t
        k.add("r", 0, t, f"{a}M4I{RL - a - 4}M", k.hap_ins(0, t, p, "GRTA"))
        k.add("c", 0, t + 1, f"{a - 1}M4I{RL - a - 3}M", k.hap_ins(0, t + 1, p, "GCTA"))
        if i % 3 == 0:
            k.add("n", 0, t + 2, f"{a - 2}M4I{RL - a - 2}M", k.hap_ins(0, t + 2, p, "GNTA"))
        if i % 3 == 1:
            k.add("u", 0, t + 2, f"{RL}M", k.hap_ins(0, t + 2, p, "GCTA"))
    k.add("star", 0, 975, "60M", "", qual=b"")
    return k, 1, 0


def late_kept(seed=107):
    """134 reads to clean; only numbers 70 and 129 (from 0, in file order) have two blocks: the kept consensuses
    first appear in the second and the third 64-read chunk.  The sample carries an 8-base insertion at 985:
    read 129 has it, read 70 a 2-base deletion nobody else supports, the others are ungapped.  The last four
    start inside the insertion, mapped 5 bases left of it: on the insertion's consensus their best offset lies
    8 past their original one, so it is found only under that consensus's own maxStart."""
    k = Case(seed)
    q, ins = 985, "".join(k.rnd.choice("ACGT") for _ in range(8))
    k.interval(0, 1000)
    for i in range(130):
        t = 945 + i // 4  # 945..977, four reads a position
        if i == 70:
            k.add("g", 0, t, f"{1004 - t}M2D{RL - (1004 - t)}M", k.hap_del(0, t, 1004, 2))
        elif i == 129:
            k.add("g", 0, t, f"{q - t}M8I{RL - 8 - (q - t)}M", k.hap_ins(0, t, q, ins))
        else:
            k.add("u", 0, t, f"{RL}M", k.hap_ins(0, t, q, ins))
    for i in range(4):
        k.add("in", 0, q - 5, f"{RL}M", (ins[3:] + k.refs[0][q:q + RL])[:RL])
    assert k.mismatches(0, q - 5, ins[3:]) > 0
    return k, 1, 0


def many_consensuses(seed=108):
    """72 distinct consensuses (deletions of 1..8 at sites 988..1002 that give different strings), each created
    twice; every first copy lies left of every second copy, so a second copy's duplicate search has 72 distinct
    consensuses before it and finds its match beyond the first 64."""
    k = Case(seed)
    k.interval(0, 1000)
    seen, combos = set(), []
    for site in range(988, 1003):
        for L in range(1, 9):
            s = k.hap_del(0, 940, site, L, 140)
            if s not in seen:
                seen.add(s)
                combos.append((site, L))
    assert len(combos) >= 72, len(combos)
    combos = combos[:72]
    for rep in range(2):
        for d, (site, L) in enumerate(combos):
            t = 950 + 4 * rep + d % 4
            s = k.hap_del(0, t, site, L)
            assert k.mismatches(0, t, s) > 0
            k.add(f"c{rep}_", 0, t, f"{site - t}M{L}D{RL - (site - t)}M", s)
    # (the second copy of the first consensus comes after all 72 first copies)
    return k, 1, 0


def _cap(seed, n_cand):
    k = Case(seed)
    p, L = 1000, 3
    k.interval(0, p)
    starts = [952, 958, 964, 970]
    made = 0
    for j, t in enumerate(starts):
        m = n_cand // len(starts) + (1 if j < n_cand % len(starts) else 0)
        s = k.hap_del(0, t, p, L)
        assert k.mismatches(0, t, s) > 0  # an altRead, and with its two blocks a consensus candidate
        for _ in range(m):
            k.add("g", 0, t, f"{p - t}M{L}D{RL - (p - t)}M", s)
            made += 1
        k.add("u", 0, t, f"{RL}M", s)
    assert made == n_cand
    return k


def cap_2048(seed=109):
    return _cap(seed, 2048), 1, 0


def cap_2049(seed=109):
    return _cap(seed, 2049), 1, 1


def nine_ops(seed=110):
    k = Case(seed)
    p = 1000
    k.interval(0, p)
    _site_reads(k, 0, p, 3, range(p - 50, p - 8, 4))
    _nine_op_read(k, 0, p, p - 30)
    return k, 1, 1


def five_op_newcigar(seed=111):
    k = Case(seed)
    p = 1000
    k.interval(0, p)
    _site_reads(k, 0, p, 3, range(960, 990, 4), shapes="g")
    _five_op_read(k, 0, 970)
    return k, 1, 1


def mixed(seed=112):
    """Two contigs, six intervals in file order: device; host (a 9-operation read); device with ungapped reads
    only (no consensus: nothing in the batch); host (a 5-operation new cigar); device; no reads at all."""
    k = Case(seed, 2)
    host = []
    k.interval(0, 500)
    _site_reads(k, 0, 500, 3, range(450, 492, 4))
    host.append(k.interval(0, 1100))
    _site_reads(k, 0, 1100, 3, range(1050, 1092, 4))
    _nine_op_read(k, 0, 1100, 1071)
    k.interval(0, 1700)
    _site_reads(k, 0, 1700, 3, range(1650, 1692, 4), shapes="u")
    host.append(k.interval(1, 500))
    _site_reads(k, 1, 500, 3, range(460, 490, 4), shapes="g")
    _five_op_read(k, 1, 470)
    k.interval(1, 1100)
    _site_reads(k, 1, 1100, 0, range(1050, 1092, 4), ins="ACCA")
    k.interval(1, 1700)
    return k, 5, 2, host


def eq_x_ops(seed=113):
    """Gapped reads written with '=' and 'X' where the others have 'M' (the reference aborts on these: this
    case has no golden and is checked device against host)."""
    k = Case(seed)
    p, L = 1000, 3
    k.interval(0, p)
    for i, t in enumerate(range(p - 50, p - 8, 3)):
        a, b = p - t, RL - (p - t)
        s = k.hap_del(0, t, p, L)
        sh = i % 5
        if sh == 0: k.add("e", 0, t, f"{a}={L}D{b}=", s)
        elif sh == 4: k.add("me", 0, t, f"{a}M{L}D{b}=", s)
        elif sh == 1: k.add("m", 0, t, f"{a}M{L}D{b}M", s)
        elif sh == 2:
            s = s[:5] + ("A" if s[5] != "A" else "C") + s[6:]
            k.add("x", 0, t, f"5=1X{a - 6}M{L}D{b}M", s)
        else: k.add("u", 0, t, f"{RL}=", s)
    return k, 1, 0


CASES = {f.__name__: f for f in (clips, early_indel, homopolymer, contig_start, contig_end, irregular_insert, late_kept,
                                 many_consensuses, cap_2048, cap_2049, nine_ops, five_op_newcigar, mixed, eq_x_ops)}
NO_GOLDEN = ("eq_x_ops",)
GOLDEN_CASES = [n for n in CASES if n not in NO_GOLDEN]


def build_case(name: str, d, seed: int | None = None) -> Built:
    r = CASES[name]() if seed is None else CASES[name](seed)
    k, work, host = r[0], r[1], r[2]
    fa, iv, bam = k.write(d)
    b = Built(name, fa, iv, bam, work, host, golden=name not in NO_GOLDEN)
    if name == "mixed":
        b.host_intervals = r[3]
        b.host_pairs = MIXED_HOST_PAIRS
    return b


# mixed: the scan pairs of its two host intervals, kept consensuses x altReads.  chr1:1076-1126 holds 6 gapped and
# 5 ungapped reads of one deletion and the 9-operation read: one consensus, 12 altReads.  chr2:476-526 holds 8 gapped
# reads of one deletion and the two-indel read, whose own consensus is refused: one consensus, 9 altReads.
# (test_realign_craft.py checks the figure against the host path run on those two intervals alone.)
MIXED_HOST_PAIRS = 12 + 9

GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "rl_craft"


def load_case(name: str, d):
    """Build a case (with its golden's seed) -> (Built, golden dict or None, header, recs, offs[n + 1]); the
    builder's output is checked against the input digests the golden was made from."""
    import hashlib
    import json

    import numpy as np

    import realign_util as R
    meta = json.loads((GOLDEN_DIR / f"{name}.json").read_text()) if name not in NO_GOLDEN else None
    b = build_case(name, d, meta["seed"] if meta else None)
    h, _, recs, offs = bamutil.read_bam(b.bam)
    if meta:
        sha = lambda p: hashlib.sha256(Path(p).read_bytes()).hexdigest()
        inp = meta["input"]
        assert sha(b.fasta) == inp["fasta_sha256"] and sha(b.fasta + ".fai") == inp["fai_sha256"]
        assert sha(b.intervals) == inp["intervals_sha256"]
        assert h == inp["header"] and len(offs) == inp["n"]
        assert R.digest(recs, offs)["stream_sha256"] == inp["records_sha256"]
    recs = np.concatenate([recs, np.zeros(16, np.uint8)])
    offs = np.append(offs, np.uint64(len(recs) - 16))
    return b, meta, h, recs, offs


def check_golden(meta: dict, out, oo) -> None:
    """The output stream is the reference's: n_out and the stream SHA-256; a mismatch names the first differing
    record where the golden carries per-record digests."""
    import numpy as np

    import realign_util as R
    d = R.digest(out, oo[:-1])
    assert len(oo) - 1 == meta["n_out"], (len(oo) - 1, meta["n_out"])
    if d["stream_sha256"] != meta["stream_sha256"]:
        if "per_record" in meta:
            bad = np.nonzero(d["per_record"] != np.array(meta["per_record"], np.uint64))[0]
            k = int(bad[0])
            raise AssertionError(f"{len(bad)} records differ from the reference output; first at {k}: "
                                 f"{bamutil.fields(bamutil.rec_bytes(out, oo[k]))}")
        raise AssertionError("output stream differs from the reference output")
