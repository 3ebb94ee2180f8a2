"""`openge stats`, `count` and `coverage` restated in plain Python / numpy: the flag
counters, `Sorted` in the reference's serial form and in the local form the kernel evaluates, read lengths,
insert sizes, the float32 text renderer, coverage bins by brute force per position and in closed form per bin,
the TSV and the stderr summary.  tests/test_qc_model.py pins it against the reference's recorded output."""
from __future__ import annotations

import struct

import numpy as np

COUNTERS = ("reads", "mapped", "forward", "reverse", "failed_qc", "duplicates", "paired", "proper_pair", "read1", "read2",
            "both_mapped", "singletons")


def cores(recs, offs) -> dict:
    """refid, pos, flag, lseq, tlen of the records recs[offs[i]:] as numpy arrays."""
    buf = recs.tobytes() if isinstance(recs, np.ndarray) else bytes(recs)
    n = len(offs)
    out = {k: np.zeros(n, np.int64) for k in ("refid", "pos", "flag", "lseq", "tlen")}
    for i, o in enumerate(offs):
        o = int(o)
        refid, pos, _ln, _mq, _bin, _nc, flag, lseq, _mr, _mp, tlen = struct.unpack_from("<iiBBHHHiiii", buf, o + 4)
        out["refid"][i], out["pos"][i], out["flag"][i], out["lseq"][i], out["tlen"][i] = refid, pos, flag, lseq, tlen
    return out


def counters(flag: np.ndarray) -> dict:
    f = np.asarray(flag, np.int64)
    mapped, paired = (f & 4) == 0, (f & 1) != 0
    c = {
        "reads": len(f), "mapped": mapped.sum(), "forward": ((f & 0x10) == 0).sum(), "reverse": ((f & 0x10) != 0).sum(),
        "failed_qc": ((f & 0x200) != 0).sum(), "duplicates": ((f & 0x400) != 0).sum(), "paired": paired.sum(),
        "proper_pair": (paired & ((f & 2) != 0)).sum(), "read1": (paired & ((f & 0x40) != 0)).sum(),
        "read2": (paired & ((f & 0x80) != 0)).sum(), "both_mapped": (paired & mapped & ((f & 8) == 0)).sum(),
        "singletons": (paired & mapped & ((f & 8) != 0)).sum(),
    }
    return {k: int(v) for k, v in c.items()}


def sorted_serial(refid, pos) -> bool:
    """Statistics::runInternal's loop: a higher refID resets last_pos to -1 and does NOT record this position."""
    last_rid, last_pos = -1, -1
    for r, p in zip(map(int, refid), map(int, pos)):
        if r == -1 or p == -1:
            continue
        if last_rid > r:
            return False
        if last_rid < r:
            last_rid, last_pos = r, -1
        elif last_pos > p:
            return False
        else:
            last_pos = p
    return True


def sorted_local(refid, pos) -> bool:
    """The local form over the considered records c_0..c_k: unsorted iff some j >= 1 has rid_j < rid_{j-1}, or
    rid_j == rid_{j-1} and j-1 >= 1 and rid_{j-1} == rid_{j-2} and pos_j < pos_{j-1}.  For valid BAM input
    (refID >= -1, pos >= -1)."""
    c = [(int(r), int(p)) for r, p in zip(refid, pos) if r != -1 and p != -1]
    for j in range(1, len(c)):
        if c[j][0] < c[j - 1][0]:
            return False
        if c[j][0] == c[j - 1][0] and j - 1 >= 1 and c[j - 1][0] == c[j - 2][0] and c[j][1] < c[j - 1][1]:
            return False
    return True


def sorted_local_exact(refid, pos) -> bool:
    """The form the kernel evaluates, equal to the serial form for every int32 input: in front of c_0 stand two
    virtual records (-1, -1); c_j is out of order when rid_j < rid_{j-1}, or when rid_j == rid_{j-1} and
    pos_j < (pos_{j-1} if rid_{j-1} == rid_{j-2} else -1)."""
    c = [(-1, -1), (-1, -1)] + [(int(r), int(p)) for r, p in zip(refid, pos) if r != -1 and p != -1]
    for j in range(2, len(c)):
        if c[j][0] < c[j - 1][0]:
            return False
        if c[j][0] == c[j - 1][0] and c[j][1] < (c[j - 1][1] if c[j - 1][0] == c[j - 2][0] else -1):
            return False
    return True


def lengths(lseq) -> tuple[np.ndarray, np.ndarray]:
    v, c = np.unique(np.asarray(lseq, np.int64) & 0xFFFFFFFF, return_counts=True)
    return v.astype(np.uint32), c.astype(np.uint64)


def inserts(flag, tlen) -> dict:
    """Over paired first mates with tlen != 0: count, sum of |tlen| and the two middle order statistics."""
    f, t = np.asarray(flag, np.int64), np.asarray(tlen, np.int64)
    v = np.sort(np.abs(t[((f & 1) != 0) & ((f & 0x40) != 0) & (t != 0)]))
    m = len(v)
    return {"n_insert": m, "insert_sum": int(v.sum()), "insert_mid_lo": int(v[(m - 1) // 2]) if m else 0,
            "insert_mid_hi": int(v[m // 2]) if m else 0}


def stats(recs, offs) -> dict:
    """Everything oge_stats_dev reports, `lengths` included."""
    c = cores(recs, offs)
    out = counters(c["flag"])
    out["sorted"] = sorted_serial(c["refid"], c["pos"])
    out.update(inserts(c["flag"], c["tlen"]))
    out["lengths"] = lengths(c["lseq"])
    return out


def _pct(a: int, b: int) -> str:
    with np.errstate(all="ignore"):
        p = (np.float32(a) / np.float32(b)) * np.float32(100)  # ((float)a / b) * 100
    return "%5.1f" % float(p)


def stats_text(s: dict, show_inserts: bool = False, show_lengths: bool = False) -> tuple[str, str]:
    """(stdout, stderr) of `openge stats [-I] [-L]` (statistics.cpp:157-201)."""
    def line(label, v, of):
        return f"{label}{v:>10} ({_pct(v, of)}%)\n"

    n = s["reads"]
    out = f"Total reads:       {n:>10}\n"
    out += line("Mapped reads:      ", s["mapped"], n) + line("Forward strand:    ", s["forward"], n)
    out += line("Reverse strand:    ", s["reverse"], n) + line("Failed QC:         ", s["failed_qc"], n)
    out += line("Duplicates:        ", s["duplicates"], n) + line("Paired-end reads:  ", s["paired"], n)
    if s["paired"]:
        p = s["paired"]
        out += line("'Proper-pairs':    ", s["proper_pair"], p) + line("Both pairs mapped: ", s["both_mapped"], p)
        out += f"Read 1:            {s['read1']:>10}\nRead 2:            {s['read2']:>10}\n"
        out += line("Singletons:        ", s["singletons"], p)
    out += "Sorted:            %10s\n" % ("Yes" if s["sorted"] else "No")
    err = ""
    if show_lengths:
        err = "Read lengths:\n"
        for ln, ct in zip(*s["lengths"]):
            pct = np.float32(100.0 * float(ct) / float(n))  # double arithmetic stored in a float
            out += " %5d" % int(np.int32(np.uint32(ln))) + "bp:          %10d (%5.1f%%)\n" % (int(ct), float(pct))
    if show_inserts:
        out += "Insert size (absolute value):\n"
        m = s["n_insert"]
        if m:
            out += "    Mean:          %10.1f\n" % (s["insert_sum"] / m)
            med = float(s["insert_mid_hi"]) if m % 2 else (s["insert_mid_hi"] + s["insert_mid_lo"]) / 2.0
            out += "    Median:        %10.1f\n" % med
    return out, err


# ------------------------------------------------------------------------------------------- coverage
def coverage_layout(ref_len, binsize: int) -> np.ndarray:
    base = [0]
    for ln in ref_len:
        base.append(base[-1] + (max(int(ln), 0) + binsize - 1) // binsize)
    return np.array(base, np.uint64)


def counted(c: dict) -> np.ndarray:
    return (c["refid"] != -1) & (c["pos"] != -1)


def defined_by_reference(c: dict, ref_len, binsize: int) -> bool:
    """True when every counted position lies inside its contig's bins (elsewhere the reference writes outside its
    vector)."""
    base = coverage_layout(ref_len, binsize)
    for r, p, l in zip(c["refid"][counted(c)], c["pos"][counted(c)], c["lseq"][counted(c)]):
        if not 0 <= r < len(ref_len) or p < 0 or l < 0 or (p + l) // binsize >= int(base[r + 1] - base[r]):
            return False
    return True


def coverage_brute(c: dict, ref_len, binsize: int) -> tuple[dict, int]:
    """{global bin: count} position by position, and the skipped reads.  Positions below 0 or in a bin past the
    contig's last one are dropped."""
    base = coverage_layout(ref_len, binsize)
    bins, skipped = {}, 0
    for r, p, l in zip(map(int, c["refid"]), map(int, c["pos"]), map(int, c["lseq"])):
        if r == -1 or p == -1:
            skipped += 1
            continue
        nb = int(base[r + 1] - base[r])
        for i in range(p, p + l + 1):
            if i >= 0 and i // binsize < nb:
                g = int(base[r]) + i // binsize
                bins[g] = bins.get(g, 0) + 1
    return bins, skipped


def coverage_sparse(c: dict, ref_len, binsize: int) -> tuple[np.ndarray, np.ndarray, int]:
    """The same in closed form: a read over [lo, hi] gives bin b the overlap min(hi, (b+1)*binsize - 1) -
    max(lo, b*binsize) + 1.  -> (global bins ascending, their counts, skipped)."""
    base = coverage_layout(ref_len, binsize).astype(np.int64)
    k = counted(c)
    r, p, l = c["refid"][k], c["pos"][k], c["lseq"][k]
    assert ((r >= 0) & (r < len(ref_len))).all()
    nb = base[r + 1] - base[r]
    lo, hi = np.maximum(p, 0), np.minimum(p + l, nb * binsize - 1)
    ok = lo <= hi
    r, lo, hi = r[ok], lo[ok], hi[ok]
    b0, b1 = lo // binsize, hi // binsize
    cnt = b1 - b0 + 1
    idx = np.repeat(np.arange(len(r)), cnt)
    b = b0[idx] + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    ov = np.minimum(hi[idx], (b + 1) * binsize - 1) - np.maximum(lo[idx], b * binsize) + 1
    g, inv = np.unique(base[r[idx]] + b, return_inverse=True)
    return g.astype(np.int64), np.bincount(inv, weights=ov, minlength=len(g)).astype(np.int64), int((~k).sum())


def dense(g: np.ndarray, v: np.ndarray, nb: int) -> np.ndarray:
    out = np.zeros(nb, np.uint32)
    out[g] = v
    return out


def coverage_text(names, ref_len, binsize: int, bins: np.ndarray, skipped: int, omit_uncovered: bool, overflow: bool = False):
    """(TSV, stderr summary) of `openge coverage -o FILE` (measure_coverage.cpp:128-181): contigs in bytewise name
    order, every bin or only the non-zero ones."""
    base = coverage_layout(ref_len, binsize)
    order = sorted(range(len(names)), key=lambda r: names[r].encode())
    err = f"Skipped {skipped} unmapped reads.\n" if skipped else ""
    err += "Average coverage:\n"
    tsv = ["chromosome\tposition\tcoverage\n"]
    for r in order:
        b = bins[int(base[r]):int(base[r + 1])]
        err += "   %20s: %8gx\n" % (names[r], float(int(b.sum(dtype=np.uint64))) / ref_len[r])
        idx = np.flatnonzero(b) if omit_uncovered else np.arange(len(b))
        nm = names[r]
        tsv.extend([f"{nm}\t{p}\t{v}\n" for p, v in zip((idx * binsize + 1).tolist(), b[idx].tolist())])
    if overflow:
        err += "Error: at least one overflow occurred when measuring coverage- try reducing binsizes.\n"
    return "".join(tsv), err
