"""Python restatement of `openge compare` (the reference's commands/command_compare.cpp and the region parser
Filter::ParseRegionString, algorithms/filter.cpp:34-136): region membership, the element order, the multiset counts
and the exact text.  Held to the reference's recorded bytes by tests/test_compare_model.py; the GPU implementation
(csrc/compare.hip, compare_files) is held to this model by tests/test_gpu_compare.py."""
from __future__ import annotations

import struct
from collections import Counter

INT_MAX = 2**31 - 1
NO_REGION = (0, 0, INT_MAX, INT_MAX)
TYPES = "MIDNSHP=X"


def elements(recs, offs, region=NO_REGION) -> list[tuple]:
    """The elements (refID, pos, ((length, type char), ...)) of the records that belong to the region: those whose
    START lies in it, both ends inclusive (regionContainsRead)."""
    lr, lp, rr, rp = region
    out = []
    buf = bytes(recs)
    for o in offs:
        o = int(o)
        refid, pos, lname = struct.unpack_from("<iiB", buf, o + 4)
        if not (lr <= refid <= rr and lp <= pos <= rp):
            continue
        (ncig,) = struct.unpack_from("<H", buf, o + 16)
        ops = struct.unpack_from(f"<{ncig}I", buf, o + 36 + lname)
        out.append((refid, pos, tuple((op >> 4, TYPES[op & 0xF]) for op in ops)))
    return out


def order_key(e: tuple):
    """CompareElement::operator<: refID, pos, the number of ops, then per op the length and the type CHARACTER"""
    refid, pos, ops = e
    return (refid, pos, len(ops), tuple((ln, ord(t)) for ln, t in ops))


def compare(a: list[tuple], b: list[tuple]) -> dict:
    """File 0's elements a against another file's b: the counts, and the surplus elements of either side in order,
    each repeated by its surplus multiplicity (std::set_intersection / set_difference on the sorted vectors)."""
    ca, cb = Counter(a), Counter(b)
    common = sum(min(n, cb[e]) for e, n in ca.items())
    adds = sorted((e for e, n in cb.items() for _ in range(n - min(n, ca[e]))), key=order_key)
    dels = sorted((e for e, n in ca.items() for _ in range(n - min(n, cb[e]))), key=order_key)
    return {"n_ref": len(a), "n_other": len(b), "common": common, "additions": len(b) - common, "deletions": len(a) - common,
            "adds": adds, "dels": dels}


def diff_entries(res: dict) -> list[tuple]:
    """The diff as the device reports it, ordered: (side, refID, pos, surplus, ops) with side 1 = addition"""
    out = []
    for side, key in ((1, "adds"), (0, "dels")):
        for e, n in sorted(Counter(res[key]).items(), key=lambda kv: order_key(kv[0])):
            out.append((side, e[0], e[1], n, e[2]))
    return out


def _atoi(s: str) -> int:
    s = s.lstrip(" \t\n\v\f\r")
    k = 1 if s[:1] in "+-" else 0
    j = k
    while j < len(s) and s[j].isdigit():
        j += 1
    return int(s[:j]) if j > k else 0


def parse_region(rs: str, refs: list[tuple[str, int]]):
    """Filter::ParseRegionString -> ((left_ref, left_pos, right_ref, right_pos) or None, what it prints on stderr)"""
    if not rs:
        return None, ""
    c1 = rs.find(":")
    if c1 < 0:
        chrom, start, stop = rs, 0, -1
    else:
        chrom = rs[:c1]
        dots = rs.find("..", c1 + 1)
        if dots < 0:
            start = stop = _atoi(rs[c1 + 1:])
        else:
            start = _atoi(rs[c1 + 1:dots])
            if rs.find(":", dots + 1) >= 0:
                return None, ""
            stop = _atoi(rs[dots + 2:])
    ref = -1
    for i, (name, _ln) in enumerate(refs):
        if name == chrom:
            ref = i
    if ref == -1:
        return None, f"Can't find chromosome'{chrom}'\n"
    ln = refs[ref][1]
    if start >= ln:
        return None, f"Start position ({start}) after end of the reference sequence ({ln})\n"
    if stop > ln:
        return None, f"Start position ({stop}) after end of the reference sequence ({ln})\n"
    if stop == -1:
        stop = ln
    return (ref, start, ref, stop), ""


def element_text(e: tuple, names: list[str]) -> str:
    return f"{names[e[0]]}:{e[1]} " + "".join(f"{ln}{t}" for ln, t in e[2])


def run(files: list[tuple], refs: list[tuple[str, int]], region_strings: list[str] | None = None, print_changes: bool = False):
    """CompareCommand::runCommand on files = [(name, recs, offs)], refs = file 0's dictionary
    -> (stdout, stderr, exit status)"""
    out, err = [], []
    if region_strings:
        regions = []
        for rs in region_strings:
            rg, msg = parse_region(rs, refs)
            err.append(msg)
            if rg is None:
                err.append(f"Couldn't understand region string {rs}. Exiting.\n")
                return "", "".join(err), 255
            regions.append(rg)
        strings = list(region_strings)
        longest = max(len(s) for s in strings)
    else:
        regions, strings, longest = [NO_REGION], [""], 0
    names = [n for n, _ in refs]
    with_names = len(files) > 2
    ref = [elements(files[0][1], files[0][2], rg) for rg in regions] if files else []
    for name, recs, offs in files[1:]:
        if with_names:
            err.append(f"{name}:\n")
        for k, rg in enumerate(regions):
            res = compare(ref[k], elements(recs, offs, rg))
            if print_changes:
                out += [f"Add: {element_text(e, names)}\n" for e in res["adds"]]
                out += [f"Del: {element_text(e, names)}\n" for e in res["dels"]]
            if res["additions"] or res["deletions"]:
                out.append(f"{'   ' if with_names else ''}{strings[k]:>{longest}}\t{res['additions']:8d} added\t{res['deletions']:8d} removed\n")
    return "".join(out), "".join(err), 0
