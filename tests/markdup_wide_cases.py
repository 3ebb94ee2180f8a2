"""Directed duplicate-marking and sort inputs at real-genome contig and library counts.

The device MarkDuplicates packs (library, refID, 5' coordinate, strand / orientation, score) into 64-bit
words whose field positions depend on sb = bits for n_ref and lb = bits for the largest library id
(csrc/md_keys.h, csrc/markdup.hip: md_layout); sb + lb may not pass 13.  The sets here sit below, at
and above that limit, with records on the contigs and in the libraries that fill the top bit of every
field, and with "twin" groups whose packed keys differ in one field only, so that a field shifted or
masked one bit short merges two groups and changes the marks.

Every builder is deterministic and returns a `WideSet`; `build(name)` also gives the tuple the
tests use, (header, n_ref, records, twins).  Expected marks are by construction: each cluster is
built with distinct scores and names which of its records is kept.
"""
from __future__ import annotations

import random
import re
import struct
from dataclasses import dataclass, field

from bamutil import make_record

# name -> (n_ref, named libraries, accepted by the packed group key)
LAYOUTS = {
    "w12": (1023, 2, True),     # sb 10 + lb 2
    "w13a": (2047, 2, True),    # sb 11 + lb 2, at the limit
    "w13b": (1023, 3, True),    # sb 10 + lb 3, at the limit
    "w13c": (4095, 0, True),    # sb 12 + lb 1 (no @RG), at the limit
    "w14a": (2048, 1, False),   # sb 12 + lb 2
    "w14b": (2047, 3, False),   # sb 11 + lb 3
}
ACCEPTED = [k for k, v in LAYOUTS.items() if v[2]]
REFUSED = [k for k, v in LAYOUTS.items() if not v[2]]
BIG = 1 << 29       # length of the last contig
PLACED_LEN = 99999  # length of the other contigs that carry clusters
PLAIN_LEN = 999
RL = 50             # read length


def bits_for(v: int) -> int:
    return max(1, int(v).bit_length())


@dataclass
class WideSet:
    name: str
    header: str
    n_ref: int
    refs: list
    records: list          # BAM records (bytes) in input order
    expect: list           # by construction: 1 = marked duplicate, 0 = kept, per input record
    twins: list            # {"name", "field", "patch": [(input index, {field: value})]}
    clusters: dict = field(default_factory=dict)  # cluster name -> input indices
    sb: int = 0
    lb: int = 0
    max_lib: int = 0


def rg_tag(rg: str | None) -> bytes:
    return b"" if rg is None else b"RGZ" + rg.encode() + b"\0"


def contig_name(i: int) -> str:
    return format(i, "x")  # short on purpose: the golden stores the header several times


def make_header(n_ref: int, k_libs: int) -> tuple[str, list]:
    placed = placed_refs(n_ref)
    refs = [(contig_name(i), BIG if i == n_ref - 1 else PLACED_LEN if i in placed else PLAIN_LEN) for i in range(n_ref)]
    h = "@HD\tVN:1.4\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    h += "".join(f"@RG\tID:rg{j}\tLB:L{j}\tSM:s\n" for j in range(1, k_libs + 1))
    return h, refs


def top_ref_bit(n_ref: int) -> int:
    """The top bit of the largest refID: 2^(sb-1) in every accepted layout."""
    return 1 << (bits_for(n_ref - 1) - 1)


def placed_refs(n_ref: int) -> list[int]:
    mid = top_ref_bit(n_ref)
    hi = n_ref - 1
    return sorted({0, 1, mid - 1, mid, 1 | mid, hi ^ mid, n_ref - 2, hi})


def build_set(name: str, seed: int = 29) -> WideSet:
    n_ref, k, _ = LAYOUTS[name]
    rnd = random.Random(seed)
    header, refs = make_header(n_ref, k)
    sb, max_lib = bits_for(n_ref), k + 1
    lb = bits_for(max_lib)
    hi = n_ref - 1
    mid = top_ref_bit(n_ref)
    items = []      # [record bytes, expectation, cluster name or None]
    clusters = {}
    twins = []      # patches keyed by item index (before the shuffle)
    slot = {}

    def lib_rg(lib: int):
        """An RG value that resolves to library id `lib` (the unknown library is max_lib)."""
        if lib <= k:
            return f"rg{lib}"
        return "rgZ"  # not in the header

    lib_lo = None if k == 0 else "rg1"  # library 1 (with no @RG line: the unknown library, RG absent)
    lib_hi = lib_rg(max_lib)

    def base(ref: int) -> int:
        slot[ref] = slot.get(ref, 0) + 1
        assert slot[ref] * 1000 + 1000 < refs[ref][1]
        return slot[ref] * 1000

    def seq(n):
        return "".join(rnd.choice("ACGT") for _ in range(n))

    def add(rec, exp, cluster):
        items.append([rec, exp, cluster])
        if cluster is not None:
            clusters.setdefault(cluster, []).append(len(items) - 1)
        return len(items) - 1

    def frag(nm, ref, pos, rev, q, rg, exp, cluster=None, cigar=f"{RL}M", flag=0, mref=-1, mpos=-1):
        ln = sum(int(x) for x in re.findall(r"(\d+)[MIS=X]", cigar))
        return add(make_record(nm, flag | (0x10 if rev else 0), ref, pos, cigar, seq(ln), bytes([q] * ln), mref=mref,
                               mpos=mpos, tags=rg_tag(rg)), exp, cluster)

    def pair(nm, e1, e2, q, rg, exp, cluster=None, first=0):
        """e = (ref, pos, rev); `first` says which end carries 0x40 and comes first in the input."""
        out = []
        for w in (first, 1 - first):
            (ref, pos, rev), (mr, mp, mrev) = (e1, e2) if w == 0 else (e2, e1)
            fl = 0x1 | (0x40 if w == first else 0x80) | (0x10 if rev else 0) | (0x20 if mrev else 0)
            out.append(add(make_record(nm, fl, ref, pos, f"{RL}M", seq(RL), bytes([q] * RL), mref=mr, mpos=mp,
                                       tags=rg_tag(rg)), exp, cluster))
        return out

    def frag_cluster(cl, ref, pos, rev, rg, qs=(24, 37, 31), **kw):
        """unpaired reads at one 5' end: the best score is kept"""
        return [frag(f"{cl}_{i}", ref, pos, rev, q, rg, int(q != max(qs)), cl, **kw) for i, q in enumerate(qs)]

    def pair_cluster(cl, e1, e2, rg, qs=(22, 35, 28), first=0):
        out = []
        for i, q in enumerate(qs):
            out += pair(f"{cl}_{i}", e1, e2, q, rg, int(q != max(qs)), cl, first)
        return out

    def both(cl, ref, rg):
        p = base(ref)
        frag_cluster(cl + "F", ref, p, False, rg)
        frag_cluster(cl + "R", ref, p, True, rg, qs=(33, 21))
        pair_cluster(cl + "P", (ref, p + 100, False), (ref, p + 400, True), rg)
        return p

    # --- the top of the ref and lib fields, and the bottom
    p_top = both("top", hi, lib_hi)
    p_bot = both("bot", 0, lib_lo)
    # fragments at a pair's 5' end ("contains pairs"): every unpaired one is marked whatever it scores
    for cl, pc, ref, p, rg in (("cpT", "topP", hi, p_top, lib_hi), ("cpB", "botP", 0, p_bot, lib_lo)):
        frag(cl + "_u", ref, p + 100, False, 45, rg, 1, pc)
        frag(cl + "_m", ref, p + 100, False, 44, rg, 1, pc, flag=0x1 | 0x8 | 0x40, mref=ref, mpos=p + 100)
        # its unmapped mate, placed on the contig: written through
        add(make_record(cl + "_m", 0x1 | 0x80 | 0x4, ref, p + 100, "", seq(RL), bytes([30] * RL), mapq=0,
                        mref=ref, mpos=p + 100, tags=rg_tag(rg)), 0, None)
    # --- a cluster on each of the other placed contigs, same coordinates on all of them
    for ref in (1, mid - 1, mid, n_ref - 2):
        both(f"r{ref}", ref, lib_lo)

    def twin(nm, fld, group_b, patch):
        twins.append({"name": nm, "field": fld, "patch": [(i, dict(patch(i))) for i in group_b]})

    def patch_ref(to_ref, from_ref):
        def f(i):
            refid, = struct.unpack_from("<i", items[i][0], 4)
            mref, = struct.unpack_from("<i", items[i][0], 24)
            d = {}
            if refid == from_ref:
                d["refid"] = to_ref
            if mref == from_ref:
                d["mref"] = to_ref
            return d
        return f

    # --- twins: one ref bit (the top one) between two fragment groups / two pair groups
    for a, b, rev, rg in ((0, mid, False, lib_lo), (hi ^ mid, hi, True, lib_hi)):
        pa, pb = base(a), base(b)
        pa = pb = max(pa, pb)
        slot[a] = slot[b] = pa // 1000
        frag_cluster(f"tfr{a}a", a, pa, rev, rg, qs=(30, 20))
        gb = frag_cluster(f"tfr{a}b", b, pb, rev, rg, qs=(35, 25))
        twin(f"frag_ref_{a}_{b}", "ref", gb, patch_ref(a, b))
        # pairs, both ends on the contig
        pair_cluster(f"tpr{a}a", (a, pa + 100, False), (a, pa + 400, True), rg, qs=(30, 20))
        gb = pair_cluster(f"tpr{a}b", (b, pb + 100, False), (b, pb + 400, True), rg, qs=(35, 25))
        twin(f"pair_ref_{a}_{b}", "ref", gb, patch_ref(a, b))
    # pairs with the same read1 end and read2 on contigs that differ in the top bit, and the other way round
    p0, p1, p1m, ph = base(0), base(1), base(1 | mid), base(hi)
    p1 = p1m = max(p1, p1m)
    slot[1] = slot[1 | mid] = p1 // 1000
    pair_cluster("t2a", (0, p0 + 100, False), (1, p1 + 400, True), lib_lo, qs=(30, 20))
    gb = pair_cluster("t2b", (0, p0 + 100, False), (1 | mid, p1 + 400, True), lib_lo, qs=(35, 25), first=1)
    twin("pair_ref2", "ref2", gb, patch_ref(1, 1 | mid))
    pair_cluster("t1a", (1, p1 + 100, False), (hi, ph + 400, True), lib_hi, qs=(30, 20), first=1)
    gb = pair_cluster("t1b", (1 | mid, p1 + 100, False), (hi, ph + 400, True), lib_hi, qs=(35, 25))
    twin("pair_ref1", "ref1", gb, patch_ref(1, 1 | mid))
    # --- twins: one library bit.  Library ids start at 1, so a partner that differs in the top lb bit alone
    # exists only where max_lib ^ top is an id (k = 2: 3 and 1); otherwise (k = 3: ids 1..4) the partner is
    # library 1, which still differs from max_lib in the top bit.  With no @RG there is one library, no twin.
    if max_lib > 1:
        top = 1 << (lb - 1)
        la, lbb = (max_lib ^ top) if (max_lib ^ top) >= 1 else 1, max_lib
        p = base(hi)
        frag_cluster("tfla", hi, p, True, lib_rg(la), qs=(30, 20))
        gb = frag_cluster("tflb", hi, p, True, lib_rg(lbb), qs=(35, 25))
        twin("frag_lib", "lib", gb, lambda i: {"rg": lib_rg(la)})
        pair_cluster("tpla", (hi, p + 100, False), (hi, p + 400, True), lib_rg(la), qs=(30, 20))
        gb = pair_cluster("tplb", (hi, p + 100, False), (hi, p + 400, True), lib_rg(lbb), qs=(35, 25))
        twin("pair_lib", "lib", gb, lambda i: {"rg": lib_rg(la)})
    # --- twins: orientation.  FR, FF and RF pairs with the same two 5' ends (forward: pos; reverse: pos + RL - 1)
    p = base(hi)
    c1, c2 = p + 100, p + 449
    pair_cluster("toFR", (hi, c1, False), (hi, c2 - RL + 1, True), lib_hi, qs=(30, 20))
    gff = pair_cluster("toFF", (hi, c1, False), (hi, c2, False), lib_hi, qs=(35, 25))
    grf = pair_cluster("toRF", (hi, c1 - RL + 1, True), (hi, c2, False), lib_hi, qs=(36, 26), first=1)

    def to_fr(i):
        refid, pos, _, _, _, _, fl, _, mref, mpos, _ = struct.unpack_from("<iiBBHHHiiii", items[i][0], 4)
        d = {}
        # make the end at c1 forward and the end at c2 reverse
        if pos in (c1, c1 - RL + 1):
            d["pos"], d["flag"], d["mpos"] = c1, (fl & ~0x10) | 0x20, c2 - RL + 1
        else:
            d["pos"], d["flag"], d["mpos"] = c2 - RL + 1, (fl | 0x10) & ~0x20, c1
        return d

    twin("pair_orient_FF", "orient", gff, to_fr)
    twin("pair_orient_RF", "orient", grf, to_fr)
    # --- pairs that span contig 0 and the last one, the first-in-file read on either: one group
    pa, pb = base(0), base(hi)
    for i, (q, first) in enumerate(((23, 0), (32, 0), (29, 1), (38, 1))):
        pair(f"span_{i}", (0, pa, False), (hi, pb, True), q, lib_lo, int(q != 38), "span", first)
    # --- leading soft clips that make the unclipped start negative, next to the ref field
    for cl, ref, rg in (("negT", hi, lib_hi), ("negB", 0, lib_lo)):
        frag(cl + "_0", ref, 2, False, 30, rg, 1, cl, cigar="10S40M")
        frag(cl + "_1", ref, 0, False, 36, rg, 0, cl, cigar="8S42M")
        frag(cl + "_2", ref, 1, False, 20, rg, 1, cl, cigar="9H50M")
        frag(cl + "_x", ref, 2, False, 20, rg, 0, None, cigar="9S41M")    # -7: alone
    # --- positions just below 2^29 on the contig of that length; reverse ends past the contig end
    frag_cluster("endF", hi, BIG - RL, False, lib_hi)
    pair_cluster("endP", (hi, BIG - 300, False), (hi, BIG - RL, True), lib_hi)
    frag("past_0", hi, BIG - 40, True, 30, lib_hi, 1, "past", cigar="40M10S")
    frag("past_1", hi, BIG - 45, True, 40, lib_hi, 0, "past", cigar="45M10S")  # both end at 2^29 + 9
    frag("past_x", hi, BIG - 40, True, 20, lib_hi, 0, None, cigar="40M11S")
    # --- an RG that the header lacks and no RG at all are one library; a named one is another
    p = base(1)
    frag("unk_z", 1, p, False, 30, "rgZ", 0, "unk")
    frag("unk_n", 1, p, False, 20, None, 1, "unk")
    frag("unk_1", 1, p, False, 25, "rg1", 1 if k == 0 else 0, "unk" if k == 0 else None)
    # --- unmapped: a placed one at a duplicate's position on the last contig, and the refID -1 tail
    add(make_record("placed", 0x4, hi, p_top, "", seq(RL), bytes([40] * RL), mapq=0, tags=rg_tag(lib_hi)), 0, None)
    for i in range(5):
        add(make_record(f"tail{i}", 0x4, -1, -1, "", seq(RL), bytes([40] * RL), mapq=0, tags=rg_tag(lib_hi if i & 1 else None)),
            0, None)
    # --- one read on many other contigs (no duplicates), so the sort and the windows see the whole refID range
    for ref in range(2, n_ref - 2, 7):
        if ref not in placed_refs(n_ref):
            frag(f"bg{ref}", ref, 100 + ref * 37 % 800, bool(ref & 1), 30, lib_rg(1 + ref % max_lib), 0)

    order = list(range(len(items)))
    rnd.shuffle(order)
    where = {old: new for new, old in enumerate(order)}
    records = [items[o][0] for o in order]
    expect = [items[o][1] for o in order]
    for t in twins:
        t["patch"] = [(where[i], d) for i, d in t["patch"]]
    cl = {c: sorted(where[i] for i in v) for c, v in clusters.items()}
    return WideSet(name, header, n_ref, refs, records, expect, twins, cl, sb, lb, max_lib)


_FIELD_OFF = {"refid": (4, "<i"), "pos": (8, "<i"), "flag": (18, "<H"), "mref": (24, "<i"), "mpos": (28, "<i")}


def apply_twin(records: list, twin: dict) -> list:
    """The records with one twin group rewritten onto its partner's key (ref, lib or orientation)."""
    out = list(records)
    for i, d in twin["patch"]:
        b = bytearray(out[i])
        for k, v in d.items():
            if k == "rg":
                j = b.rfind(b"RGZ")
                new = b[:j] + rg_tag(v)
                struct.pack_into("<I", new, 0, len(new) - 4)
                b = new
            else:
                off, fmt = _FIELD_OFF[k]
                struct.pack_into(fmt, b, off, v)
        out[i] = bytes(b)
    return out


_cache: dict = {}


def get(name: str) -> WideSet:
    if name not in _cache:
        _cache[name] = build_set(name)
    return _cache[name]


def build(name: str):
    s = get(name)
    return s.header, s.n_ref, s.records, s.twins
