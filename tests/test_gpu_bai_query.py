"""The index query on the GPU (oge_bai_open, oge_bai_query, oge_bai_query_dev) against bai_query_model: the merged
ranges must be the model's exactly, for the canonical image and for other valid forms of it."""
import random
import struct

import os
import subprocess

import numpy as np
import pytest
import torch

import bai_cases as K
import bai_model as M
import bai_query_model as Q
import bamutil
import regions_model as R
from goldens import GOLDEN, load_case
from openge_amd import lib as L
from test_gpu_cli import OPENGE, case_input
from test_bai_query_model import CASES, regions_for

pytestmark = pytest.mark.gpu
# 1, 2: the smallest; 63, 64, 65: 6 items per region around one workgroup of the count kernel and a wave; 300:
# several workgroups
COUNTS = (1, 2, 63, 64, 65, 300)


def query_both(ctx, image, regions, widen, n_ref=-1):
    h = ctx.bai_open(image, n_ref)
    try:
        host = ctx.bai_query(h, regions, widen)
        d, n = ctx.bai_query_dev(h, regions, widen)
        assert n == len(host) and (d != 0) == (n != 0)
        if n:  # the device form's pairs, read back through the context
            dev = np.frombuffer(ctx._fetch(d, 16 * n), dtype=np.uint64)
            assert [(int(dev[2 * k]), int(dev[2 * k + 1])) for k in range(n)] == host
        assert ctx.counter("baiq_ranges") == n
        return host
    finally:
        ctx.bai_close(h)


def build_case(name, payload):
    refs, recs = CASES[name]()
    bam = K.make_bam(refs, recs, payload=payload)
    bai = M.build_from_bam(bam)
    return dict(name=name, refs=refs, recs=recs, bam=bam, bai=bai, parsed=M.parse(bai))


@pytest.mark.parametrize("payload", [700, 65280])
@pytest.mark.parametrize("name", sorted(CASES))
def test_ranges_equal_the_model(ctx, name, payload):
    case = build_case(name, payload)
    regions = regions_for(case, random.Random(7), 300)
    n_ref = len(case["refs"])
    rev = Q.serialise(case["parsed"], reverse_bins=True)
    bare = Q.serialise(case["parsed"], n_no_coor=False)
    for n in COUNTS:
        sub = regions[:n] if n > 2 else regions[20:20 + n]
        for widen in (0, Q.WIDEN):
            want = Q.merged_ranges(case["parsed"], sub, widen)
            assert query_both(ctx, case["bai"], sub, widen, n_ref) == want, (n, widen)
            assert query_both(ctx, rev, sub, widen, n_ref) == want, (n, widen, "reversed bins")
        assert query_both(ctx, bare, sub, Q.WIDEN) == Q.merged_ranges(case["parsed"], sub, Q.WIDEN)
    # a reference without records in the middle: the later references move up by one
    wide, remap = Q.with_empty_ref(case["parsed"], 1 if n_ref > 1 else 0)
    moved = [(remap(r), a, b) for r, a, b in regions]
    assert query_both(ctx, Q.serialise(wide), moved, Q.WIDEN, n_ref + 1) == Q.merged_ranges(case["parsed"], regions, Q.WIDEN)
    # every region on its own finds what the model finds (one handle for all of them)
    h = ctx.bai_open(case["bai"], n_ref)
    try:
        for reg in regions[:60]:
            assert ctx.bai_query(h, [reg], Q.WIDEN) == Q.merged_ranges(case["parsed"], [reg], Q.WIDEN), reg
        assert ctx.bai_query(h, [], 0) == []
    finally:
        ctx.bai_close(h)


@pytest.fixture(scope="module")
def dense():
    """30,000 records on one reference, alternating between a window's own bin and a wider one, in 700-byte blocks:
    the runs break at every record, so every bin has about one chunk per block and a list of regions asks for tens
    of thousands of ranges -- more than one tile of the radix sort (4096) and of the running maximum (1024)."""
    recs = [K.rec(f"d{i}", 0, 40 * i, "10M" if i % 2 else "10M20000N10M") for i in range(30000)]
    bam = K.make_bam(K.refs(1), recs, payload=700)
    bai = M.build_from_bam(bam)
    return dict(refs=K.refs(1), recs=recs, bam=bam, bai=bai, parsed=M.parse(bai))


@pytest.mark.parametrize("n", [1, 65, 300])
def test_many_ranges_cross_the_sort_and_scan_tiles(ctx, dense, n):
    rng = random.Random(n)
    regions = [(0, a, a + rng.choice([0, 500, 20000, 100000])) for a in (rng.randrange(0, 1_250_000) for _ in range(n))]
    raw = Q.raw_ranges(dense["parsed"], regions, Q.WIDEN)
    if n == 300:
        assert len(raw) > 3 * 4096
    want = Q.union(raw)
    assert len(want) >= 1
    assert query_both(ctx, dense["bai"], regions, Q.WIDEN, 1) == want
    assert query_both(ctx, Q.serialise(dense["parsed"], reverse_bins=True), regions, Q.WIDEN, 1) == want


def test_open_refuses_a_bad_image(ctx):
    case = build_case("refs_and_gaps", 700)
    bai, n_ref = case["bai"], len(case["refs"])
    ctx.bai_close(ctx.bai_open(bai, n_ref))
    ctx.bai_close(ctx.bai_open(bai))
    bad = {
        "magic": b"BAJ\1" + bai[4:],
        "short": bai[:6],
        "cut in a bin": bai[:40],
        "cut in the linear index": bai[:-20],
        "cut by one": bai[:-9],
        "trailing": bai + b"\0" * 4,
        "trailing 16": bai + b"\0" * 16,
        "n_bin too large": bai[:16] + struct.pack("<i", 1 << 30) + bai[20:],
        "n_chunk too large": bai[:24] + struct.pack("<i", 1 << 27) + bai[28:],
        "n_intv too large": bai[:12] + struct.pack("<i", 1 << 28) + bai[16:],
        "negative n_bin": bai[:8] + struct.pack("<i", -1) + bai[12:],
    }
    for why, img in bad.items():
        with pytest.raises(L.OgeError, match=r"error -1: index:"):
            ctx.bai_open(img, n_ref)
    with pytest.raises(L.OgeError, match=r"error -1: index: n_ref 5 differs from the header's 4"):
        ctx.bai_open(bai, n_ref - 1)
    # a refused image launches nothing: the open's prologue, which comes before its first launch and clears the
    # counters of the call before, is not reached
    assert query_both(ctx, bai, [(1, 0, 400_000)], 0, n_ref) and ctx.counter("baiq_ranges") > 0
    with pytest.raises(L.OgeError):
        ctx.bai_open(bad["trailing"], n_ref)
    assert ctx.counter("baiq_ranges") > 0
    ctx.bai_close(ctx.bai_open(bai, n_ref))  # an open that passes does reach it
    assert ctx.counter("baiq_ranges") is None
    # a failed open leaves the context usable
    assert query_both(ctx, bai, [(1, 0, 400_000)], 0, n_ref) == Q.merged_ranges(case["parsed"], [(1, 0, 400_000)], 0)


# ------------------------------------------------------------------------------------------ decode
def spans_of(bam: bytes, ranges):
    """The file spans of ascending ranges: from the first block of a range to the end of the block that holds
    end - 1; spans that touch or lie less than 64 KiB apart are one."""
    spans = []
    for beg, end in ranges:
        sb, se = beg >> 16, end >> 16
        if end & 0xFFFF:
            se += struct.unpack_from("<H", bam, se + 16)[0] + 1
        if spans and sb <= spans[-1][1] + 65536:
            spans[-1][1] = max(spans[-1][1], se)
        else:
            spans.append([sb, se])
    return spans


def decode_dev(ctx, bam: bytes, ranges, n_ref: int, load=None):
    spans = spans_of(bam, load or ranges)  # load: the ranges whose spans are loaded, when not the ranges asked for
    z = b"".join(bam[a:b] for a, b in spans)
    span_z = [0]
    for a, b in spans:
        span_z.append(span_z[-1] + b - a)
    d_z = torch.from_numpy(np.frombuffer(z + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    d_r = torch.from_numpy(np.array([x for r in ranges for x in r], dtype=np.uint64).view(np.int64)).cuda()
    out, offs = ctx.bam_decode_ranges_dev(d_z.data_ptr(), len(z), span_z, [a for a, _ in spans], d_r.data_ptr(), len(ranges), n_ref)
    return [out[a:b] for a, b in zip(offs, offs[1:])], len(z)


@pytest.mark.parametrize("payload", [700, 65280])
def test_decode_of_hand_made_ranges(ctx, payload):
    refs, recs, _idx = K.block_layout(700)  # records of up to 1,600 bytes: over three 700-byte blocks, or all in one
    bam = K.make_bam(refs, recs, payload=payload)
    uoff, cstart = M.block_table(bam)
    _n, base, offs = M.stream_layout(M.inflate_all(bam))

    def voff(x):
        import bisect
        b = bisect.bisect_right(uoff, x) - 1
        return cstart[b] << 16 | (x - uoff[b])

    v = [voff(o) for o in offs] + [voff(offs[-1] + len(recs[-1]))]  # v[i]: record i; v[-1]: the end of the file's records
    assert v[-1] == cstart[-1] << 16
    edge = [i for i in range(1, len(v)) if v[i] & 0xFFFF == 0]
    cases = {
        "inside a block": [(v[1], v[3])],
        "touching": [(v[0], v[2]), (v[2], v[3]), (v[3], v[5])],
        "apart": [(v[0], v[1]), (v[2], v[3]), (v[6], v[7])],
        "to the end of the file": [(v[len(recs) - 2], v[-1])],
        "everything": [(v[0], v[-1])],
        "one record": [(v[5], v[6])],
    }
    if payload == 700:
        assert edge, "block_layout places a record end on a block edge"
        cases["ends at a block edge"] = [(v[edge[0] - 1], v[edge[0]])]
        cases["begins at a block edge"] = [(v[edge[0]], v[edge[0] + 1])]
    rd = M.Reader(bam)
    for why, ranges in cases.items():
        want = [rb for b, e in ranges for _vo, rb in rd.records(b, e)]
        assert want, why
        got, _z = decode_dev(ctx, bam, ranges, len(refs))
        assert got == want, why
    # a range that begins in the middle of a block's compressed bytes, the whole file loaded
    with pytest.raises(L.OgeError, match="index: range 0 does not begin and end in BGZF blocks"):
        decode_dev(ctx, bam, [((cstart[0] + 7) << 16, v[-1])], len(refs), load=[(v[0], v[-1])])
    # a range that reaches past its block's payload
    with pytest.raises(L.OgeError, match="index: range 0 does not begin and end in BGZF blocks"):
        decode_dev(ctx, bam, [(v[0], cstart[0] << 16 | 0xFFFF)], len(refs), load=[(v[0], v[-1])])


@pytest.mark.parametrize("payload", [700, 65280])
@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_of_the_index_ranges_equals_the_reader(ctx, name, payload):
    case = build_case(name, payload)
    regions = regions_for(case, random.Random(3), 120)
    rd = M.Reader(case["bam"])
    for sub in (regions, regions[:1], regions[30:33], regions[::7]):
        ranges = Q.merged_ranges(case["parsed"], sub, Q.WIDEN)
        want = [rb for b, e in ranges for _vo, rb in rd.records(b, e)]
        got, _z = decode_dev(ctx, case["bam"], ranges, len(case["refs"])) if ranges else ([], 0)
        assert got == want


def test_decode_many_ranges(ctx, dense):
    rng = random.Random(9)
    regions = [(0, a, a + rng.choice([0, 50, 300])) for a in (rng.randrange(0, 1_190_000) for _ in range(20))]
    ranges = Q.merged_ranges(dense["parsed"], regions, 0)
    assert len(ranges) > 512  # several workgroups of the position kernel, hundreds of short copies
    rd = M.Reader(dense["bam"])
    want = [rb for b, e in ranges for _vo, rb in rd.records(b, e)]
    got, zbytes = decode_dev(ctx, dense["bam"], ranges, 1)
    assert got == want and zbytes < len(dense["bam"])
    assert ctx.counter("baiq_blocks") < len(M.block_table(dense["bam"])[0]) - 1


# ------------------------------------------------------------------------------------------ the CLI
def cli(*args, env=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env={**os.environ, **(env or {})})


@pytest.fixture(scope="module")
def indexed(tmp_path_factory, built):
    """c2_20k sorted and indexed by the CLI, written in many blocks (one deflate segment per block row)."""
    tmp = tmp_path_factory.mktemp("indexed")
    src = case_input(load_case("c2_20k"), tmp)
    bam = tmp / "s.bam"
    r = cli("sort", "--nopg", "--index", src, "-o", bam, env={"OGE_WRITE_SEG_BLOCKS": "1"})
    assert r.returncode == 0, r.stderr
    assert (tmp / "s.bam.bai").exists()
    _h, refs, recs, offs = bamutil.read_bam(bam)
    records = [bamutil.rec_bytes(recs, o) for o in offs]
    rng = random.Random(4)
    used = sorted({R.core(rb)[0] for rb in records if R.core(rb)[0] >= 0})
    lines, regions = [], []
    for k in range(12):
        ref = rng.choice(used)
        a = rng.choice([R.core(rb)[1] for rb in records if R.core(rb)[0] == ref])
        z = min(a + rng.randrange(0, 60_000), refs[ref][1])
        lines.append(f"{refs[ref][0]}:{a}..{z}")
        regions.append((ref, a, z))
    (tmp / "list.txt").write_text("\n".join(lines) + "\n")
    return dict(tmp=tmp, bam=bam, refs=refs, records=records, regions=regions, lines=lines, list=tmp / "list.txt")


def test_cli_indexed_equals_noindex_and_the_predicate(indexed):
    t, bam = indexed["tmp"], indexed["bam"]
    assert len(M.block_table(bam.read_bytes())[0]) > 20
    runs = {"r": (("-r", indexed["lines"][0]), indexed["regions"][:1]), "L": (("-L", indexed["list"]), indexed["regions"]),
            "rL": (("-r", indexed["lines"][3], "-L", indexed["list"], "-q", "10", "-n", "50"), None)}
    for tag, cmd, fmt in (("r", "view", "bam"), ("r", "view", "sam"), ("L", "view", "bam"), ("L", "sort", "bam"), ("rL", "view", "sam")):
        args, regions = runs[tag]
        a, b = t / f"{tag}_{cmd}_ix.{fmt}", t / f"{tag}_{cmd}_no.{fmt}"
        x = cli(cmd, "--nopg", "-v", *args, bam, "-o", a)
        y = cli(cmd, "--nopg", "-v", "--noindex", *args, bam, "-o", b)
        assert x.returncode == 0 and y.returncode == 0, (x.stderr, y.stderr)
        assert a.read_bytes() == b.read_bytes(), (tag, cmd, fmt)
        line = [ln for ln in x.stderr.decode().splitlines() if "FileReader (indexed)" in ln]
        assert len(line) == 1 and b"(indexed)" not in y.stderr and b"full scan" not in y.stderr, x.stderr
        w = line[0].replace(",", "").split()
        got, of = int(w[w.index("of") - 1]), int(w[w.index("of") + 1])
        assert 0 < got < of == bam.stat().st_size  # fewer bytes read than the file has
        if regions is not None and fmt == "bam" and cmd == "view":
            _h, _r, recs, offs = bamutil.read_bam(a)
            keep = R.keep_regions(indexed["records"], regions)
            assert len(keep) > 0
            assert [bamutil.match_key(bamutil.rec_bytes(recs, o)) for o in offs] == [bamutil.match_key(indexed["records"][i]) for i in keep]


def test_cli_goldens_are_unchanged_with_an_index_beside_the_input(tmp_path):
    """The view -r goldens (tests/golden/view, written by the reference) with an index beside a copy of the input."""
    from test_sam_model import FILES, MANIFEST, same
    import sam_model as SM
    used = 0
    for name in sorted(MANIFEST["filters"]):
        src = tmp_path / f"{name}.bam"
        src.write_bytes((GOLDEN / "inputs" / FILES[name]).read_bytes())
        if cli("index", src).returncode != 0:  # not coordinate-sorted: no index can lie beside it
            continue
        for key, g in sorted(MANIFEST["filters"][name].items()):
            if "-r" not in g["args"]:
                continue
            r = cli("view", "--nopg", "-v", *g["args"], src)
            assert r.returncode == 0, r.stderr
            h, b = SM.split_header(r.stdout)
            assert same(g["header"], h) and same(g["body"], b), (name, key)
            # through the index, or back to the full scan where the region names most of a small file
            assert b"FileReader (indexed)" in r.stderr or b"more than half of the file" in r.stderr, r.stderr
            used += b"FileReader (indexed)" in r.stderr
    assert used > 0


def test_cli_fallbacks_give_the_full_scan(indexed, tmp_path):
    bam, good = indexed["bam"], (indexed["tmp"] / "s.bam.bai").read_bytes()
    args = ("view", "--nopg", "-v", "-L", indexed["list"])
    want = cli(*args, "--noindex", bam).stdout
    assert want.count(b"\n") > 20
    other = K.make_bam(K.refs(2), [K.rec("x", 0, 5)], payload=700)
    parsed = M.parse(good)
    # a chunk that points into the middle of a block: every chunk begin moved 9 bytes into the file
    moved = {"refs": [dict(r, bins={b: [(cb + (9 << 16), ce) for cb, ce in ch] for b, ch in r["bins"].items()}) for r in parsed["refs"]],
             "n_no_coor": parsed["n_no_coor"]}
    cases = {
        "older": (good, "older than the file"),
        "magic": (b"BAJ\1" + good[4:], "no BAI magic"),
        "n_ref": (M.build_from_bam(other), "differs from the header's"),
        "truncated": (good[:-30], "truncated image"),
        "mid-block": (Q.serialise(moved), "index:"),
    }
    for why, (img, msg) in cases.items():
        d = tmp_path / why
        d.mkdir()
        f = d / "in.bam"
        f.write_bytes(bam.read_bytes())
        (d / "in.bam.bai").write_bytes(img)
        now = f.stat().st_mtime
        os.utime(d / "in.bam.bai", (now - 100, now - 100) if why == "older" else (now + 1, now + 1))
        r = cli(*args, f)
        assert r.returncode == 0, (why, r.stderr)
        assert r.stdout == want, why
        err = r.stderr.decode()
        assert "FileReader: full scan" in err and msg in err and "(indexed)" not in err, (why, err)
    # in.bai beside in.bam is found too
    d = tmp_path / "short"
    d.mkdir()
    (d / "in.bam").write_bytes(bam.read_bytes())
    (d / "in.bai").write_bytes(good)
    os.utime(d / "in.bai", (now + 1, now + 1))
    r = cli(*args, d / "in.bam")
    assert r.returncode == 0 and r.stdout == want and b"(indexed)" in r.stderr


def test_cli_bad_line_fails_before_the_file_is_decoded(indexed):
    bad = indexed["tmp"] / "bad.txt"
    bad.write_text(f"{indexed['lines'][0]}\n\nnope:1..2\n")
    out = indexed["tmp"] / "never.bam"
    r = cli("view", "-v", "-L", bad, indexed["bam"], "-o", out)
    assert r.returncode != 0 and b"bad.txt line 3" in r.stderr and b"FileReader (" not in r.stderr
    assert not out.exists() or out.stat().st_size == 0


def test_cli_a_list_that_names_most_of_the_file_takes_the_full_scan(indexed):
    whole = indexed["tmp"] / "whole.txt"
    whole.write_text("".join(f"{n}\n" for n, _ in indexed["refs"]))
    x = cli("view", "--nopg", "-v", "-L", whole, indexed["bam"])
    y = cli("view", "--nopg", "--noindex", "-L", whole, indexed["bam"])
    assert x.returncode == 0 and y.returncode == 0 and x.stdout == y.stdout and x.stdout.count(b"\n") > 1000
    assert b"full scan, the index names more than half of the file" in x.stderr and b"(indexed)" not in x.stderr


def test_paths_without_an_index_record_none_of_the_new_stages(built):
    """What `view -r --noindex` and a chain without a region run -- the whole-file decode, the single-region
    filter -- in a context of their own: none of the stages and counters of the index path appear."""
    c = L.Context(0)
    try:
        refs, recs, _ = K.block_layout(700)
        bam = K.make_bam(refs, recs, payload=700)
        c.bam_index(bam)  # framing index, inflate, header, record walk of a whole file
        packed, offs = bamutil.pack_records(recs)
        d_recs, d_off = torch.from_numpy(packed).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
        d_out = torch.zeros(packed.size + 64, dtype=torch.uint8, device="cuda")
        d_oo = torch.zeros(len(recs) + 1, dtype=torch.int64, device="cuda")
        m = c.filter_records_dev(d_recs.data_ptr(), d_off.data_ptr(), len(recs), L.filter_opts(has_region=1, ref_id=0, left_pos=0, right_pos=500),
                                 d_out.data_ptr(), d_oo.data_ptr())
        assert m > 0 and c.timing("filter") > 0
        for stage in ("bai_query", "ranges_pack", "filter_regions"):
            assert c.timing(stage) == -1, stage
        for counter in ("baiq_ranges", "baiq_blocks"):
            assert c.counter(counter) is None, counter
    finally:
        c.close()
