"""The index query on the Python model alone (bai_query_model over bai_model): what the merged ranges are, and
that decoding them and then applying the Filter's predicate gives what the predicate gives on the whole file --
the argument behind asking the index for [left_pos - W, right_pos + 1)."""
import random
import struct

import pytest

import bai_cases as K
import bai_model as M
import bai_query_model as Q
import regions_model as R


def soft_clip_edge():
    """Records whose pos + l_seq reaches into the next 16 Ki / 128 Ki window while their reference span (what the
    index was built from) ends before it: 2M8S and 1M9I just before an edge."""
    rows = []
    for shift in (14, 17, 20):
        edge = 3 << shift
        rows += [(edge - 5, "2M8S"), (edge - 3, "1M9I"), (edge + 100, "10M")]
    rows.sort()
    return K.refs(2), [K.rec(f"s{i}", 0, p, c) for i, (p, c) in enumerate(rows)]


CASES = {**K.CRAFTED, "soft_clip_edge": soft_clip_edge, "block_layout_700": lambda: K.block_layout(700)[:2]}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    refs, recs = CASES[request.param]()
    payload = 700 if request.param != "bin_edges" else 65280
    bam = K.make_bam(refs, recs, payload=payload)
    bai = M.build_from_bam(bam)
    return dict(name=request.param, refs=refs, recs=recs, bam=bam, bai=bai, parsed=M.parse(bai), reader=M.Reader(bam))


def regions_for(case, rng, n):
    """Random regions plus the ones that can go wrong: left_pos < W, edges of every bin level, a reference
    without records, a position past the last window, the positions just behind every record's start.  No ref_id
    -1: oge_parse_region gives none, and the reads without a reference are in no bin."""
    n_ref = len(case["refs"])
    starts = sorted({R.core(rb)[1] for rb in case["recs"] if R.core(rb)[0] >= 0})
    out = [(0, 0, 0), (0, 5, Q.WIDEN - 1), (n_ref - 1, 0, K.REF_LEN), (0, K.REF_LEN - 1, K.REF_LEN), (n_ref + 2, 0, 100),
           (0, 1 << 28, (1 << 28) + 5)]
    for shift in (14, 17, 20, 23, 26):
        for mult in (1, 3):
            e = mult << shift
            out += [(0, e, e), (0, e - 1, e - 1), (0, e + 1, e + 9), (0, e - 20, e + 20)]
    for s in starts[:40]:
        out += [(rng.randrange(n_ref), s + 1, s + 1), (rng.randrange(n_ref), s + 9, s + 12), (rng.randrange(n_ref), s - 1, s - 1)]
    while len(out) < n:
        ref = rng.randrange(n_ref)
        a = rng.choice(starts) + rng.randrange(-30000, 30000) if starts and rng.random() < 0.7 else rng.randrange(K.REF_LEN)
        a = max(0, a)
        out.append((ref, a, min(K.REF_LEN, a + rng.choice([0, 1, 10, 1000, 20000, 1 << 20]))))
    return out


def decode(case, ranges) -> list[bytes]:
    return [rb for b, e in ranges for _vo, rb in case["reader"].records(b, e)]


def all_records(case) -> list[bytes]:
    return list(case["recs"])


def test_decoding_the_ranges_then_filtering_equals_filtering_the_file(case):
    rng = random.Random(len(case["recs"]))
    regions = regions_for(case, rng, 300)
    recs = all_records(case)
    for reg in regions:
        ranges = Q.merged_ranges(case["parsed"], [reg], Q.WIDEN)
        got = decode(case, ranges)
        want = [recs[i] for i in R.keep_regions(recs, [reg])]
        assert [got[i] for i in R.keep_regions(got, [reg])] == want, reg
    # the whole list at once, and halves of it: still exact, every record once, in file order
    for sub in (regions, regions[::2], regions[:7]):
        got = decode(case, Q.merged_ranges(case["parsed"], sub, Q.WIDEN))
        assert [got[i] for i in R.keep_regions(got, sub)] == [recs[i] for i in R.keep_regions(recs, sub)]


def test_without_widening_a_soft_clipped_read_is_missed():
    refs, recs = soft_clip_edge()
    bam = K.make_bam(refs, recs, payload=700)
    parsed, rd = M.parse(M.build_from_bam(bam)), M.Reader(bam)
    reg = (0, (3 << 14) + 1, (3 << 14) + 2)  # reached by pos + l_seq of the 2M8S and 1M9I reads only
    want = [recs[i] for i in R.keep_regions(recs, [reg])]
    assert len(want) == 2

    def kept(widen):
        got = [rb for b, e in Q.merged_ranges(parsed, [reg], widen) for _v, rb in rd.records(b, e)]
        return [got[i] for i in R.keep_regions(got, [reg])]

    assert kept(Q.WIDEN) == want and kept(0) != want


def test_bins_in_reverse_order_give_the_same_ranges(case):
    rng = random.Random(1)
    regions = regions_for(case, rng, 120)
    rev = Q.serialise(case["parsed"], reverse_bins=True)
    assert Q.serialise(case["parsed"]) == case["bai"]
    if any(r["bins"] for r in case["parsed"]["refs"]):
        assert rev != case["bai"]
    for sub in (regions, regions[:1], regions[5:9]):
        assert Q.merged_ranges(rev, sub, Q.WIDEN) == Q.merged_ranges(case["bai"], sub, Q.WIDEN)


def test_overlapping_nested_duplicate_and_touching_regions_give_the_union(case):
    starts = sorted({R.core(rb)[1] for rb in case["recs"] if R.core(rb)[0] >= 0}) or [0]
    s = starts[len(starts) // 2]
    ref = next((R.core(rb)[0] for rb in case["recs"] if R.core(rb)[0] >= 0), 0)
    a = (ref, max(0, s - 40000), s + 10)
    lists = [[a, a], [a, (ref, s, s + 5)], [a, (ref, s + 11, s + 90000)], [a, (ref, s - 5, s + 70000)],
             [(ref, 0, K.REF_LEN), a]]
    for regs in lists:
        parts = [x for r in regs for x in Q.merged_ranges(case["parsed"], [r], 0)]
        got = Q.merged_ranges(case["parsed"], regs, 0)
        assert got == Q.union(parts)
        assert all(b < e for b, e in got) and all(x[1] < y[0] for x, y in zip(got, got[1:]))


def test_an_image_without_n_no_coor_parses_to_the_same_ranges(case):
    img = Q.serialise(case["parsed"], n_no_coor=False)
    assert len(img) + 8 == len(case["bai"]) and struct.unpack_from("<i", img, 4)[0] == len(case["refs"])
