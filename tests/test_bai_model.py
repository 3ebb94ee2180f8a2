"""CPU: the Python restatement of the canonical BAM index (tests/bai_model.py) finds what a brute-force scan
finds, on the golden sorted outputs and on the crafted cases the GPU tests compare the device against."""
import random
import struct

import pytest

import bai_cases as K
import bai_model as M
import bamutil
from goldens import load_case
from test_gpu_cli import _refs


def check_queries(bam: bytes, bai: bytes, n_regions: int, seed: int) -> None:
    M.check_invariants(bai)
    idx, rd = M.parse(bai), M.Reader(bam)
    raw = M.inflate_all(bam)
    n_ref, _base, offs = M.stream_layout(raw)
    spans = [M.span(raw[o:o + 4 + struct.unpack_from("<I", raw, o)[0]]) for o in offs]
    assert idx["n_no_coor"] == sum(1 for s in spans if s[0] < 0)
    for r in range(n_ref):
        assert M.query(idx, bam, r, 0, 1 << 29, rd) == M.brute(bam, r, 0, 1 << 29)
    placed = [s for s in spans if s[0] >= 0]
    rng = random.Random(seed)
    for _ in range(n_regions if placed else 0):
        r, rbeg, rend, _f = rng.choice(placed)
        beg = max(0, rbeg + rng.randint(-40_000, 40_000))
        end = min(1 << 29, beg + rng.choice((1, 50, 1000, 20_000, 400_000)))
        assert M.query(idx, bam, r, beg, end, rd) == M.brute(bam, r, beg, end), (r, beg, end)


def sorted_bam(case, payload=65280) -> bytes:
    """The case's records in the golden sorted order (the reference's own output order)."""
    if "perm" in case.arrays:
        perm = case.arrays["perm"]
    else:
        key = [((int.from_bytes(case.recs[int(o) + 4:int(o) + 8].tobytes(), "little")),
                int.from_bytes(case.recs[int(o) + 8:int(o) + 12].tobytes(), "little", signed=True)) for o in case.offs[:-1]]
        perm = sorted(range(case.n), key=lambda i: key[i])
    recs = [bamutil.rec_bytes(case.recs, case.offs[i]) for i in perm]
    return K.make_bam(_refs(case.header), recs, payload, level=1)


@pytest.mark.parametrize("name,regions", [("simple", 300), ("yhet208", 300), ("mix3k", 300), ("c2_20k", 200)])
def test_query_equals_brute_force_on_golden_outputs(built, name, regions):
    bam = sorted_bam(load_case(name))
    check_queries(bam, M.build_from_bam(bam), regions, seed=len(name))


@pytest.mark.parametrize("payload", [700, 65280])
@pytest.mark.parametrize("name", list(K.CRAFTED))
def test_query_equals_brute_force_on_crafted_cases(name, payload):
    refs, recs = K.CRAFTED[name]()
    bam = K.make_bam(refs, recs, payload)
    check_queries(bam, M.build_from_bam(bam), 200, seed=payload)


@pytest.mark.parametrize("payload", [700, 4096, 65280])
def test_block_layout_cases_are_what_they_claim(payload):
    refs, recs, idx = K.block_layout(payload, 140_000 if payload == 65280 else None)
    bam = K.make_bam(refs, recs, payload)
    raw = M.inflate_all(bam)
    _n, _b, offs = M.stream_layout(raw)
    ends = [o + len(r) for o, r in zip(offs, recs)]
    assert ends[idx["edge"]] % payload == 0                                  # ends exactly on a payload boundary
    assert ends[idx["big"]] // payload - offs[idx["big"]] // payload >= 2    # spans three blocks
    bai = M.build_from_bam(bam)
    bins = M.parse(bai)["refs"][0]["bins"]
    assert len(bins[4681]) == 1    # revisited in the same block: merged
    assert len(bins[4682]) == 2    # revisited in a later block: not merged
    uoff, cstart = M.block_table(bam)
    b = ends[idx["edge"]] // payload
    assert bins[4681][0][1] == cstart[b] << 16  # the record on the edge ends at offset 0 of the next block
    check_queries(bam, bai, 100, seed=1)


def test_last_record_ends_at_the_table_end():
    refs, recs = K.one_record()
    bam = K.make_bam(refs, recs)
    uoff, cstart = M.block_table(bam)
    assert M.parse(M.build_from_bam(bam))["refs"][0]["pseudo"][1] == cstart[-1] << 16 == (len(bam) - 28) << 16


def test_errors():
    refs, recs = K.over_limit()
    with pytest.raises(M.Limit) as e:
        M.build_from_bam(K.make_bam(refs, recs))
    assert e.value.index == 1
    refs, recs = K.bin_edges()
    recs[3], recs[4] = recs[4], recs[3]
    with pytest.raises(M.Unsorted) as e:
        M.build_from_bam(K.make_bam(refs, recs))
    assert e.value.index == 4
    refs, recs = K.refs_and_gaps()
    with pytest.raises(M.Unsorted):  # a placed read after the unplaced ones
        M.build_from_bam(K.make_bam(refs, recs + [K.rec("late", 4, 5)]))
