"""The model of `openge targets` (tests/targets_model.py) on hand-worked cases and on the crafted realignment cases:
its intervals lie inside the cases' own and realign to the same bytes."""
from __future__ import annotations

import re

import pytest

import bamutil
import realign_cases as RC
import realign_util as R
import targets_cases as TC
import targets_model as M

REFS = TC.REFS


def run(elements, refs=REFS, **kw):
    return M.targets(TC.recs_of(elements), refs, **kw)


def rows(res):
    return [tuple(int(v) for v in r) for r in res.array]


def test_one_deletion_and_one_insertion():
    r = run([(0, 100, "10M2D10M"), (1, 49, "1M3I5M")])
    assert rows(r) == [(0, 110, 112, 1), (1, 50, 51, 1)]
    assert r.text == b"chrA:110-112\nchrB:50-51\n"
    assert r.counters() == dict(reads_used=2, events=2, intervals=2, dropped_long=0, targets=2, text_bytes=24)


def test_end_indels_do_not_count():
    r = run([(0, 100, "2I10M"), (0, 200, "10M2D"), (0, 300, "5S2I10M"), (0, 400, "5H5S10M2I3S"), (0, 500, "10M2I10M5S")])
    assert rows(r) == [(0, 510, 511, 1)] and r.reads_used == 5 and r.events == 1


def test_n_and_p_are_never_events_but_n_consumes():
    r = run([(0, 100, "10M100N5M2D5M"), (0, 1000, "5M2P5M1I5M")])
    assert rows(r) == [(0, 215, 217, 1), (0, 1010, 1011, 1)]


def test_eq_x_anchor_and_adjacent_indels_both_count():
    r = run([(0, 100, "5=2I5X"), (0, 500, "10M2I3D10M")])
    assert rows(r) == [(0, 105, 106, 1), (0, 510, 513, 2)]  # the I (510, 511) and the D (510, 513)


def test_filter():
    recs, refs = TC.cases()["filters"]
    r = M.targets(recs, refs)
    assert [row[1] for row in rows(r)] == [1510, 1710, 1910, 2310, 2510]
    assert r.reads_used == 5


def test_enclosing_deletion_and_gap():
    recs, refs = TC.cases()["enclose"]
    assert rows(M.targets(recs, refs)) == [(0, 100, 400, 4), (0, 401, 402, 1)]
    assert rows(M.targets(recs, refs, gap=1)) == [(0, 100, 402, 5)]


def test_drop_at_max_interval():
    recs, refs = TC.cases()["width_499_500"]
    r = M.targets(recs, refs)
    assert rows(r) == [(0, 1010, 1509, 1), (1, 110, 111, 1)] and r.dropped_long == 2 and r.intervals == 4
    assert M.targets(recs, refs, max_interval=501).targets == 3
    recs, refs = TC.cases()["chain5000"]
    r = M.targets(recs, refs)
    assert (r.events, r.intervals, r.dropped_long, r.targets, r.text) == (5000, 1, 1, 0, b"")
    assert rows(M.targets(recs, refs, max_interval=100000)) == [(0, 1005, 1005 + 3 * 4999 + 5, 5000)]


def test_contig_change_never_merges():
    recs, refs = TC.cases()["contigs3"]
    for gap in (0, 10, 10 ** 6):
        got = rows(M.targets(recs, refs, gap=gap, max_interval=10 ** 7))
        assert max(r[2] for r in got if r[0] == 0) == 90000
        assert min(r[1] for r in got if r[0] == 1) == 5 and min(r[1] for r in got if r[0] == 2) == 1
        assert sum(r[3] for r in got) == 6


def test_stop_is_clipped_to_the_contig():
    recs, refs = TC.cases()["clip_end"]
    assert rows(M.targets(recs, refs)) == [(1, 49950, 50000, 1), (2, 3000, 3000, 1)]


def test_every_decimal_width():
    recs, refs = TC.cases()["widths"]
    text = M.targets(recs, refs).text.decode().splitlines()
    assert text[:3] == ["big:9-10", "big:99-100", "big:999-1000"] and text[8] == "big:999999999-1000000000"
    assert text[9] == "big:2147483605-2147483606" and text[10] == "small:99-100"


def test_input_order_does_not_matter():
    c = TC.cases()
    a, b = M.targets(*c["mixed"]), M.targets(*c["mixed_shuffled"])
    assert a.text == b.text and (a.array == b.array).all() and a.counters() == b.counters() and a.targets > 100


def test_errors_name_the_lowest_record():
    for name, (recs, refs, bad, kind) in TC.error_cases().items():
        if bad is None:
            assert M.targets(recs, refs).reads_used == 5
            continue
        with pytest.raises(M.TargetsError) as e:
            M.targets(recs, refs)
        assert (e.value.record, e.value.kind) == (bad, kind), name
        assert f"record {bad} " in str(e.value)


def test_options_are_checked():
    for kw in (dict(max_interval=0), dict(gap=-1)):
        with pytest.raises(ValueError):
            M.targets([], REFS, **kw)


# ---- the crafted realignment cases: (targets, events) as measured with this definition
EXPECT = {"clips": (3, 13), "early_indel": (2, 14), "homopolymer": (2, 18), "contig_start": (2, 10), "contig_end": (2, 18),
          "irregular_insert": (1, 19), "late_kept": (2, 2), "many_consensuses": (1, 144), "cap_2048": (1, 2048), "cap_2049": (1, 2049),
          "nine_ops": (3, 9), "five_op_newcigar": (2, 11), "mixed": (7, 32), "eq_x_ops": (1, 11)}


def _model_of_case(name, d):
    b = RC.build_case(name, d)
    h, refs, recs, offs = bamutil.read_bam(b.bam)
    return b, h, refs, recs, offs, M.targets_of_arena(recs, offs, refs)


def test_expectations_cover_every_case():
    assert set(EXPECT) == set(RC.CASES)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_model_targets_lie_inside_the_case_intervals(tmp_path, name):
    b, h, refs, recs, offs, res = _model_of_case(name, tmp_path)
    own = [(m.group(1), int(m.group(2)), int(m.group(3))) for m in re.finditer(r"(\S+):(\d+)-(\d+)\n", open(b.intervals).read())]
    assert (res.targets, res.events) == EXPECT[name]
    for rid, a, z, _ in rows(res):
        assert any(c == refs[rid][0] and lo <= a and z <= hi for c, lo, hi in own), (rid, a, z)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_model_targets_realign_to_the_same_bytes(built, tmp_path, name):
    b, meta, h, recs, offs = RC.load_case(name, tmp_path)
    refs = bamutil.read_bam(b.bam)[1]
    res = M.targets_of_arena(recs, offs[:-1], refs)
    iv = tmp_path / "model.intervals"
    iv.write_bytes(res.text)
    n = len(offs) - 1
    out0, oo0 = R.realign_cpu(h, recs, offs, n, b.fasta, b.intervals)
    out1, oo1 = R.realign_cpu(h, recs, offs, n, b.fasta, str(iv))
    assert list(oo0) == list(oo1) and bytes(out0[:int(oo0[-1])]) == bytes(out1[:int(oo1[-1])])
    assert bytes(out1[:int(oo1[-1])]) != bytes(recs[:int(offs[-1])])  # reads really are realigned
