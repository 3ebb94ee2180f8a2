"""CPU: the duplicate-set model (tests/dupsets_model.py) against hand-worked values, and the crafted cases
(tests/dupsets_cases.py) against what they say they build."""
import functools
import itertools

import pytest

import bamutil
import dupmetrics_model as DM
import dupsets_cases as K
import dupsets_model as M
from goldens import load_case


@pytest.mark.parametrize("name,want", [
    (b"a:1:10:10", None),                                  # 4 fields
    (b"a:1:10:11:12", (10, 11, 12)),                       # 5
    (b"a:b:1:10:10:10", None),                             # 6
    (b"a:b:c:d:1:20:30", (1, 20, 30)),                     # 7
    (b"a:b:c:d:e:1:10:10", None),                          # 8
    (b"USI-EAS376_6_PE1_FC30C59AAXX:1:76:66:953", (76, 66, 953)),
    (b"q:w:1:12#0/1:12abc", (1, 12, 12)),                  # junk behind the digits
    (b"e:r:1::14", (1, 0, 14)),                            # an empty field: no digit gives 0
    (b"t:y:-7:-3:9", (-7, -3, 9)),
    (b"t:y:1:-:+9", (1, 0, 0)),                            # a sign alone; '+' is no sign
    (b"t:y:1:--3:3-", (1, 0, 3)),
    (b"t:y:x1:007:123456789", (0, 7, 123456789)),
    (b"::::", (0, 0, 0)),
    (b"", None),
    (b"plain", None),
])
def test_name_parser(name, want):
    assert M.location(name) == want


def loc(*p):
    return [(True, (0,) + q) for q in p]


def test_chain_counts_components_in_every_order():
    a, b, c = (5, 1000, 1000), (5, 1100, 1000), (5, 1200, 1000)
    for order in itertools.permutations((a, b, c)):
        assert M.set_optical(loc(*order), True, 100) == (3, 2)     # A-C are 200 apart, joined through B
        assert M.set_optical(loc(*order), True, 99) == (3, 0)
    assert M.set_optical(loc(a, c), True, 100) == (2, 0)


def test_distance_d_and_d_plus_1():
    a, b = (1, 0, 0), (1, 101, -101)
    assert M.set_optical(loc(a, b), False, 100) == (2, 0)
    assert M.set_optical(loc(a, b), False, 101) == (2, 1)
    assert M.set_optical(loc(a, (1, 101, 0)), False, 100) == (2, 0)   # |dx| alone is enough to be apart
    assert M.set_optical(loc(a, (1, 0, 101)), False, 100) == (2, 0)
    assert M.set_optical(loc(a, a, a), False, 0) == (3, 2)


def test_parts_tiles_and_read_groups():
    a = (1, 10, 10)
    two_parts = [(True, (0,) + a), (False, (0,) + a), (True, (0,) + a)]
    assert M.set_optical(two_parts, True, 100) == (3, 1)    # FR / RF: divided by 0x40
    assert M.set_optical(two_parts, False, 100) == (3, 2)   # FF / RR: not divided
    assert M.set_optical([(True, (0,) + a), (True, (1,) + a)], False, 100) == (2, 0)           # two read groups
    assert M.set_optical([(True, (-1,) + a), (True, (-1,) + a)], False, 100) == (2, 1)         # none and none
    assert M.set_optical([(True, (0, 1, 10, 10)), (True, (0, 2, 10, 10))], False, 100) == (2, 0)   # two tiles
    assert M.set_optical([(True, None), (True, (0,) + a), (True, None), (True, (0,) + a)], False, 100) == (2, 1)
    assert M.set_optical([(True, None)], True, 100) == (0, 0)


@functools.lru_cache(maxsize=None)
def computed(name, D):
    header, records, _ = K.cases()[name]
    recs, offs = bamutil.pack_records(records)
    return M.compute(recs, offs[:-1], header, D)


def bins(h):
    return {k: v for k, v in enumerate(h) if v}


def test_crafted_cases_build_what_they_say():
    per_lib, hist = computed("n0", 100)
    assert not any(any(r) for r in per_lib) and not any(any(h) for h in hist)
    assert computed("no_pairs", 100) == computed("n0", 100)
    per_lib, hist = computed("sizes_small", 100)
    assert bins(hist[0]) == {1: 2, 2: 1, 3: 1, 63: 1, 64: 1, 65: 1} and per_lib[1][:2] == [199, 7]
    assert sum(r[3] for r in per_lib) > 0
    for name, size in (("block_m1", K.BLOCK_CAP - 1), ("block", K.BLOCK_CAP), ("block_p1", K.BLOCK_CAP + 1)):
        per_lib, hist = computed(name, 100)
        assert hist[0][min(size, M.BINS - 1)] == 1 and 0 < per_lib[1][3] < per_lib[1][2]
    per_lib, hist = computed("chain", 100)
    assert per_lib[1] == [18, 6, 18, 12] and bins(hist[1]) == {3: 6} and bins(hist[2]) == {1: 6}
    assert computed("chain", 101) == computed("chain", 100) and computed("chain", 99)[0][1] == [18, 6, 18, 0]
    per_lib, hist = computed("twos33", 100)
    assert per_lib[1] == [66, 33, 66, 22] and bins(hist[0]) == {2: 33}   # dx 0 and 60 are close, 120 is not
    per_lib, hist = computed("libs_rgs_tiles", 100)
    # libA: {a1 x 2}: 1; {a1 x 4, a2 x 2}: 3 + 1; the four tiles: 0; the unknown library: one set of four: 3.  libB: 1
    assert [r[3] for r in per_lib[1:]] == [5, 1, 3] and [r[1] for r in per_lib[1:]] == [3, 1, 1]
    per_lib, hist = computed("orientations_contigs", 100)
    # FR 1 (the second-first member is a part of its own), FF 2, RR 2, RF 1, two contigs 3, chrB 1
    assert per_lib[1][3] == 10 and per_lib[1][1] == 6
    # the set of five: two equal to the first, then all; the set of three: 90 apart in x, 90 apart in y
    assert [computed("d0", D)[0][1][3] for D in (0, 1, 90)] == [2, 4, 4 + 2]
    per_lib, hist = computed("names", 100)
    # 5 + 2 + 1 + 1 + 10 pairs; 2 located in the first set; of the ten names those of 5 and 7 fields: 7
    assert per_lib[1][:3] == [19, 5, 9]
    assert computed("mixed", 100) == computed("mixed_shuffled", 100)


def test_identity_and_figures_on_the_reference_file():
    """yhet208: pairs - sets equals section 26's READ_PAIR_DUPLICATES of the reference's own flags; the figures the
    issue quotes for the file (6,950 pairs in 3,819 sets of sizes 1 to 12; with read groups ignored 13 optical
    duplicates at distance 100 and 48 at 2500)."""
    case = load_case("yhet208")
    rg_lib, unknown, names = DM.lib_table(case.header)
    dup_at = set(int(i) for i in case.arrays["dedup_input_v"])
    marked = []
    for i, rb in enumerate(DM.records_of_arena(case.recs, case.offs[:-1])):
        b = bytearray(rb)
        b[19] = (b[19] & ~0x04 & 0xFF) | (0x04 if i in dup_at else 0)
        marked.append(bytes(b))
    counts = DM.count(marked, rg_lib, unknown, len(names))
    per_lib, hist = M.compute(case.recs, case.offs[:-1], case.header, 100)
    assert [r[0] - r[1] for r in per_lib] == [c[5] // 2 for c in counts]
    assert sum(r[0] for r in per_lib) == 6950 and sum(r[1] for r in per_lib) == 3819 and sum(r[0] - r[1] for r in per_lib) == 3131
    assert min(bins(hist[0])) == 1 and max(bins(hist[0])) == 12 and sum(k * v for k, v in bins(hist[0]).items()) == 6950
    assert sum(r[3] for r in M.compute(case.recs, case.offs[:-1], case.header, 100, ignore_rg=True)[0]) == 13
    assert sum(r[3] for r in M.compute(case.recs, case.offs[:-1], case.header, 2500, ignore_rg=True)[0]) == 48
    assert sum(r[3] for r in per_lib) > 0


def test_text_layout():
    hist = [[0] * M.BINS for _ in range(3)]
    hist[0][1], hist[0][3], hist[1][2], hist[2][1], hist[2][2] = 5, 1, 1, 5, 1
    one = M.text([("lib", [0, 20, 0, 0, 0, 4], [8, 6, 3, 1])], hist, "cmd").decode().split("\n")
    assert one[5].split("\t")[6:8] == ["2", "1"] and one[5].split("\t")[9] == str(DM.estimate_library_size(9, 8))
    assert one[7] == "## HISTOGRAM\tjava.lang.Double" and one[8] == "BIN\tCoverageMult\tall_sets\toptical_sets\tnon_optical_sets"
    assert one[9].startswith("1.0\t") and one[9].endswith("\t5\t0\t5") and one[11].endswith("\t1\t0\t0") and one[108].startswith("100.0\t")
    assert one[109:] == ["", ""]
    two = M.text([("b", [0, 20, 0, 0, 0, 4], [8, 6, 3, 1]), ("a", [0] * 6, [0] * 4)], hist, "cmd").decode().split("\n")
    assert two[9] == "BIN\tall_sets\toptical_sets\tnon_optical_sets" and two[10:] == ["1.0\t5\t0\t5", "2.0\t0\t1\t1", "3.0\t1\t0\t0", "", ""]
    none = M.text([], [[0] * M.BINS] * 3, "cmd").decode().split("\n")
    assert none[5:] == ["", "## HISTOGRAM\tjava.lang.Double", "BIN\tall_sets\toptical_sets\tnon_optical_sets", "", ""]


# ------------------------------------------------------------------------------------------- the host text (no GPU)
def hist_of(all_sets, optical_sets, non_optical_sets):
    h = [[0] * M.BINS for _ in range(3)]
    for col, d in enumerate((all_sets, optical_sets, non_optical_sets)):
        for k, v in d.items():
            h[col][k] = v
    return h


HOST_TEXT = {
    "none": ([], hist_of({}, {}, {})),
    "one_with_estimate": ([("libA", [10, 2000, 3, 4, 1, 200], [1000, 900, 40, 13])], hist_of({1: 850, 3: 50}, {2: 13}, {1: 850, 2: 13, 3: 37})),
    "one_past_bin_100": ([("libA", [10, 2000, 3, 4, 1, 200], [1000, 900, 40, 13])], hist_of({1: 1, 130: 2, 1023: 1}, {1023: 1}, {1: 4})),
    "one_no_duplicates": ([("libA", [10, 2000, 3, 4, 1, 0], [1000, 1000, 0, 0])], hist_of({1: 1000}, {}, {1: 1000})),
    "one_all_optical": ([("libA", [0, 200, 0, 0, 0, 100], [100, 50, 100, 50])], hist_of({2: 50}, {2: 50}, {1: 50})),      # n - o == c: no estimate
    "one_more_optical_than_pairs": ([("libA", [0, 20, 0, 0, 0, 10], [10, 5, 10, 11])], hist_of({2: 5}, {}, {2: 5})),
    "two": ([("zeta", [5, 40, 0, 1, 2, 6], [20, 17, 3, 1]), ("Alpha", [0, 2000, 7, 9, 0, 200], [1000, 900, 0, 0])], hist_of({1: 7, 2: 3}, {2: 1}, {1: 8, 2: 2})),
}


def test_host_symbols_are_exported(built):
    from openge_amd import lib as L
    names = L.exported_symbols()
    for s in ("oge_dup_sets_dev", "oge_dup_sets", "oge_bam_dup_sets_dev", "oge_dup_sets_text"):
        assert s in names and hasattr(L.lib(), s), s


@pytest.mark.parametrize("name", list(HOST_TEXT))
def test_host_text_equals_the_model_byte_for_byte(built, name):
    from openge_amd import lib as L
    rows, hist = HOST_TEXT[name]
    got, want = L.dup_sets_text(rows, hist, "openge dupmetrics --optical-distance 100 in.bam"), M.text(rows, hist, "openge dupmetrics --optical-distance 100 in.bam")
    assert got == want
    lines = got.decode().split("\n")
    k = lines.index("## HISTOGRAM\tjava.lang.Double")
    roi = name in ("one_with_estimate", "one_past_bin_100")
    assert lines[k + 1] == ("BIN\tCoverageMult\tall_sets\toptical_sets\tnon_optical_sets" if roi else "BIN\tall_sets\toptical_sets\tnon_optical_sets")
    top = {"none": 0, "one_with_estimate": 100, "one_past_bin_100": 1023, "one_no_duplicates": 1, "one_all_optical": 2, "one_more_optical_than_pairs": 2, "two": 2}[name]
    assert lines[k + 2 + top:] == ["", ""] and all(lines[k + 1 + b].startswith("%d.0\t" % b) for b in range(1, top + 1))
    if name == "one_with_estimate":   # the optical duplicates leave the estimate's first argument
        row = lines[5].split("\t")
        assert row[7] == "13" and row[9] == str(DM.estimate_library_size(1000 - 13, 900)) != str(DM.estimate_library_size(1000, 900))
