"""CPU: the host pieces of the duplication metrics (host_capi.cpp: oge_estimate_library_size, oge_dup_metrics_text)
against the model (tests/dupmetrics_model.py): exact equality -- the same doubles in the same order, the same libm.
No GPU: the functions touch no device.  Without the feature the symbols do not exist and every test here fails."""
import random

import pytest

import dupmetrics_model as M
from openge_amd import lib as L

FIXED = [(0, 0), (1, 1), (12345, 12345), (2, 1), (10, 9), (10 ** 6, 999_999), (10 ** 9, 10 ** 9 // 2), (10 ** 9, 1)]


def sweep():
    rnd = random.Random(20261021)
    out = []
    for _ in range(1000):
        n = int(10 ** rnd.uniform(0, 10))
        unique = int(n * rnd.random() ** rnd.choice((0.2, 1, 5)))
        out.append((n, max(1, min(n, unique))))
    return out


def test_symbols_are_exported(built):
    names = L.exported_symbols()
    for s in ("oge_dup_metrics_dev", "oge_dup_metrics", "oge_bam_dup_metrics_dev", "oge_estimate_library_size", "oge_dup_metrics_text"):
        assert s in names and hasattr(L.lib(), s), s


def test_estimate_equals_the_model_exactly(built):
    """(0, 0), (n, n), (2, 1), (10, 9), (10^6, 999 999), (10^9, 10^9 / 2), (10^9, 1) and a seeded sweep of 1000
    pairs; for every estimate c <= L and f(L) >= f(L + 1)."""
    some = 0
    for n, c in FIXED + sweep():
        got, want = L.estimate_library_size(n, c), M.estimate_library_size(n, c)
        assert got == want, (n, c, got, want)
        if n == c or n == 0:
            assert got is None
        if got is not None:
            some += 1
            assert c <= got, (n, c, got)
            assert M.f_at(n, c, float(got)) >= M.f_at(n, c, float(got + 1)), (n, c, got)
    assert some > 900
    assert L.estimate_library_size(10, 9) is not None and L.estimate_library_size(3, 4) is None  # more unique pairs than pairs


ONE = [("libA", [10, 2000, 3, 4, 1, 200])]
THREE = [("zeta", [5, 40, 0, 1, 2, 6]), ("Alpha", [0, 0, 7, 9, 0, 0]), ("mid dle", [123456789, 9876543210, 5, 6, 7654321, 1234567890])]
TEXT_CASES = {
    "zero_libraries": [],
    "one_with_estimate": ONE,                                     # with the histogram
    "one_without_estimate": [("libA", [10, 2000, 3, 4, 1, 0])],   # no duplicate pair: no estimate, no histogram
    "one_unpaired_only": [("solo", [9, 0, 0, 0, 3, 0])],
    "one_odd_pair_counts": [("odd", [0, 2001, 0, 0, 0, 201])],
    "one_all_pairs_duplicate": [("none unique", [0, 2, 0, 0, 0, 2])],   # an estimate of 0: no histogram
    "three": THREE,
    "byte_order": [(n, [k, 2 * k, 0, 0, 0, 0]) for k, n in enumerate(("b", "B", "a", "_", "Z", "é", "a b", "aB", "Unknown Library"))],
}


@pytest.mark.parametrize("name", list(TEXT_CASES))
def test_text_equals_the_model_byte_for_byte(built, name):
    rows = TEXT_CASES[name]
    cl = "openge dedup --metrics m.txt in.bam -o out.bam"
    got, want = L.dup_metrics_text(rows, cl), M.text(rows, cl)
    assert got == want
    parsed = M.parse(got)
    assert parsed[0] == cl and len(parsed[1]) == len(rows)
    assert (len(parsed[2]) == 100) == (name in ("one_with_estimate", "one_odd_pair_counts"))
    assert M.same_rows(parsed[1], M.parse(want)[1])  # integers exactly, the float field at 1e-6 absolute
    if name == "byte_order":
        order = [r["LIBRARY"] for r in parsed[1]]
        assert order == sorted(order, key=str.encode) and order != sorted(order, key=str.lower)


def test_size_query_convention(built):
    """The length comes back whatever the buffer; a buffer one byte short of text + NUL gets the text cut by one byte."""
    want = M.text(THREE, "x")
    assert L.dup_metrics_text(THREE, "x") == want
    assert L.dup_metrics_text(THREE, "x", cap=len(want)) == want[:-1]
    assert L.dup_metrics_text(THREE, "x", cap=1) == b"" and L.dup_metrics_text(THREE, "x", cap=0) == b""
    assert L.dup_metrics_text(THREE, "x", cap=len(want) + 100) == want
