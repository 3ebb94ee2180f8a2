"""CPU: the wide-layout sets of markdup_wide_cases.py against the oracle restatement of MarkDuplicates.

The GPU tests compare the device paths with the oracle on these sets; they only bite if the oracle itself
separates the twin groups and marks what each cluster was built to have marked.  That is checked here,
without a GPU: expected marks by construction, twins that change the marks when their keys are made to
collide, and clusters that each keep one record and mark another."""
import numpy as np
import pytest

import bamutil
import markdup_wide_cases as W
import oracle


def oracle_marks(records, header):
    """dup bytes in input order, from the oracle on the oracle-sorted stream"""
    recs, offs = bamutil.pack_records(records)
    n = len(records)
    perm = oracle.sort_perm(recs, offs, n)
    dup, nd = oracle.markdup(recs, offs[:-1][perm], n, header)
    d = np.empty(n, np.uint8)
    d[perm] = dup
    return d, nd


@pytest.fixture(scope="module", params=W.ACCEPTED)
def wset(request, built):
    s = W.get(request.param)
    return s, oracle_marks(s.records, s.header)


def test_layout_bits(built):
    """The table of the sets: sb + lb on either side of the 13-bit budget, as md_layout counts them."""
    got = {k: (W.get(k).sb, W.get(k).lb) for k in W.LAYOUTS}
    assert got == {"w12": (10, 2), "w13a": (11, 2), "w13b": (10, 3), "w13c": (12, 1), "w14a": (12, 2), "w14b": (11, 3)}
    for k, (n_ref, libs, ok) in W.LAYOUTS.items():
        s = W.get(k)
        assert (s.sb + s.lb <= 13) == ok and len(s.records) <= 4000
        if ok:
            assert W.top_ref_bit(n_ref) == 1 << (s.sb - 1)
        # the header resolves to the library ids the builder assumed
        from openge_amd import lib as L
        opts, keep = L.markdup_opts_from_header(s.header, s.n_ref)
        assert max([opts.unknown_lib] + keep[1][:opts.n_rg].tolist()) == s.max_lib == libs + 1


def test_records_sit_where_the_fields_end(wset):
    s, _ = wset
    mid, hi = 1 << (s.sb - 1), s.n_ref - 1
    seen = {bamutil.fields(r)["refid"] for r in s.records}
    assert {0, 1, mid - 1, mid, s.n_ref - 2, hi, -1} <= seen
    pos = [bamutil.fields(r)["pos"] for r in s.records if bamutil.fields(r)["refid"] == hi]
    assert max(pos) >= W.BIG - W.RL and min(pos) == 0


def test_oracle_equals_construction(wset):
    s, (d, nd) = wset
    exp = np.array(s.expect, np.uint8)
    bad = np.nonzero(d != exp)[0]
    assert not len(bad), [(bamutil.fields(s.records[i])["name"], int(d[i])) for i in bad]
    assert nd == int(exp.sum())
    # input order gives the same marks (distinct scores: no tie falls to the record order)
    recs, offs = bamutil.pack_records(s.records)
    du, _ = oracle.markdup(recs, offs, len(s.records), s.header)
    assert np.array_equal(du, exp)


def test_twins_collide_changes_marks(wset):
    s, (d, nd) = wset
    fields = {t["field"] for t in s.twins}
    assert {"ref", "ref1", "ref2", "orient"} <= fields and (("lib" in fields) == (s.max_lib > 1))
    for t in s.twins:
        assert t["patch"] and all(p for _, p in t["patch"])
        d2, nd2 = oracle_marks(W.apply_twin(s.records, t), s.header)
        assert not np.array_equal(d2, d) and nd2 > nd, t["name"]


def test_every_cluster_marks_and_keeps(wset):
    s, (d, _) = wset
    assert len(s.clusters) >= 30
    for name, idx in s.clusters.items():
        assert d[idx].max() == 1 and d[idx].min() == 0, name
