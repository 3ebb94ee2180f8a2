"""CPU: the Python restatement of stats / coverage (tests/qc_model.py) reproduces every fixture recorded from
the reference (tests/golden/qc/manifest.json, tests/golden/make_qc_goldens.py) byte for byte; the serial and the
local form of `Sorted` agree; the closed-form per-bin overlap equals the per-position brute force."""
import hashlib
import json
import random

import numpy as np
import pytest

import bamutil
import qc_cases as K
import qc_model as M
from goldens import GOLDEN

MANIFEST = json.loads((GOLDEN / "qc" / "manifest.json").read_text())
FILES = {"simple": "simple.bam", "yhet208": "208.yhet.bam"}


def same(blob: dict, data: bytes) -> bool:
    """A recorded blob (text, or SHA-256 and length) against bytes."""
    if "text" in blob:
        return blob["text"].encode() == data
    return blob["bytes"] == len(data) and blob["sha256"] == hashlib.sha256(data).hexdigest()


def file_case(name):
    _t, refs, recs, offs = bamutil.read_bam(GOLDEN / "inputs" / FILES[name])
    return refs, np.concatenate([recs, np.zeros(16, np.uint8)]), offs


def stats_input(name):
    if name in FILES:
        return file_case(name)
    refs, records = K.stats_cases()[name]
    return (refs, *K.pack(records))


def coverage_input(name):
    if name in FILES:
        return file_case(name)
    refs, records, _d = K.coverage_cases()[name]
    return (refs, *K.pack(records))


def test_the_fast_record_builder_is_make_record():
    assert K.rec(3, 0, 5, flag=0x41, lseq=5, tlen=-7) == bamutil.make_record("r3", 0x41, 0, 5, "", "=====", tlen=-7)


def test_every_crafted_stats_case_defined_by_the_reference_is_recorded():
    want = {k for k, (_r, recs) in K.stats_cases().items() if recs} - {"ins_max", "len_big"} | set(FILES)
    assert set(MANIFEST["stats"]) == want
    assert set(MANIFEST["coverage"]) == {k for k, v in K.coverage_cases().items() if v[2]} | set(FILES)


@pytest.mark.parametrize("name", sorted(MANIFEST["stats"]))
def test_stats_text_equals_the_reference(name):
    _refs, recs, offs = stats_input(name)
    out, err = M.stats_text(M.stats(recs, offs), show_inserts=True, show_lengths=True)
    g = MANIFEST["stats"][name]
    assert same(g["stdout"], out.encode()), out
    assert same(g["stderr"], err.encode()), err


def test_reference_lines_quoted_in_the_design():
    _refs, recs, offs = file_case("yhet208")
    out, _ = M.stats_text(M.stats(recs, offs), show_inserts=True)
    assert "Mapped reads:           14812 ( 96.1%)\n" in out
    assert "    Mean:               218.7\n    Median:             189.0\n" in out
    refs, recs, offs = file_case("simple")
    g, v, sk = M.coverage_sparse(M.cores(recs, offs), [ln for _, ln in refs], 100)
    assert (g.tolist(), v.tolist(), sk, len(offs)) == ([0, 1, 2], [353, 333, 22], 0, 10)


@pytest.mark.parametrize("name", sorted(MANIFEST["coverage"]))
def test_coverage_text_equals_the_reference(name):
    refs, recs, offs = coverage_input(name)
    c, names, lens = M.cores(recs, offs), [n for n, _ in refs], [ln for _, ln in refs]
    for key, g in MANIFEST["coverage"][name].items():
        bs, mode = key.split("_")
        gb, v, sk = M.coverage_sparse(c, lens, int(bs))
        bins = M.dense(gb, v, int(M.coverage_layout(lens, int(bs))[-1]))
        tsv, err = M.coverage_text(names, lens, int(bs), bins, sk, omit_uncovered=mode == "nz")
        assert same(g["tsv"], tsv.encode()), (key, tsv[:300])
        assert same(g["stderr"], err.encode()), (key, err)


def test_sorted_cases_have_the_stated_answer_in_every_form():
    for name, (keys, want) in K.sorted_cases().items():
        r, p = [a for a, _ in keys], [b for _, b in keys]
        assert M.sorted_serial(r, p) == want, name
        assert M.sorted_local(r, p) == want, name
        assert M.sorted_local_exact(r, p) == want, name


def test_serial_and_local_sorted_forms_agree_on_random_sequences():
    """10,000 seeded sequences with unplaced records, refID runs of every length and few distinct positions, so
    that run starts, ties and violations are all common; both outcomes must occur often."""
    rng = random.Random(2024)
    yes = 0
    for _ in range(10_000):
        n, rid, keys = rng.randint(0, 14), rng.randint(0, 2), []
        for _i in range(n):
            u = rng.random()
            if u < 0.2:
                keys.append(rng.choice(((-1, -1), (rid, -1), (-1, rng.randint(0, 5)))))
                continue
            if u < 0.45:
                rid += rng.choice((1, 1, 1, -1))
                rid = max(rid, 0)
            keys.append((rid, rng.randint(0, 4) if rng.random() < 0.5 else (keys[-1][1] + 1 if keys and keys[-1][1] >= 0 else 0)))
        r, p = [a for a, _ in keys], [b for _, b in keys]
        s = M.sorted_serial(r, p)
        assert M.sorted_local(r, p) == s and M.sorted_local_exact(r, p) == s, keys
        yes += s
    assert 1500 < yes < 8500, yes


def test_exact_local_form_equals_the_serial_one_on_any_int32():
    """refID below -1 and positions below -1 included (invalid BAM; the kernel still answers as the reference)."""
    rng = random.Random(7)
    for _ in range(5000):
        keys = [(rng.randint(-3, 2), rng.choice((-7, -2, -1, 0, 1, 5, 2**31 - 1, -2**31))) for _i in range(rng.randint(0, 8))]
        r, p = [a for a, _ in keys], [b for _, b in keys]
        assert M.sorted_local_exact(r, p) == M.sorted_serial(r, p), keys


@pytest.mark.parametrize("binsize", K.BINSIZES)
def test_closed_form_overlap_equals_brute_force(binsize):
    for name, (refs, records, _d) in K.coverage_cases().items():
        if binsize == 1 and name in ("contention", "unsorted_wide", "sorted_window"):
            records = records[::37]  # the per-position loop is slow; every shape is still there
        c, lens = M.cores(*K.pack(records)), [ln for _, ln in refs]
        g, v, sk = M.coverage_sparse(c, lens, binsize)
        bins, sk2 = M.coverage_brute(c, lens, binsize)
        assert sk == sk2 and dict(zip(g.tolist(), v.tolist())) == bins, name
    rng = random.Random(binsize)  # random reads around both ends of a short contig
    lens = [rng.randint(1, 400), rng.randint(1, 400)]
    c = {"refid": np.array([rng.randint(-1, 1) for _ in range(300)]), "pos": np.array([rng.randint(-30, 420) for _ in range(300)]),
         "lseq": np.array([rng.randint(0, 120) for _ in range(300)])}
    g, v, sk = M.coverage_sparse(c, lens, min(binsize, 50))
    bins, sk2 = M.coverage_brute(c, lens, min(binsize, 50))
    assert sk == sk2 and dict(zip(g.tolist(), v.tolist())) == bins


def test_insert_edges_sit_on_the_radix_digits():
    ins = M.stats(*K.pack(K.insert_cases()["ins_max"][1]))
    assert (ins["n_insert"], ins["insert_mid_lo"], ins["insert_mid_hi"]) == (5, 2**31 - 1, 2**31 - 1)
    assert ins["insert_sum"] == 2 * 2**31 + 2 * 2**31 - 3 + 5
    for m in range(5):
        assert M.stats(*K.pack(K.insert_cases()[f"ins_n{m}"][1]))["n_insert"] == m
