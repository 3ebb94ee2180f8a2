"""CPU: the Python restatement of `openge compare` (tests/compare_model.py) reproduces every run recorded from the
reference (tests/golden/compare/manifest.json, tests/golden/make_compare_goldens.py) byte for byte: stdout, stderr
and the exit status; and the properties the GPU tests rely on (the order of the type characters, region membership
by start position, counts that do not depend on the order of the records)."""
import functools
import json
import random

import numpy as np
import pytest

import bamutil
import compare_cases as K
import compare_model as M
import samin_model
from goldens import GOLDEN
from test_qc_model import same

MANIFEST = json.loads((GOLDEN / "compare" / "manifest.json").read_text())
CASES = K.cases()


@functools.lru_cache(maxsize=None)
def input_file(name: str):
    """(refs, recs, offs) of a file under tests/golden/inputs; SAM text through the SAM model"""
    path = GOLDEN / "inputs" / name
    if name.endswith(".sam"):
        text = path.read_bytes()
        header, _lines = samin_model.split_text(text)
        refs = []
        for ln in header.decode().splitlines():
            if ln.startswith("@SQ\t"):
                f = dict(x.split(":", 1) for x in ln.split("\t")[1:])
                refs.append((f["SN"], int(f["LN"])))
        records, _w, _h = samin_model.parse_text(text)
        return (refs, *K.pack(records))
    _t, refs, recs, offs = bamutil.read_bam(path)
    return refs, np.concatenate([recs, np.zeros(16, np.uint8)]), offs


@functools.lru_cache(maxsize=None)
def crafted(name: str):
    ra, rb, _regions = CASES[name]
    return K.pack(ra), K.pack(rb)


def model_run(entry: dict):
    args, regions, names = list(entry["args"]), [], []
    print_changes = False
    while args:
        a = args.pop(0)
        if a == "-r":
            regions.append(args.pop(0))
        elif a == "-p":
            print_changes = True
        else:
            names.append(a)
    if entry["dir"] == "inputs":
        refs = input_file(names[0])[0]
        files = [(n, *input_file(n)[1:]) for n in names]
    else:
        a, b = crafted(entry["dir"])
        refs, files = K.REFS, [("a.bam", *a), ("b.bam", *b)]
    return M.run(files, refs, regions, print_changes)


def test_every_crafted_case_is_recorded_with_and_without_print():
    for name, (_a, _b, regions) in CASES.items():
        for key in (f"case_{name}", f"case_{name}_print"):
            assert key in MANIFEST and MANIFEST[key]["dir"] == name
            assert [x for x in MANIFEST[key]["args"] if x not in ("-p", "-r", "a.bam", "b.bam")] == (regions or [])


@pytest.mark.parametrize("key", sorted(MANIFEST))
def test_model_text_equals_the_reference(key):
    g = MANIFEST[key]
    out, err, status = model_run(g)
    assert status == g["status"]
    assert same(g["stderr"], err.encode()), err
    assert same(g["stdout"], out.encode()), out[:2000]


def test_reference_lines_quoted_in_the_design():
    assert MANIFEST["simple_bam__208_bam"]["stdout"]["text"] == "\t   15409 added\t       0 removed\n"
    assert MANIFEST["three_region"]["stdout"]["text"] == "   YHet:0..300\t       5 added\t       0 removed\n"
    assert MANIFEST["three_region"]["stderr"]["text"] == "208.yhet.bam:\nsimple.sam:\n"
    assert MANIFEST["one_input"] == {"dir": "inputs", "args": ["simple.bam"], "stdout": {"text": ""}, "stderr": {"text": ""}, "status": 0}


def test_type_characters_order_as_ascii():
    ranked = sorted(M.TYPES, key=lambda t: M.order_key((0, 0, ((5, t),))))
    assert "".join(ranked) == "=DHIMNPSX"
    # the length decides before the type, the op count before both
    assert M.order_key((0, 0, ((4, "X"),))) < M.order_key((0, 0, ((5, "="),))) < M.order_key((0, 0, ((1, "="), (1, "="))))


def test_membership_is_the_start_position_with_both_ends():
    recs, offs = K.pack(K.recs_of([(0, 99, "500M", 1), (0, 100, "1M", 1), (0, 200, "1M", 1), (0, 201, "1M", 1), (-1, 150, "", 1), (0, -1, "", 1)]))
    assert [e[1] for e in M.elements(recs, offs, (0, 100, 0, 200))] == [100, 200]  # the read over 99..598 does not belong
    assert [e[1] for e in M.elements(recs, offs)] == [99, 100, 200, 201]           # refID -1 and pos -1 never do
    assert M.parse_region("chrA:100..200", K.REFS) == ((0, 100, 0, 200), "")
    assert M.parse_region("chrB", K.REFS) == ((1, 0, 1, 50000), "")
    assert M.parse_region("chrA:5-9", K.REFS) == ((0, 5, 0, 5), "")  # atoi stops at the '-'


def test_counts_are_multiset_counts_whatever_the_order():
    (ra, oa), (rb, ob) = crafted("ladder")
    a, b = M.elements(ra, oa), M.elements(rb, ob)
    want = M.compare(a, b)
    assert want["common"] + want["deletions"] == len(a) and want["common"] + want["additions"] == len(b)
    assert want["additions"] == len(want["adds"]) and want["deletions"] == len(want["dels"])
    rnd = random.Random(3)
    rnd.shuffle(a)
    rnd.shuffle(b)
    assert M.compare(a, b) == want
    back = M.compare(b, a)
    assert (back["additions"], back["deletions"], back["adds"], back["dels"]) == (want["deletions"], want["additions"], want["dels"], want["adds"])
    assert sum(n for *_x, n, _ops in M.diff_entries(want)) == want["additions"] + want["deletions"]
