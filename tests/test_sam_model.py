"""CPU: the Python restatement of the SAM and FASTQ text (tests/sam_model.py) reproduces every fixture recorded
from the reference (tests/golden/view/manifest.json, tests/golden/make_view_goldens.py) byte for byte: every
crafted case the reference defines, simple.bam and 208.yhet.bam, the filtered runs and the FASTQ runs."""
import hashlib
import json

import pytest

import bamutil
import sam_cases as K
import sam_model as M
from goldens import GOLDEN

MANIFEST = json.loads((GOLDEN / "view" / "manifest.json").read_text())
FILES = {"simple": "simple.bam", "yhet208": "208.yhet.bam"}
CASES = K.sam_cases()


def same(blob: dict, data: bytes) -> bool:
    """A recorded blob (latin-1 text, or SHA-256 and length) against bytes."""
    if "text" in blob:
        return blob["text"].encode("latin-1") == data
    return blob["bytes"] == len(data) and blob["sha256"] == hashlib.sha256(data).hexdigest()


def file_records(name):
    """(refs, the file's records as byte strings)"""
    _t, refs, recs, offs = bamutil.read_bam(GOLDEN / "inputs" / FILES[name])
    return refs, M.split_records(recs, offs)


def sam_input(name):
    return file_records(name) if name in FILES else (K.REFS, CASES[name])


def test_every_crafted_case_the_reference_defines_is_recorded():
    want = {k for k, v in CASES.items() if v and K.defined_by_reference(v)} | set(FILES)
    assert set(MANIFEST["sam"]) == want
    assert not {"arrays", "mix", "seq"} & want and {"floats", "mix_ref", "seq_short", "tags", "cigar"} <= want
    assert set(MANIFEST["fastq"]) == {"crafted"} | set(FILES)


@pytest.mark.parametrize("name", sorted(MANIFEST["sam"]))
def test_sam_text_equals_the_reference(name):
    refs, records = sam_input(name)
    kept = M.filter_keep(records)  # the chain's Filter drops reads without bases (len > trim total, filter.cpp:202)
    assert len(kept) == len(records) - sum(M.parse(r)["lseq"] == 0 for r in records)
    body = b"".join(M.lines(kept, [n for n, _ in refs]))
    assert same(MANIFEST["sam"][name]["body"], body), body[:300]


@pytest.mark.parametrize("name,key", [(n, k) for n in sorted(MANIFEST["filters"]) for k in sorted(MANIFEST["filters"][n])])
def test_filtered_sam_text_equals_the_reference(name, key):
    refs, records = file_records(name)
    g = MANIFEST["filters"][name][key]
    kept = M.filter_keep(records, **M.filter_args(g["args"], refs))
    assert 0 < len(kept) and (len(kept) < len(records) or key == "r_contig"), (key, len(kept))
    assert same(g["body"], b"".join(M.lines(kept, [n for n, _ in refs])))
    assert g["header"] == MANIFEST["sam"][name]["header"]


@pytest.mark.parametrize("name", sorted(MANIFEST["fastq"]))
def test_fastq_text_equals_the_reference(name):
    """Recorded without a trim window only: under -B / -E the reference's QUAL is not a function of the record."""
    _refs, records = (K.REFS, K.fastq_records()) if name == "crafted" else file_records(name)
    kept = M.filter_keep(records)
    assert same(MANIFEST["fastq"][name], b"".join(M.lines(kept, [], "fastq")))


@pytest.mark.parametrize("trim", K.TRIMS)
def test_trimmed_fastq_entries_are_well_formed(trim):
    for r in K.fastq_records() + K.seq_records(K.SEQ_LENS):
        p = M.parse(r)
        _at, seq, _plus, qual, _end = M.fastq_entry(r, *trim).split(b"\n") if b"\n" not in p["name"] + M.quals(p["qual"], 0, p["lseq"]) else [b""] * 5
        assert len(seq) == len(qual) == (max(p["lseq"] - sum(trim), 0) if b"\n" not in p["name"] + M.quals(p["qual"], 0, p["lseq"]) else 0)
        if len(seq):
            assert seq == M.bases(p["seq"], 0, p["lseq"])[trim[0]:p["lseq"] - trim[1]]


def test_lines_quoted_in_the_design():
    refs, records = file_records("simple")
    line = M.sam_line(records[0], [n for n, _ in refs])
    assert line.startswith(b"USI-EAS376_6_PE1_FC30C59AAXX:1:76:66:953\t")
    assert M.fastq_entry(records[0], 3, 4).split(b"\n")[1] == b"CATTCATGTTGTTGCTCTTGCTTTGATTCCGACTTCTAACGTTTAACCTGTGATCAGACGCTTGACTG"
    assert len(M.fastq_entry(records[0], 3, 4).split(b"\n")[3]) == 68  # the reference writes 61 qualities under these 68 bases


def test_host_path_is_taken_only_for_printed_f_and_b_tags():
    assert [M.needs_host(r) for r in K.tag_records()] == [False] * len(K.tag_records())  # the f behind the NUL is not printed
    assert all(M.needs_host(r) for r in K.float_records() + K.array_records())
    assert sum(M.needs_host(r) for r in CASES["mix"]) == 60
