"""CPU: tests/samin_model.py (SAM line -> BAM record) against the reference's own records
(tests/golden/samin/manifest.json, recorded by tests/golden/make_samin_goldens.py) and as the exact inverse of
tests/sam_model.py, the reference-pinned BAM -> SAM, on the two real files."""
import hashlib
import json
from pathlib import Path

import pytest

import bamutil
import sam_model
import samin_cases as K
import samin_model as M

GOLDEN = Path(__file__).resolve().parent / "golden"
MANIFEST = json.loads((GOLDEN / "samin" / "manifest.json").read_text())
TEXTS = dict(K.reference_subset(), simple_sam=(GOLDEN / "inputs" / "simple.sam").read_bytes())


def test_the_manifest_covers_every_case_the_reference_defines():
    assert sorted(MANIFEST) == sorted(TEXTS)


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_model_equals_the_reference_records(name):
    recs, _, hosts = M.parse_text(TEXTS[name])
    got = b"".join(recs)
    want = MANIFEST[name]["records"]
    assert len(recs) == MANIFEST[name]["n"] and not any(hosts)
    if "hex" in want:
        assert got.hex() == want["hex"]
    else:
        assert (len(got), hashlib.sha256(got).hexdigest()) == (want["bytes"], want["sha256"])


@pytest.mark.parametrize("fn", ["simple.bam", "208.yhet.bam"])
def test_model_inverts_the_sam_text_of_the_real_files(fn):
    """samin_model(sam_model(records)) == records, bin, tag types and order included."""
    _, refs, recs, offs = bamutil.read_bam(GOLDEN / "inputs" / fn)
    records = sam_model.split_records(recs, offs)
    names = [n for n, _ in refs]
    for i, r in enumerate(records):
        back, warn, host = M.parse_line(sam_model.sam_line(r, names)[:-1], names)
        assert back == r, f"record {i}"
        assert not warn and not host


def test_simple_sam_is_simple_bam():
    _, refs, recs, offs = bamutil.read_bam(GOLDEN / "inputs" / "simple.bam")
    got, warns, hosts = M.parse_text(TEXTS["simple_sam"])
    assert got == sam_model.split_records(recs, offs) and not any(warns) and not any(hosts)
    assert M.contigs(M.split_text(TEXTS["simple_sam"])[0]) == [n for n, _ in refs]


def test_line_index_and_header_split():
    t = K.cases()["no_trailing_newline"]
    off = M.line_offsets(t)
    assert off[0] == len(K.header()) and off[-1] == len(t) + 1 and len(off) == 7
    assert M.line_offsets(K.header()) == [len(K.header())]
    assert M.line_offsets(b"") == [0]
    assert M.line_offsets(b"a\n\nb\n") == [0, 2, 3, 5]


@pytest.mark.parametrize("name", sorted(K.cases()))
def test_every_crafted_case_parses(name):
    recs, warns, hosts = M.parse_text(K.cases()[name])
    for r in recs:
        assert sam_model.parse(r)  # a well-formed record


def test_differences_from_the_reference():
    names = [n for n, _ in K.REFS]
    rec = lambda **kw: M.parse_line(K.line(**kw), names)[0]  # noqa: E731
    assert sam_model.parse(rec(seq="ACG", qual="*"))["qual"] == b"\xff\xff\xff"
    assert sam_model.parse(rec(seq="*", qual="*"))["lseq"] == 0
    assert rec(seq="acgtn") == rec(seq="ACGTN")
    assert rec(tags=("XI:i:2147483648",))[-7:] == b"XII\x00\x00\x00\x80"
    assert rec(tags=("XH:H:1AE3",))[-8:] == b"XHH1AE3\0"
    assert rec(tags=("XB:B:s,1,-1",))[-12:] == b"XBBs\x02\0\0\0\x01\0\xff\xff"
    assert sam_model.parse(rec(pos=0))["pos"] == -1 and rec(pos=0, cigar="*")[14:16] == (4680).to_bytes(2, "little")


@pytest.mark.parametrize("name", sorted(K.error_cases()))
def test_error_cases_name_line_and_field(name):
    text, line, field = K.error_cases()[name]
    with pytest.raises(M.BadLine) as e:
        M.parse_text(text)
    assert (e.value.line, e.value.field) == (line, field)
