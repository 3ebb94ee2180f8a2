"""CPU: the Python restatement of `openge calmd` (tests/calmd_model.py) against values that do not come from it --
the issue's hand-worked table, the MD and NM every directed row of tests/calmd_cases.py declares from its own
construction, and the NM the realigner stores in the reads it moves (pinned to the reference by the goldens of the
crafted realignment cases)."""
import struct

import numpy as np
import pytest

import bamutil
import calmd_cases as K
import calmd_model as M
import realign_cases as RC
import realign_util as RU


def tags_after(rb: bytes, ref: bytes, name="c"):
    out = M.calmd([rb], [(name, len(ref))], {name: ref}).records[0]
    t = M.tags_of(out)
    return t["MD"][1], t["NM"][1]


def test_hand_worked_table():
    ref = b"ACGTACGTAC"
    assert tags_after(bamutil.make_record("r1", 0, 0, 0, "10M", "ACGTTCGTAC"), ref) == (b"4A5", 1)
    ref = b"ACGTACGT"
    assert tags_after(bamutil.make_record("r2", 0, 0, 0, "3M2D3M", "ACGCGT"), ref) == (b"3^TA3", 2)
    assert tags_after(bamutil.make_record("r3", 0, 0, 0, "3M2D3M", "ACGAGT"), ref) == (b"3^TA0C2", 3)
    ref = b"ACGTACGTAC"
    assert tags_after(bamutil.make_record("r4", 0, 0, 0, "10M", "CCGTACGTAA"), ref)[0] == b"0A8C0"
    assert tags_after(bamutil.make_record("r5", 0, 0, 0, "3M1I3M", "ACGGTAC"), ref) == (b"6", 1)


@pytest.mark.parametrize("name", list(K.rows()))
def test_rows_give_their_declared_tags(name):
    rb, md, nm = K.rows()[name]
    out = M.calmd([rb], K.REFS, K.REFERENCE)
    t = M.tags_of(out.records[0])
    assert (t["MD"], t["NM"][1]) == (("Z", md), nm)
    assert t["NM"][0] == ("C" if nm < 256 else "S" if nm < 65536 else "I")
    assert out.counters() == {"records": 1, "skipped": 0, "no_reference": 0, "nm_changed": 1, "md_changed": 1,
                              "bytes_out": len(rb) + 3 + (1 if nm < 256 else 2 if nm < 65536 else 4) + 3 + len(md) + 1}
    # nothing but the appended tags and block_size differs
    new = out.records[0]
    assert new[4:len(rb)] == rb[4:] and struct.unpack_from("<I", new)[0] == len(new) - 4


@pytest.mark.parametrize("name", list(K.tag_states()))
def test_tag_states(name):
    rb, nm_changed, md_changed = K.tag_states()[name]
    out = M.calmd([rb], K.REFS, K.REFERENCE)
    new = out.records[0]
    assert (out.nm_changed, out.md_changed) == (nm_changed, md_changed)
    t = M.tags_of(new)
    assert t["NM"][1] == 1 and t["MD"] == ("Z", K.T_MD.encode())
    if not nm_changed and not md_changed:
        assert new == rb
    tail = (b"NMC\1" if nm_changed else b"") + (K.md_tag(K.T_MD) if md_changed else b"")
    assert new.endswith(tail) and struct.unpack_from("<I", new)[0] == len(new) - 4
    # every other tag is where it was, in order, byte for byte
    keep = lambda r: [r[a:b] for n, _, a, b in M.parse_tags(r, 36 + len(name) + 1 + 4 + 5 + 10)]
    old_tags, new_tags = keep(rb), keep(new)
    first = {}
    for tg in old_tags:
        first.setdefault(tg[:2], tg)
    gone = [first[k] for k, ch in ((b"NM", nm_changed), (b"MD", md_changed)) if ch and k in first]
    rest = [tg for tg in old_tags if not any(tg is g for g in gone)]
    assert new_tags[:len(rest)] == rest and b"".join(new_tags[len(rest):]) == tail


def test_pass_through_and_counters():
    records, refs, reference = K.cases()["pass_through"]
    out = M.calmd(records, refs, reference)
    assert out.records[:-1] == records[:-1] and out.records[-1] != records[-1]
    assert out.counters() == {"records": 7, "skipped": 5, "no_reference": 1, "nm_changed": 1, "md_changed": 1,
                              "bytes_out": sum(map(len, out.records))}


def test_limit_and_errors():
    records, refs, reference = K.cases()["limit_exact"]
    assert struct.unpack_from("<I", M.calmd(records, refs, reference).records[1])[0] == M.MAX_BLOCK_SIZE
    for name, (records, refs, reference, code, bad) in K.error_cases().items():
        with pytest.raises(M.CalmdError) as e:
            M.calmd(records, refs, reference)
        assert (e.value.code, e.value.record) == (code, bad), name
    # each fault on its own names its own reason
    why = {name: None for name in K.bad_records()}
    for name, rb in K.bad_records().items():
        with pytest.raises(M.CalmdError) as e:
            M.calmd([rb], K.REFS, K.REFERENCE)
        why[name] = e.value.why
    assert len(set(why.values())) == 6 and why["query_length"] != why["op_code_9"]


@pytest.mark.parametrize("name", list(K.cases()))
def test_idempotence(name):
    records, refs, reference = K.cases()[name]
    once = M.calmd(records, refs, reference)
    twice = M.calmd(once.records, refs, reference)
    assert twice.records == once.records and (twice.nm_changed, twice.md_changed) == (0, 0)
    assert (twice.skipped, twice.no_reference) == (once.skipped, once.no_reference)


def test_generated_cases_have_the_shapes_they_promise():
    c = K.cases()
    assert [len(c[f"n{n}"][0]) for n in (0, 1, 63, 64, 65, 1025)] == [0, 1, 63, 64, 65, 1025]
    out = M.calmd(*c["n1025"])
    assert 0 < out.nm_changed < 1025 and 0 < out.md_changed < 1025 and out.nm_changed != out.md_changed
    assert sum(a == b for a, b in zip(out.records, c["n1025"][0])) > 100  # reads whose tags were right stay


def test_fasta_loader_of_the_model(tmp_path):
    fa = K.write_fasta(tmp_path / "ref.fa")
    assert M.load_fasta(fa) == K.REFERENCE


@pytest.mark.parametrize("name", ["early_indel", "homopolymer", "contig_start", "late_kept", "mixed"])
def test_nm_equals_what_the_realigner_stores(name, tmp_path):
    """Independent of the model: the realigner rewrites NM of every read it moves (the tag was there: the crafted
    reads carry none, so the harness's output is asked for reads that carry OC), from its own mismatch count plus
    the indel lengths.  For those reads the model's nm is the stored NM."""
    b, meta, h, recs, offs = RC.load_case(name, tmp_path)
    # the crafted reads carry no NM: give every read one (wrong on purpose) so that the realigner rewrites it
    refs = bamutil.read_bam(b.bam)[1]
    records = [bamutil.rec_bytes(recs, o) for o in offs[:-1]]
    with_nm = [struct.pack("<I", len(r) - 4 + 7) + r[4:] + b"NMi" + struct.pack("<i", 77) for r in records]
    arena, aoffs = bamutil.pack_records(with_nm)
    out, oo = RU.realign_cpu(h, arena, aoffs, len(with_nm), b.fasta, b.intervals)
    reference = M.load_fasta(b.fasta)
    moved = kept = 0
    for o in oo[:-1]:
        rb = bamutil.rec_bytes(out, o)
        t = M.tags_of(rb)
        if "OC" not in t or "NM" not in t:
            continue
        moved += 1
        f = bamutil.fields(rb)
        ref = reference[refs[f["refid"]][0]]
        span = sum(w >> 4 for w in f["cigar"] if (w & 15) in (0, 2, 3, 7, 8))
        seq_at = 36 + len(f["name"]) + 1 + 4 * len(f["cigar"])
        codes = [(rb[seq_at + i // 2] >> 4) if i % 2 == 0 else (rb[seq_at + i // 2] & 15) for i in range(f["lseq"])]
        if not set(codes) <= {1, 2, 4, 8} or not set(ref[f["pos"]:f["pos"] + span]) <= set(b"ACGT") or f["pos"] + span > len(ref):
            continue
        kept += 1
        assert M.nm_md_of_record(rb, ref)[0] == t["NM"][1], (f["name"], f["cigar"])
        assert "MD" not in t  # the realigner removes it: what `calmd` is there to put back
    assert moved > 0 and kept >= 0.9 * moved, (moved, kept)
