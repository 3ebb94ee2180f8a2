"""GPU: `openge targets` computed on the device (csrc/targets.hip: oge_targets_dev, its host-buffer and whole-file
forms, the lib.py wrappers, the CLI command and `localrealign --auto-targets`) equals the Python restatement
(tests/targets_model.py) on every crafted case, and the computed intervals realign the crafted realignment cases to
the reference's records.

Neither the symbols, the command nor the flag exist before this feature: every test here fails without it."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import realign_cases as RC
import targets_cases as K
import targets_model as M
from openge_amd import lib as L
from test_gpu_cli import OPENGE

pytestmark = pytest.mark.gpu

CASES = K.cases()
COMBOS = [(mi, gap) for mi in K.MAX_INTERVALS for gap in K.GAPS]


def dev(recs: np.ndarray, offs: np.ndarray):
    """(device records, device offsets): keep both alive while the pointers are in use."""
    return torch.from_numpy(np.ascontiguousarray(recs)).cuda(), torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()).cuda()


@functools.lru_cache(maxsize=None)
def packed(name):
    records, refs = CASES[name]
    recs, offs = bamutil.pack_records(records)
    return recs, offs[:-1]


@functools.lru_cache(maxsize=None)
def bam_bytes(name) -> bytes:
    records, refs = CASES[name]
    return bamutil.bgzf_blocks(_bam_body(K.header_text(refs), refs, records))


def _bam_body(header_text, refs, records) -> bytes:
    import struct
    ht = header_text.encode()
    body = b"BAM\1" + struct.pack("<i", len(ht)) + ht + struct.pack("<i", len(refs))
    for name, ln in refs:
        nb = name.encode() + b"\0"
        body += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    return body + b"".join(records)


@functools.lru_cache(maxsize=None)
def model(name, mi, gap):
    records, refs = CASES[name]
    return M.targets(records, refs, max_interval=mi, gap=gap)


def check(got, want: M.Result, what):
    counters, arr, text = got
    assert counters == want.counters(), (what, counters, want.counters())
    assert arr.shape == want.array.shape and (arr == want.array).all(), what
    assert text == want.text, what


@pytest.mark.parametrize("name", list(CASES))
def test_targets_equal_the_model_in_every_form(ctx, name):
    """Empty input and reads without events, one event, events in the last record of a wave, a row and a tile and in
    the first of the next, 60 indels in one read and in every read of more than a tile, 70 ops, every filter bit,
    indels at the read ends, N and P, = and X anchors, an enclosing deletion, 3,000 copies of one event, a chain
    over the sort tile, widths 499 and 500, a contig change, a clipped stop, every decimal width, shuffled input:
    device records, host buffers and the whole file give the model's counters, intervals and text at gaps 0, 1
    and 10 and both maximal lengths."""
    records, refs = CASES[name]
    recs, offs = packed(name)
    d = dev(recs, offs)
    for mi, gap in COMBOS:
        want = model(name, mi, gap)
        check(ctx.targets_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), refs, mi, gap), want, (name, mi, gap, "dev"))
        assert ctx.counter("targets_events") == want.events
        check(ctx.targets(recs, offs, len(offs), refs, mi, gap), want, (name, mi, gap, "host"))
        check(ctx.bam_targets(bam_bytes(name), mi, gap), want, (name, mi, gap, "file"))
    assert ctx.last_refs()[0] == [n for n, _ in refs]


def test_geometry_counters_and_stage(ctx):
    recs, offs = packed("tile_edge")
    d = dev(recs, offs)
    ctx.targets_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), K.REFS)
    assert (ctx.counter("targets_tile_records"), ctx.counter("targets_merge_tile")) == (K.TILE_RECORDS, K.MERGE_TILE)
    assert ctx.timing("targets") > 0
    # the shapes straddle the real edges
    assert len(offs) > K.TILE_RECORDS and len(CASES["all_sixty"][0]) > K.TILE_RECORDS
    assert model("copies3000", 500, 0).events > 2 * K.MERGE_TILE and model("chain5000", 500, 0).events > K.SORT_TILE
    assert model("all_sixty", 500, 0).events == 60 * len(CASES["all_sixty"][0])


def test_input_order_does_not_matter(ctx):
    a, b = ctx.targets(*packed("mixed"), len(packed("mixed")[1]), K.REFS), ctx.targets(*packed("mixed_shuffled"), len(packed("mixed")[1]), K.REFS)
    assert a[0] == b[0] and (a[1] == b[1]).all() and a[2] == b[2]


@pytest.mark.parametrize("name", list(K.error_cases()))
def test_errors_name_the_record(ctx, name):
    records, refs, bad, kind = K.error_cases()[name]
    recs, offs = bamutil.pack_records(records)
    offs = offs[:-1]
    d = dev(recs, offs)
    if bad is None:
        check(ctx.targets_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), refs), M.targets(records, refs), name)
        return
    for call in (lambda: ctx.targets_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), refs), lambda: ctx.targets(recs, offs, len(offs), refs)):
        with pytest.raises(L.OgeError) as e:
            call()
        assert "error -1:" in str(e.value) and f"targets: record {bad} {M.BAD[kind]}" in str(e.value)


def test_options_are_refused(ctx):
    recs, offs = packed("one_event")
    for mi, gap in ((0, 0), (500, -1)):
        with pytest.raises(L.OgeError) as e:
            ctx.targets(recs, offs, len(offs), K.REFS, mi, gap)
        assert "error -1:" in str(e.value)


# ------------------------------------------------------------------------------------------------ the CLI
def cli(*args, stdin=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env=dict(os.environ), stdin=stdin)


def test_cli_prints_the_model_text_for_bam_and_sam(ctx, tmp_path):
    name = "mixed_shuffled"
    records, refs = CASES[name]
    bam, sam = tmp_path / "in.bam", tmp_path / "in.sam"
    bam.write_bytes(bam_bytes(name))
    recs, offs = bamutil.pack_records(records)
    opts, keep = L.text_opts([n for n, _ in refs])
    sam.write_bytes(K.header_text(refs).encode() + ctx.text_format(recs, offs, len(offs) - 1, opts))
    for src in (bam, sam):
        r = cli("targets", src)
        assert r.returncode == 0 and r.stdout == model(name, 500, 0).text, r.stderr
        r = cli("targets", "-v", "--maxinterval", 100000, "--gap", 10, src, "-o", tmp_path / "t.intervals")
        want = model(name, 100000, 10)
        assert r.returncode == 0 and r.stdout == b"" and (tmp_path / "t.intervals").read_bytes() == want.text, r.stderr
        line = [l for l in r.stderr.decode().splitlines() if l.startswith("[openge] targets:")]
        assert len(line) == 1 and f"{want.events} events" in line[0] and f"{want.targets} targets" in line[0], r.stderr
        assert "[openge] device:" in r.stderr.decode()


def test_cli_refusals(tmp_path):
    src = tmp_path / "in.bam"
    src.write_bytes(bam_bytes("one_event"))
    for args, msg in ((("targets", src, src), "openge targets: one BAM or SAM file is required (stdin is not provided)"),
                      (("targets",), "openge targets: one BAM or SAM file is required (stdin is not provided)"),
                      (("targets", "-"), "openge targets: one BAM or SAM file is required (stdin is not provided)"),
                      (("targets", "--gpus", 2, src), "openge targets: --gpus is not provided"),
                      (("targets", "--maxinterval", 0, src), "openge targets: --maxinterval must be at least 1"),
                      (("targets", "--gap", -1, src), "openge targets: --gap must not be negative"),
                      (("localrealign", "-R", "x.fa", "-L", "x.intervals", "--auto-targets", src), "openge localrealign: -L and --auto-targets exclude each other"),
                      (("localrealign", "-R", "x.fa", src), "One intervals file is required.")):
        r = cli(*args)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr.decode().strip().splitlines()[-1] == msg, (args, r.stderr)
    r = cli("targets", src, "-o", "/dev/full")
    assert r.returncode != 0 and b"error writing /dev/full" in r.stderr


def records_of(path):
    h, _, recs, offs = bamutil.read_bam(path)
    return h, recs, np.append(offs, np.uint64(len(recs)))


@pytest.mark.parametrize("name", RC.GOLDEN_CASES)
def test_targets_then_localrealign_gives_the_reference_records(name, tmp_path):
    """`openge targets` writes the model's text; localrealign with that file and localrealign --auto-targets give
    the same records: the reference's realigned output (the case's golden)."""
    b, meta, h, recs, offs = RC.load_case(name, tmp_path)
    refs = bamutil.read_bam(b.bam)[1]
    want = M.targets_of_arena(recs, offs[:-1], refs)
    iv = tmp_path / "t.intervals"
    r = cli("targets", b.bam, "-o", iv)
    assert r.returncode == 0 and iv.read_bytes() == want.text, r.stderr
    r = cli("localrealign", "--nopg", "-R", b.fasta, "-L", iv, b.bam, "-o", tmp_path / "by_file.bam")
    assert r.returncode == 0, r.stderr
    r = cli("localrealign", "-v", "--nopg", "-T", tmp_path, "-R", b.fasta, "--auto-targets", b.bam, "-o", tmp_path / "auto.bam")
    assert r.returncode == 0 and f"{want.targets} targets" in r.stderr.decode(), r.stderr
    assert not list(tmp_path.glob("oge_targets_*"))  # the computed file is gone
    h1, r1, o1 = records_of(tmp_path / "by_file.bam")
    h2, r2, o2 = records_of(tmp_path / "auto.bam")
    assert h1 == h2 and list(o1) == list(o2) and bytes(r1) == bytes(r2)
    RC.check_golden(meta, r2, o2)


def test_auto_targets_over_two_ranks_and_from_the_host_batch_equal_one_device(tmp_path):
    """--gpus 2 computes the targets once on the first device; a BAM on stdin is read on the host, so the targets
    come through the host-buffer form: the same records as from the device batch of one GPU."""
    b = RC.build_case("mixed", tmp_path)
    for out, more in (("one.bam", ()), ("two.bam", ("--gpus", 2))):
        r = cli("localrealign", "--nopg", *more, "-T", tmp_path, "-R", b.fasta, "--auto-targets", b.bam, "-o", tmp_path / out)
        assert r.returncode == 0, r.stderr
    with open(b.bam, "rb") as f:
        r = cli("localrealign", "--nopg", "-T", tmp_path, "-R", b.fasta, "--auto-targets", "-o", tmp_path / "stdin.bam", stdin=f)
    assert r.returncode == 0, r.stderr
    h1, r1, o1 = records_of(tmp_path / "one.bam")
    for other in ("two.bam", "stdin.bam"):
        h2, r2, o2 = records_of(tmp_path / other)
        assert h1 == h2 and list(o1) == list(o2) and bytes(r1) == bytes(r2), other
    _, rin, _ = records_of(b.bam)
    assert bytes(r1) != bytes(rin) and not list(tmp_path.glob("oge_targets_*"))


def test_auto_targets_without_indels_passes_the_records_through(tmp_path):
    b = RC.build_case("clips", tmp_path)
    refs = bamutil.read_bam(b.bam)[1]
    hdr = "@HD\tVN:1.4\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    records = [bamutil.make_record(f"p{i}", 0, 0, 100 + 7 * i, "60M", "ACGT" * 15) for i in range(50)]
    src = tmp_path / "plain.bam"
    bamutil.write_bam_py(src, hdr, refs, records)
    r = cli("localrealign", "-v", "--nopg", "-T", tmp_path, "-R", b.fasta, "--auto-targets", src, "-o", tmp_path / "out.bam")
    assert r.returncode == 0 and "[openge] LocalRealignment: no targets, the records pass through unchanged" in r.stderr.decode(), r.stderr
    assert "0 targets" in r.stderr.decode() and not list(tmp_path.glob("oge_targets_*"))
    _, rout, oout = records_of(tmp_path / "out.bam")
    assert len(oout) - 1 == len(records)
    assert [bamutil.match_key(bamutil.rec_bytes(rout, o)) for o in oout[:-1]] == [bamutil.match_key(rb) for rb in records]
