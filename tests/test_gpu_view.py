"""GPU: SAM and FASTQ text formatted on the device (csrc/sam.hip: oge_text_size_dev, oge_text_emit_dev,
oge_text_format, oge_text_host_line, the text writer of the module chain, `openge view` and -F sam on mergesort /
dedup) equal the Python restatement (tests/sam_model.py) on every crafted case, and the commands' text equals what
the reference wrote (tests/golden/view/manifest.json) byte for byte.

None of the symbols, the command or the -F values exist before this feature: every test here fails without it."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import sam_cases as K
import sam_model as M
from goldens import GOLDEN
from openge_amd import lib as L
from test_gpu_cli import OPENGE
from test_sam_model import FILES, MANIFEST, file_records, same

pytestmark = pytest.mark.gpu

CASES = K.sam_cases()
CANARY = 64


def dev(recs: np.ndarray, offs: np.ndarray):
    """(device records with their 16 bytes of slack, device offsets): keep both alive while the pointers are in use."""
    return torch.from_numpy(np.ascontiguousarray(recs)).cuda(), torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()).cuda()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(records, the model's line per record, marks) of a crafted SAM case, computed once."""
    records = CASES[name]
    return records, M.lines(records, K.NAMES), [M.needs_host(r) for r in records]


def size_pass(ctx, d_recs, d_off, n, opts):
    d_toff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_mark = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the fills run on torch's stream, the library on the context's
    total, n_host = ctx.text_size_dev(d_recs.data_ptr(), d_off.data_ptr(), n, opts, d_toff.data_ptr(), d_mark.data_ptr())
    return d_toff, d_mark, total, n_host


def emit(ctx, d_recs, d_off, d_toff, first, count, opts, nbytes):
    """The range's text and the untouched canary behind it."""
    out = torch.full((nbytes + CANARY,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.text_emit_dev(d_recs.data_ptr(), d_off.data_ptr(), d_toff.data_ptr(), first, count, opts, out.data_ptr(), nbytes)
    ctx.sync()
    h = out.cpu().numpy()
    assert (h[nbytes:] == 0xAA).all(), "bytes behind the range's text were written"
    return h[:nbytes].tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_size_and_emit_equal_the_model(ctx, name):
    """Lengths and marks per record; the emit pass over the whole range and over ranges split at record 1, at n - 1
    and on both sides of every host-formatted record; oge_text_format with the host lines spliced in and the
    sam_host_lines counter."""
    records, lines, marks = expected(name)
    n = len(records)
    recs, offs = K.pack(records)
    d_recs, d_off = dev(recs, offs)
    opts, keep = L.text_opts(K.NAMES)
    d_toff, d_mark, total, n_host = size_pass(ctx, d_recs, d_off, n, opts)
    want_len = [0 if m else len(ln) for ln, m in zip(lines, marks)]
    toff = d_toff.cpu().numpy().view(np.uint64)
    assert np.array_equal(np.diff(toff), np.array(want_len, np.uint64)) and toff[0] == 0
    assert (total, n_host) == (sum(want_len), sum(marks)) and ctx.counter("sam_host_lines") == sum(marks)
    if n:
        assert d_mark.cpu().numpy()[:n].tolist() == [int(m) for m in marks]
    want_dev = b"".join(ln for ln, m in zip(lines, marks) if not m)
    assert emit(ctx, d_recs, d_off, d_toff, 0, n, opts, total) == want_dev
    cuts = {1, n - 1} | {i + d for i, m in enumerate(marks) if m for d in (0, 1)}
    for c in sorted(x for x in cuts if 0 < x < n)[:12]:
        a, z = int(toff[c]), int(toff[n])
        assert emit(ctx, d_recs, d_off, d_toff, 0, c, opts, a) == want_dev[:a], c
        assert emit(ctx, d_recs, d_off, d_toff, c, n - c, opts, z - a) == want_dev[a:], c
    assert ctx.text_format(recs, offs, n, opts) == b"".join(lines)
    assert ctx.counter("sam_host_lines") == sum(marks)
    del keep


def test_kernel_geometry_is_what_the_cases_assume(ctx):
    records, _l, _m = expected("n5")
    recs, offs = K.pack(records)
    d_recs, d_off = dev(recs, offs)
    opts, _keep = L.text_opts(K.NAMES)
    d_toff, _mk, total, _h = size_pass(ctx, d_recs, d_off, 5, opts)
    assert ctx.timing("text_size") > 0
    emit(ctx, d_recs, d_off, d_toff, 0, 5, opts, total)
    assert (ctx.counter("text_wave_records"), ctx.counter("text_block_records")) == (K.WAVE_RECS, K.BLOCK_RECS)
    assert ctx.timing("text_emit") > 0


@pytest.mark.parametrize("trim", K.TRIMS)
def test_fastq_equals_the_model(ctx, trim):
    records = K.fastq_records() + K.seq_records() + K.name_records()
    lines = M.lines(records, [], "fastq", trim)
    recs, offs = K.pack(records)
    d_recs, d_off = dev(recs, offs)
    opts, _keep = L.text_opts(K.NAMES, L.TEXT_FASTQ, trim)
    d_toff, _mk, total, n_host = size_pass(ctx, d_recs, d_off, len(records), opts)
    assert np.array_equal(np.diff(d_toff.cpu().numpy().view(np.uint64)), np.array([len(x) for x in lines], np.uint64)) and n_host == 0
    assert emit(ctx, d_recs, d_off, d_toff, 0, len(records), opts, total) == b"".join(lines)
    assert ctx.text_format(recs, offs, len(records), opts) == b"".join(lines)


def test_no_contigs_and_a_changed_table(ctx):
    """n_ref 0 prints * for every contig; the next call with other names uses them (the table is uploaded again)."""
    records = K.ref_records() + [K.basic(i) for i in range(5)]
    recs, offs = K.pack(records)
    for names in ([], K.NAMES, ["x", "chr2", "yy"], K.NAMES):
        opts, _keep = L.text_opts(names)
        assert ctx.text_format(recs, offs, len(records), opts) == b"".join(M.lines(records, names))


def test_unknown_tag_type_is_an_error_and_nothing_is_written(ctx, tmp_path):
    records = K.unknown_records()
    recs, offs = K.pack(records)
    d_recs, d_off = dev(recs, offs)
    opts, _keep = L.text_opts(K.NAMES)
    with pytest.raises(L.OgeError, match=r"error -1: .*record 2 "):
        size_pass(ctx, d_recs, d_off, len(records), opts)
    out = np.full(4096, 0xAA, np.uint8)
    nb = C.c_uint64(5)
    rc = L.lib().oge_text_format(ctx.h, recs.ctypes.data, recs.nbytes - 16, offs.ctypes.data, len(records), C.byref(opts), out.ctypes.data,
                                 out.nbytes, C.byref(nb))
    assert rc == -1 and nb.value == 0 and (out == 0xAA).all()
    for name, bad in K.malformed_records().items():
        r2, o2 = K.pack(bad)
        with pytest.raises(L.OgeError, match=rf"error -1: .*record {len(bad) - 1} "):
            ctx.text_format(r2, o2, len(bad), opts)
    with pytest.raises(L.OgeError, match="error -1: .*unknown tag type 'q'"):
        L.Context.text_host_line(records[2], opts)
    p = tmp_path / "bad.bam"
    bamutil.write_bam_py(p, K.header_text(), K.REFS, records)
    r = cli("view", "--nopg", "-o", tmp_path / "bad.sam", p)
    assert r.returncode != 0 and b"record 2 " in r.stderr and r.stdout == b"" and not (tmp_path / "bad.sam").exists()


def test_argument_errors_go_through_the_error_message(ctx):
    opts, _keep = L.text_opts(K.NAMES)
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tot, nh = C.c_uint64(), C.c_uint64()
    lib = L.lib()
    assert lib.oge_text_size_dev(ctx.h, t.data_ptr(), t.data_ptr(), 1, None, t.data_ptr(), t.data_ptr(), C.byref(tot), C.byref(nh)) == -1
    assert b"null argument" in lib.oge_last_error(ctx.h)
    assert lib.oge_text_size_dev(ctx.h, None, t.data_ptr(), 1, C.byref(opts), t.data_ptr(), t.data_ptr(), C.byref(tot), C.byref(nh)) == -1
    assert lib.oge_text_size_dev(ctx.h, t.data_ptr(), t.data_ptr(), (1 << 32) - 1, C.byref(opts), t.data_ptr(), t.data_ptr(), C.byref(tot),
                                 C.byref(nh)) == -3
    assert b"2^32" in lib.oge_last_error(ctx.h)
    bad, _k2 = L.text_opts(K.NAMES, 2)
    assert lib.oge_text_size_dev(ctx.h, t.data_ptr(), t.data_ptr(), 0, C.byref(bad), t.data_ptr(), t.data_ptr(), C.byref(tot), C.byref(nh)) == -1
    neg, _k3 = L.text_opts(K.NAMES, L.TEXT_FASTQ, (-1, 0))
    assert lib.oge_text_size_dev(ctx.h, t.data_ptr(), t.data_ptr(), 0, C.byref(neg), t.data_ptr(), t.data_ptr(), C.byref(tot), C.byref(nh)) == -1
    records, lines, _m = expected("n5")
    recs, offs = K.pack(records)
    d_recs, d_off = dev(recs, offs)
    d_toff, _mk, total, _h = size_pass(ctx, d_recs, d_off, 5, opts)
    out = torch.full((total + CANARY,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (ctx.h, d_recs.data_ptr(), d_off.data_ptr(), d_toff.data_ptr(), 0, 5, C.byref(opts), out.data_ptr())
    assert lib.oge_text_emit_dev(*args, total - 1) == -3 and b"smaller" in lib.oge_last_error(ctx.h)
    ctx.sync()
    assert (out.cpu().numpy() == 0xAA).all()
    assert lib.oge_text_emit_dev(ctx.h, d_recs.data_ptr(), d_off.data_ptr(), None, 0, 5, C.byref(opts), out.data_ptr(), total) == -1
    assert lib.oge_text_emit_dev(*args, total) == 0


# ------------------------------------------------------------------------------------------------ the CLI
def cli(*args, env=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env={**os.environ, **(env or {})})


def sam_of(name) -> tuple[dict, dict]:
    return MANIFEST["sam"][name]["header"], MANIFEST["sam"][name]["body"]


@pytest.mark.parametrize("name", ["simple", "yhet208"])
def test_cli_view_writes_the_reference_sam(name, tmp_path):
    """stdout, -o out.sam and many chunks (OGE_TEXT_CHUNK=4096) give the bytes the reference's chain wrote."""
    src = GOLDEN / "inputs" / FILES[name]
    header, body = sam_of(name)
    r = cli("view", "--nopg", src)
    assert r.returncode == 0, r.stderr
    h, b = M.split_header(r.stdout)
    assert same(header, h) and same(body, b)
    out = tmp_path / "out.sam"
    f = cli("view", "--nopg", "-o", out, src)
    assert f.returncode == 0 and f.stdout == b"" and out.read_bytes() == r.stdout
    c = cli("view", "--nopg", src, env={"OGE_TEXT_CHUNK": "4096"})
    assert c.returncode == 0 and c.stdout == r.stdout
    v = cli("view", "--nopg", "-v", src, env={"OGE_TEXT_CHUNK": "4096"})
    chunks = int(v.stderr.split(b" chunks")[0].split()[-1])
    assert chunks >= len(r.stdout) // 4096 and v.stdout == r.stdout
    bam = tmp_path / "out.bam"  # a .bam name keeps the BAM writer
    assert cli("view", "--nopg", "-o", bam, src).returncode == 0
    _t, refs, recs, offs = bamutil.read_bam(bam)
    assert same(body, b"".join(M.lines(M.split_records(recs, offs), [n for n, _ in refs])))


@pytest.mark.parametrize("name", ["floats", "mix_ref", "tags", "widths", "refs", "cigar", "seq_short", "names", "n17"])
def test_cli_view_of_crafted_cases_writes_the_reference_sam(name, tmp_path):
    """Through the file reader, the Filter and the chunked writer: the host lines (f tags) land inside chunks and on
    chunk edges at OGE_TEXT_CHUNK=4096."""
    src = tmp_path / "in.bam"
    bamutil.write_bam_py(src, K.header_text(), K.REFS, CASES[name])
    header, body = sam_of(name)
    for env in (None, {"OGE_TEXT_CHUNK": "4096"}, {"OGE_TEXT_CHUNK": "1"}):
        if env and env["OGE_TEXT_CHUNK"] == "1" and len(CASES[name]) > 300:
            continue
        r = cli("view", "--nopg", src, env=env)
        assert r.returncode == 0, r.stderr
        h, b = M.split_header(r.stdout)
        assert same(header, h) and same(body, b), env


def test_cli_view_with_arrays_equals_the_model(tmp_path):
    """B arrays are outside what the reference defines: the model's rendering, spliced in at every chunk size."""
    src = tmp_path / "in.bam"
    records = CASES["mix"][:600] + CASES["arrays"]
    bamutil.write_bam_py(src, K.header_text(), K.REFS, records)
    want = b"".join(M.lines(M.filter_keep(records), K.NAMES))
    for chunk in ("4096", "300", str(1 << 26)):
        r = cli("view", "--nopg", src, env={"OGE_TEXT_CHUNK": chunk})
        assert r.returncode == 0 and M.split_header(r.stdout)[1] == want, chunk


@pytest.mark.parametrize("name,key", [(n, k) for n in sorted(MANIFEST["filters"]) for k in sorted(MANIFEST["filters"][n])])
def test_cli_view_filters_write_the_reference_sam(name, key):
    g = MANIFEST["filters"][name][key]
    r = cli("view", "--nopg", *g["args"], GOLDEN / "inputs" / FILES[name])
    assert r.returncode == 0, r.stderr
    h, b = M.split_header(r.stdout)
    assert same(g["header"], h) and same(g["body"], b)


def test_cli_view_filter_combinations_equal_the_model():
    """Combinations the reference was not run on (its chain does not return from -r with -n): the model on the
    records the existing Filter semantics keep."""
    refs, records = file_records("yhet208")
    names = [n for n, _ in refs]
    for args in (["-r", "YHet:10000..200000", "-q", "30", "-n", "700"], ["-n", "5", "-l", "-64"], ["-r", "YHet:10000..30000", "-l", "+46"]):
        r = cli("view", "--nopg", *args, GOLDEN / "inputs" / FILES["yhet208"])
        kept = M.filter_keep(records, **M.filter_args(args, refs))
        assert r.returncode == 0 and kept and M.split_header(r.stdout)[1] == b"".join(M.lines(kept, names)), args


@pytest.mark.parametrize("name", ["simple", "yhet208", "crafted"])
def test_cli_view_fastq(name, tmp_path):
    """-F fastq to stdout equals the reference's text; -B 3 -E 4 the model's (the reference's QUAL under a trim window
    is not a function of the record: tests/golden/make_view_goldens.py) with the reference's names and bases."""
    if name == "crafted":
        src, records = tmp_path / "in.bam", K.fastq_records()
        bamutil.write_bam_py(src, K.header_text(), K.REFS, records)
    else:
        src, records = GOLDEN / "inputs" / FILES[name], file_records(name)[1]
    r = cli("view", "-F", "fastq", src)
    assert r.returncode == 0 and same(MANIFEST["fastq"][name], r.stdout), r.stderr
    for env in (None, {"OGE_TEXT_CHUNK": "4096"}):
        t = cli("view", "-F", "FASTQ", "-B", "3", "-E", "4", src, env=env)
        kept = M.filter_keep(records, trim_total=7)
        assert t.returncode == 0 and t.stdout == b"".join(M.lines(kept, [], "fastq", (3, 4))), t.stderr
    if name != "crafted":
        full, cut = r.stdout.split(b"\n"), t.stdout.split(b"\n")  # every read is longer than 7: the same entries in the same order
        assert len(full) == len(cut) and all(cut[k] == full[k] and cut[k + 1] == full[k + 1][3:-4] for k in range(0, len(cut) - 1, 4))


def test_cli_program_line_in_the_sam_header(tmp_path):
    src = GOLDEN / "inputs" / FILES["simple"]
    r = cli("view", "-q", "30", src)
    assert r.returncode == 0
    h, b = M.split_header(r.stdout)
    plain = cli("view", "--nopg", "-q", "30", src)
    hp, bp = M.split_header(plain.stdout)
    added = [ln for ln in h.decode().splitlines() if ln not in hp.decode().splitlines()]
    # the input carries @PG ID:openge already: FileWriter takes the next free id (file_writer.cpp:81-85)
    assert added == [f"@PG\tID:openge-2\tCL:openge view -q 30 {src} \tVN:0.3-dev"]
    assert bp == b and hp == h.replace((added[0] + "\n").encode(), b"")
    fresh = tmp_path / "in.bam"
    bamutil.write_bam_py(fresh, K.header_text(), K.REFS, CASES["n5"])
    h2 = M.split_header(cli("view", fresh).stdout)[0].decode().splitlines()
    assert [ln for ln in h2 if ln.startswith("@PG")] == [f"@PG\tID:openge\tCL:openge view {fresh} \tVN:0.3-dev"]


@pytest.mark.parametrize("cmd", [("mergesort",), ("mergesort", "-M"), ("dedup",), ("dedup", "-r"), ("sort", "-q", "30")])
def test_cli_sam_from_the_sorting_and_dedup_commands(cmd, tmp_path):
    """-F sam gives the model's text of the records the same command writes as BAM; 0x400 shows in the FLAG column."""
    src = GOLDEN / "inputs" / FILES["yhet208"]
    if cmd[0] == "dedup":  # dedup wants sorted input
        assert cli("mergesort", "--nopg", "-o", tmp_path / "s.bam", src).returncode == 0
        src = tmp_path / "s.bam"
    bam, sam = tmp_path / "x.bam", tmp_path / "x.sam"
    assert cli(*cmd, "--nopg", "-o", bam, src).returncode == 0
    r = cli(*cmd, "--nopg", "-F", "sam", "-o", sam, src)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    text, refs, recs, offs = bamutil.read_bam(bam)
    records = M.split_records(recs, offs)
    h, b = M.split_header(sam.read_bytes())
    assert b == b"".join(M.lines(records, [n for n, _ in refs]))
    assert h.decode() == text
    flags = [int(ln.split(b"\t")[1]) for ln in b.splitlines()]
    if "-M" in cmd or cmd == ("dedup",):
        assert any(f & 0x400 for f in flags)
    if "-r" in cmd:
        assert flags and not any(f & 0x400 for f in flags)
    so = cli(*cmd, "--nopg", "-F", "sam", src)  # to stdout
    assert so.returncode == 0 and so.stdout == sam.read_bytes()
    named = tmp_path / "y.sam"  # without -F the name does not choose the format on these commands
    assert cli(*cmd, "--nopg", "-o", named, src).returncode == 0 and named.read_bytes()[:2] == b"\x1f\x8b"


SIMPLE = GOLDEN / "inputs" / "simple.bam"


@pytest.mark.parametrize("args,msg", [
    (("view", "-B", "3", SIMPLE), "Trimming reads is only supported for the FASTQ format at this time. Aborting."),
    (("view", "-E", "3", "-F", "sam", SIMPLE), "Trimming reads is only supported for the FASTQ format at this time. Aborting."),
    (("view", "-F", "fastq", "-o", "reads", SIMPLE), "FASTQ output is not provided with an output file"),
    (("view", "-o", "reads.fastq", SIMPLE), "FASTQ output is not provided with an output file"),
    (("view", "--gpus", "2", SIMPLE), "SAM output is not provided with --gpus"),
    (("view", "--gpus", "2", "-F", "bam", SIMPLE), "openge view: --gpus is not provided"),
    (("mergesort", "--gpus=2", "-F", "sam", SIMPLE), "SAM output is not provided with --gpus"),
    (("mergesort", "--index", "-F", "sam", "-o", "x.sam", SIMPLE), "SAM output is not provided with --index"),
    (("dedup", "--index", "-F", "sam", "-o", "x.sam", SIMPLE), "SAM output is not provided with --index"),
    (("view", "-F", "xyz", SIMPLE), "Unknown file format specified: xyz. Aborting."),
    (("mergesort", "-F", "xyz", SIMPLE), "Unknown file format specified: xyz. Aborting."),
    (("dedup", "-F", "fastq", SIMPLE), "FASTQ output is not provided with this command"),
    (("view", "-F", "cram", SIMPLE), "is not provided (bam, sam or fastq)"),
    (("localrealign", "-F", "sam", SIMPLE), "SAM output is not provided with localrealign"),
])
def test_cli_refusals(args, msg, tmp_path):
    r = subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, cwd=tmp_path)
    assert r.returncode != 0 and msg in r.stderr.decode() and r.stdout == b"", (r.returncode, r.stderr)
    assert len(r.stderr.decode().strip().splitlines()) == 1 and not list(tmp_path.iterdir())
