"""GPU: the duplication metrics counted on the device (csrc/dupmetrics.hip: oge_dup_metrics_dev, its host-buffer and
whole-file forms, the lib.py wrappers, `dedup --metrics`, `mergesort -M --metrics` and `openge dupmetrics`) equal the
Python restatement (tests/dupmetrics_model.py) on every crafted case, and on the golden cases the counts of the
device's own marking equal the model's counts of the reference's duplicate flags.

Neither the symbols, the option nor the command exist before this feature: every test here fails without it."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import dupmetrics_cases as K
import dupmetrics_model as M
from goldens import load_case
from openge_amd import lib as L
from test_gpu_cli import OPENGE, case_input

pytestmark = pytest.mark.gpu

CASES = K.cases()


def dev(recs: np.ndarray, offs: np.ndarray):
    """(device records, device offsets): keep both alive while the pointers are in use."""
    return torch.from_numpy(np.ascontiguousarray(recs)).cuda(), torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()).cuda()


@functools.lru_cache(maxsize=None)
def want(name):
    """(read-group table, unknown_lib, names, the model's counts): computed once per case"""
    header, records = CASES[name]
    rg_lib, unknown, names = M.lib_table(header)
    return rg_lib, unknown, names, M.count(records, rg_lib, unknown, len(names))


def as_lists(a: np.ndarray) -> list[list[int]]:
    return [[int(v) for v in row] for row in a]


@pytest.mark.parametrize("name", list(CASES))
def test_counts_equal_the_model_in_every_form(ctx, name):
    """n = 0, 1, 63, 64, 65, T - 1, T, T + 1, 2 T + 1 with the records at the wave and tile edges alone in their
    libraries; the 256-record flag x refID table over three libraries; 3 T records of one key; every RG shape; a
    header without @RG; 1, 2, C and C + 1 libraries on both sides of the LDS table's limit: device records, host
    buffers and the whole file give the model's counts."""
    header, records = CASES[name]
    rg_lib, unknown, names, counts = want(name)
    recs, offs = bamutil.pack_records(records)
    offs = offs[:-1]
    opts, keep = L.markdup_opts_from_header(header, len(K.REFS))
    assert opts.unknown_lib == unknown and opts.n_rg == header.count("@RG\t")
    n_lib = len(names)
    d = dev(recs, offs)
    got = ctx.dup_metrics_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), opts, n_lib)
    assert as_lists(got) == counts, (name, "dev")
    assert (ctx.counter("dupmetrics_tile_records"), ctx.counter("dupmetrics_lds_libs")) == (K.TILE, K.LDS_LIBS)
    assert as_lists(ctx.dup_metrics(recs, offs, len(offs), opts, n_lib)) == counts, (name, "host")
    # a wider table: the same rows, the rest zero (and the other counting kernel when it crosses the LDS limit)
    wide = as_lists(ctx.dup_metrics_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), opts, K.LDS_LIBS + 9))
    assert wide[:n_lib] == counts and not any(any(r) for r in wide[n_lib:]), (name, "wide")
    fc, fnames, funknown = ctx.bam_dup_metrics(bamutil.bgzf_blocks(K.bam_body(header, K.REFS, records)))
    assert (as_lists(fc), fnames, funknown) == (counts, names, unknown), (name, "file")


def test_stage_is_timed_and_out_is_set_not_added(ctx):
    header, records = CASES["n65"]
    recs, offs = bamutil.pack_records(records)
    opts, keep = L.markdup_opts_from_header(header, len(K.REFS))
    a = ctx.dup_metrics(recs, offs[:-1], 65, opts, len(want("n65")[2]))
    assert ctx.timing("dup_metrics") > 0
    b = ctx.dup_metrics(recs, offs[:-1], 65, opts, len(want("n65")[2]))  # the wrapper hands in a filled array
    assert (a == b).all() and int(a[:, :4].sum()) == 65


def test_counts_of_a_partition_add_up(ctx):
    header, records = CASES["rg_shapes"]
    rg_lib, unknown, names, counts = want("rg_shapes")
    opts, keep = L.markdup_opts_from_header(header, len(K.REFS))
    total = np.zeros((len(names), 6), np.uint64)
    for part in (records[:1], records[1:70], records[70:]):
        recs, offs = bamutil.pack_records(part)
        total += ctx.dup_metrics(recs, offs[:-1], len(part), opts, len(names))
    assert as_lists(total) == counts


def test_library_id_outside_the_table_is_an_argument_error(ctx):
    header, records = CASES["libs2"]
    recs, offs = bamutil.pack_records(records)
    opts, keep = L.markdup_opts_from_header(header, len(K.REFS))
    n_lib = len(want("libs2")[2])
    d = dev(recs, offs[:-1])
    for call in (lambda n: ctx.dup_metrics_dev(d[0].data_ptr(), d[1].data_ptr(), len(records), opts, n),
                 lambda n: ctx.dup_metrics(recs, offs[:-1], len(records), opts, n)):
        for bad in (n_lib - 1, 2, 0, -1):  # unknown_lib, then a read group's library, fall outside
            with pytest.raises(L.OgeError) as e:
                call(bad)
            assert "error -1:" in str(e.value)
        assert as_lists(call(n_lib)) == want("libs2")[3]
    keep[1][0] = -3  # a negative id in the table
    with pytest.raises(L.OgeError) as e:
        ctx.dup_metrics(recs, offs[:-1], len(records), opts, n_lib)
    assert "error -1:" in str(e.value) and "read group 0" in str(e.value)


def test_unterminated_read_group_ids_are_an_argument_error(ctx):
    """two ids in six bytes of which rg_ids_bytes declares five: refused on the host, before anything is launched"""
    header, records = CASES["n0"]
    recs, offs = bamutil.pack_records(records)
    ids = np.frombuffer(b"g1\0g2\0", np.uint8).copy()
    libs = np.array([1, 1, 0], np.int16)
    o = L.MarkdupOpts()
    o.n_ref, o.rg_ids, o.rg_ids_bytes, o.rg_lib, o.n_rg, o.unknown_lib = len(K.REFS), ids.ctypes.data, 5, libs.ctypes.data, 2, 2
    d = dev(recs, offs[:-1])
    with pytest.raises(L.OgeError, match=r"error -1: .*not n_rg NUL-terminated"):
        ctx.dup_metrics_dev(d[0].data_ptr(), d[1].data_ptr(), len(records), o, 3)
    o.rg_ids_bytes = 6
    assert as_lists(ctx.dup_metrics_dev(d[0].data_ptr(), d[1].data_ptr(), len(records), o, 3)) == [[0] * 6] * 3


# ------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def golden(name):
    return load_case(name)


@pytest.mark.parametrize("name", ["simple", "edge", "mix3k", "c2_20k"])
def test_marking_then_metrics_equal_the_model_on_the_reference_flags(ctx, built, name):
    """oge_markdup_dev with apply, then oge_dup_metrics_dev: the model's counts of the case's input records carrying
    the reference's duplicate indices (the arrays goldens.check_dups reads for the same options)."""
    case = golden(name)
    rg_lib, unknown, names = M.lib_table(case.header)
    dup_at = set(int(i) for i in case.arrays["dedup_input_v"])
    marked = []
    for i, rb in enumerate(M.records_of_arena(case.recs, case.offs[:-1])):
        b = bytearray(rb)
        b[19] = (b[19] & ~0x04 & 0xFF) | (0x04 if i in dup_at else 0)  # FLAG 0x400 is bit 2 of the high byte
        marked.append(bytes(b))
    counts = M.count(marked, rg_lib, unknown, len(names))
    opts, keep = L.markdup_opts_from_header(case.header, case.n_ref)
    d = dev(case.recs, case.offs[:-1])
    d_dup = torch.zeros(case.n + 1, dtype=torch.uint8, device="cuda")
    nd = ctx.markdup_dev(d[0].data_ptr(), d[1].data_ptr(), case.n, opts, d_dup.data_ptr(), apply=True)
    ctx.sync()
    got = ctx.dup_metrics_dev(d[0].data_ptr(), d[1].data_ptr(), case.n, opts, len(names))
    assert as_lists(got) == counts
    assert nd > 0 and sum(r[4] + r[5] for r in counts) > 0 and sum(sum(r[:4]) for r in counts) == case.n


# ------------------------------------------------------------------------------------------------ the CLI
def cli(*args, env=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def model_text_of(bam_path, command_line: str) -> bytes:
    header, _, recs, offs = bamutil.read_bam(bam_path)
    rg_lib, unknown, names = M.lib_table(header)
    counts = M.count(M.records_of_arena(recs, offs), rg_lib, unknown, len(names))
    return M.text(M.rows(names, unknown, counts), command_line)


def command_line(*args) -> str:
    return "openge " + " ".join(map(str, args))


def rows_of(data: bytes):
    return M.parse(data)[1]


CLI_CASES = ["mix3k", "edge"]


@pytest.fixture(scope="module")
def marked(built, tmp_path_factory):
    """name -> (input, out.bam of `dedup --metrics`, the rows of its metrics file): one run per case, made when asked for"""
    made = {}

    def get(name):
        if name not in made:
            d = tmp_path_factory.mktemp(f"dupmetrics_{name}")
            src = case_input(golden(name), d)
            out, met = d / "out.bam", d / "m.txt"
            args = ("dedup", "--nopg", "--metrics", met, src, "-o", out)
            r = cli(*args)
            assert r.returncode == 0, r.stderr
            # the model's text of the records read back from out.bam
            assert met.read_bytes() == model_text_of(out, command_line(*args))
            made[name] = (src, out, rows_of(met.read_bytes()))
        return made[name]
    return get


@pytest.mark.parametrize("name", CLI_CASES)
def test_cli_dedup_metrics_file_and_unchanged_output(marked, name, tmp_path):
    src, out, rows = marked(name)
    assert sum(int(x["UNPAIRED_READ_DUPLICATES"]) + int(x["READ_PAIR_DUPLICATES"]) for x in rows) > 0
    assert sum(int(x["UNPAIRED_READS_EXAMINED"]) + 2 * int(x["READ_PAIRS_EXAMINED"]) for x in rows) > 0
    r = cli("dedup", "--nopg", src, "-o", tmp_path / "plain.bam")  # out.bam is byte-identical without --metrics
    assert r.returncode == 0 and (tmp_path / "plain.bam").read_bytes() == out.read_bytes(), r.stderr


@pytest.mark.parametrize("name", CLI_CASES)
def test_cli_remove_gives_the_same_metrics(marked, name, tmp_path):
    src, out, rows = marked(name)
    r = cli("dedup", "--nopg", "-r", "-v", "--metrics", tmp_path / "m.txt", src, "-o", tmp_path / "removed.bam")
    assert r.returncode == 0 and rows_of((tmp_path / "m.txt").read_bytes()) == rows, r.stderr
    assert len([l for l in r.stderr.decode().splitlines() if l.startswith("[openge] MarkDuplicates: metrics of") and "dup_metrics" in l]) == 1
    kept = bamutil.read_bam(tmp_path / "removed.bam")
    assert len(kept[3]) < golden(name).n and not any(f & 0x400 for f in bamutil.flags_of(kept[2], kept[3]))  # the duplicates are gone


PATHS = {"fused": (("sort", "-M"), None), "chunked": (("sort", "-M"), {"OGE_CHUNK_BYTES": "200000"}),
         "chunked_R": (("sort", "-R"), {"OGE_CHUNK_BYTES": "200000"}), "gpus2": (("sort", "-M", "--gpus", 2), None),
         "dedup_gpus2": (("dedup", "--gpus", 2), None)}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", CLI_CASES)
def test_cli_every_dedup_path_gives_the_same_counts(marked, name, path, tmp_path):
    """sort -M --metrics (the fused pipeline), a small OGE_CHUNK_BYTES (the chunked path, also with -R), two ranks
    (sharing a device where there is one), the in-place dedup over two ranks: the rows of `dedup --metrics`, and the
    same output file as without --metrics."""
    src, out, rows = marked(name)
    more, env = PATHS[path]
    r = cli(*more, "--nopg", "-v", "--metrics", tmp_path / "m.txt", src, "-o", tmp_path / "o.bam", env=env)
    assert r.returncode == 0, r.stderr
    assert ("sorted runs" in r.stderr.decode()) == path.startswith("chunked")
    assert rows_of((tmp_path / "m.txt").read_bytes()) == rows
    if "-R" not in more:
        assert (tmp_path / "m.txt").read_bytes() == model_text_of(tmp_path / "o.bam", command_line(*more, "--nopg", "-v", "--metrics", tmp_path / "m.txt", src, "-o", tmp_path / "o.bam"))
    r = cli(*more, "--nopg", src, "-o", tmp_path / "again.bam", env=env)
    assert r.returncode == 0 and (tmp_path / "again.bam").read_bytes() == (tmp_path / "o.bam").read_bytes(), r.stderr


@pytest.mark.parametrize("name", CLI_CASES)
def test_cli_dupmetrics_of_the_marked_file(marked, name, tmp_path):
    src, out, rows = marked(name)
    r = cli("dupmetrics", "-v", out)  # under its own command line
    assert r.returncode == 0 and r.stdout == model_text_of(out, command_line("dupmetrics", "-v", out)), r.stderr
    assert rows_of(r.stdout) == rows and "dup_metrics" in r.stderr.decode()
    r = cli("dupmetrics", out, "-o", tmp_path / "again.txt")
    assert r.returncode == 0 and r.stdout == b"" and rows_of((tmp_path / "again.txt").read_bytes()) == rows, r.stderr


def test_cli_dupmetrics_reads_sam_and_names_the_unknown_library(ctx, tmp_path):
    """A header without @RG: one "Unknown Library" row, from the BAM file and from its SAM text."""
    header, records = CASES["no_rg_lines"]
    bam, sam = tmp_path / "in.bam", tmp_path / "in.sam"
    bamutil.write_bam_py(bam, header, K.REFS, records)
    recs, offs = bamutil.pack_records(records)
    opts, keep = L.text_opts([n for n, _ in K.REFS])
    sam.write_bytes(header.encode() + ctx.text_format(recs, offs, len(offs) - 1, opts))
    want_rows = rows_of(model_text_of(bam, "x"))
    assert [r["LIBRARY"] for r in want_rows] == ["Unknown Library"]
    for src in (bam, sam):
        r = cli("dupmetrics", src)
        assert r.returncode == 0 and rows_of(r.stdout) == want_rows, r.stderr
    header, records = CASES["rg_shapes"]
    bamutil.write_bam_py(bam, header, K.REFS, records)
    r = cli("dupmetrics", bam)
    assert r.returncode == 0 and r.stdout == model_text_of(bam, command_line("dupmetrics", bam)), r.stderr
    assert [x["LIBRARY"] for x in rows_of(r.stdout)].count("Unknown Library") == 1


def test_cli_refusals_write_nothing(tmp_path):
    src, out, met = tmp_path / "in.bam", tmp_path / "out.bam", tmp_path / "m.txt"
    bamutil.write_bam_py(src, CASES["n65"][0], K.REFS, CASES["n65"][1])
    for args, msg in ((("mergesort", "--metrics", met, src, "-o", out), "openge mergesort: --metrics needs -M or -R (there is nothing to count without the duplicate marking)"),
                      (("sort", "--metrics", met, src, "-o", out), "openge mergesort: --metrics needs -M or -R (there is nothing to count without the duplicate marking)"),
                      (("dedup", "--metrics", out, src, "-o", out), "openge dedup: --metrics names the output file"),
                      (("sort", "-M", "--metrics", out, src, "-o", out), "openge mergesort: --metrics names the output file"),
                      (("dedup", "--metrics", "stdout", src, "-o", out), "openge dedup: --metrics needs a file name (stdout is not provided)"),
                      (("dedup", "--metrics", "-", src, "-o", out), "openge dedup: --metrics needs a file name (stdout is not provided)"),
                      (("sort", "-M", "--metrics", "-", src, "-o", out), "openge mergesort: --metrics needs a file name (stdout is not provided)"),
                      (("dupmetrics",), "openge dupmetrics: one BAM or SAM file is required (stdin is not provided)"),
                      (("dupmetrics", src, src), "openge dupmetrics: one BAM or SAM file is required (stdin is not provided)"),
                      (("dupmetrics", "-"), "openge dupmetrics: one BAM or SAM file is required (stdin is not provided)"),
                      (("dupmetrics", "--gpus", 2, src), "openge dupmetrics: --gpus is not provided")):
        r = cli(*args)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr.decode().strip().splitlines()[-1] == msg, (args, r.stderr)
        assert not out.exists() and not met.exists(), args
    r = cli("dedup", "--metrics", "/dev/full", src, "-o", out)
    assert r.returncode != 0 and b"error writing /dev/full" in r.stderr
