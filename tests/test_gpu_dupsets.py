"""GPU: the duplicate sets computed on the device (csrc/dupsets.hip: oge_dup_sets_dev, its host-buffer and whole-file
forms, the lib.py wrappers, `--optical-distance` on `dedup --metrics`, `mergesort -M --metrics` and `openge dupmetrics`)
equal the Python restatement (tests/dupsets_model.py) exactly: per library pairs, sets, located and optical duplicates,
and the three set-size histograms, on every crafted case and on the reference's own 208.yhet.bam.

Neither the symbols, the option nor the text exist before this feature: every test here fails without it."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import dupmetrics_cases as DK
import dupmetrics_model as DM
import dupsets_cases as K
import dupsets_model as M
from goldens import load_case
from openge_amd import lib as L
from test_gpu_cli import OPENGE, case_input

pytestmark = pytest.mark.gpu

CASES = K.cases()
ERR_ARG, ERR_LIMIT = -1, -3


def dev(recs: np.ndarray, offs: np.ndarray):
    """(device records, device offsets): keep both alive while the pointers are in use."""
    return torch.from_numpy(np.ascontiguousarray(recs)).cuda(), torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()).cuda()


@functools.lru_cache(maxsize=None)
def packed(name):
    header, records, _ = CASES[name]
    recs, offs = bamutil.pack_records(records)
    return header, recs, offs[:-1]


@functools.lru_cache(maxsize=None)
def want(name, D):
    """the model's (per library, histograms): computed once per case and distance"""
    header, recs, offs = packed(name)
    return M.compute(recs, offs, header, D)


def as_lists(a: np.ndarray) -> list[list[int]]:
    return [[int(v) for v in row] for row in a]


def got_lists(result):
    return as_lists(result[0]), as_lists(result[1])


@pytest.mark.parametrize("name", list(CASES))
def test_every_form_equals_the_model(ctx, name):
    """n = 0; no pairs; sets of 1, 2, 63, 64, 65, cap - 1, cap and cap + 1 pairs; a set across a wave's 64 lanes; runs of
    two-pair sets to the wave and workgroup edges, also shifted by a set of three; the chain in its six orders; one
    position in two libraries; two read groups of one library; tiles; FR / RF sets divided by 0x40 and FF / RR sets
    not; mates on two contigs; D = 0; names without a location; a shuffled copy: device records, host buffers and
    the whole file give the model's numbers."""
    header, recs, offs = packed(name)
    opts, keep = L.markdup_opts_from_header(header, len(K.REFS))
    n_lib = len(DM.lib_table(header)[2])
    d = dev(recs, offs)
    for D in CASES[name][2]:
        per_lib, hist = want(name, D)
        assert got_lists(ctx.dup_sets_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), opts, D, n_lib)) == (per_lib, hist), (name, D, "dev")
        assert (ctx.counter("dupsets_wave_cap"), ctx.counter("dupsets_block_cap")) == (K.WAVE_CAP, K.BLOCK_CAP)
        multi = sum(hist[0][2:])  # every set of two or more pairs is counted in exactly one tier
        tiers = [ctx.counter("dupsets_wave_sets"), ctx.counter("dupsets_block_sets"), ctx.counter("dupsets_host_sets")]
        assert sum(tiers) == multi, (name, tiers)
        assert tiers[0] == sum(hist[0][2:K.WAVE_CAP + 1]) and tiers[2] == (1 if name == "block_p1" else 0), (name, tiers)
        assert got_lists(ctx.dup_sets(recs, offs, len(offs), opts, D, n_lib)) == (per_lib, hist), (name, D, "host")
        assert got_lists(ctx.bam_dup_sets(bamutil.bgzf_blocks(DK.bam_body(header, K.REFS, CASES[name][1])), D)) == (per_lib, hist), (name, D, "file")
        # pairs - sets is section 26's READ_PAIR_DUPLICATES of the dedup's own marking (no mate refID is -1 here)
        d2 = dev(recs, offs)
        d_dup = torch.zeros(len(offs) + 1, dtype=torch.uint8, device="cuda")
        ctx.markdup_dev(d2[0].data_ptr(), d2[1].data_ptr(), len(offs), opts, d_dup.data_ptr(), apply=True)
        ctx.sync()
        counts = ctx.dup_metrics_dev(d2[0].data_ptr(), d2[1].data_ptr(), len(offs), opts, n_lib)
        assert [r[0] - r[1] for r in per_lib] == [int(c[5]) // 2 for c in counts], name
        # the duplicate flags are not read: the marked records give the same
        assert got_lists(ctx.dup_sets_dev(d2[0].data_ptr(), d2[1].data_ptr(), len(offs), opts, D, n_lib)) == (per_lib, hist), (name, D, "marked")


def test_tiers_take_the_sets_they_should(ctx):
    header, recs, offs = packed("sizes_small")
    opts, keep = L.markdup_opts_from_header(header, len(K.REFS))
    ctx.dup_sets(recs, offs, len(offs), opts, 100, 4)
    assert (ctx.counter("dupsets_wave_sets"), ctx.counter("dupsets_block_sets"), ctx.counter("dupsets_host_sets")) == (4, 1, 0)   # 2, 3, 63, 64 | 65
    assert ctx.timing("dup_sets") > 0 and ctx.timing("ds_locate") > 0 and ctx.timing("ds_components") > 0
    header, recs, offs = packed("block_p1")
    ctx.dup_sets(recs, offs, len(offs), opts, 100, 4)
    assert (ctx.counter("dupsets_wave_sets"), ctx.counter("dupsets_block_sets"), ctx.counter("dupsets_host_sets")) == (2, 0, 1)
    header, recs, offs = packed("block")
    ctx.dup_sets(recs, offs, len(offs), opts, 100, 4)
    assert (ctx.counter("dupsets_wave_sets"), ctx.counter("dupsets_block_sets"), ctx.counter("dupsets_host_sets")) == (1, 1, 0)


def test_a_shuffled_copy_gives_identical_output(ctx):
    opts, keep = L.markdup_opts_from_header(K.HEADER, len(K.REFS))
    out = []
    for name in ("mixed", "mixed_shuffled"):
        header, recs, offs = packed(name)
        out.append(got_lists(ctx.dup_sets(recs, offs, len(offs), opts, 100, 4)))
    assert out[0] == out[1] and sum(r[3] for r in out[0][0]) > 0


def test_a_wider_table_and_the_refusals(ctx):
    header, recs, offs = packed("libs_rgs_tiles")
    opts, keep = L.markdup_opts_from_header(header, len(K.REFS))
    per_lib, hist = want("libs_rgs_tiles", 100)
    wide = got_lists(ctx.dup_sets(recs, offs, len(offs), opts, 100, 70))
    assert wide[0][:4] == per_lib and not any(any(r) for r in wide[0][4:]) and wide[1] == hist
    for bad, code in (((100, 3), ERR_ARG), ((100, 0), ERR_ARG), ((-1, 4), ERR_ARG), ((1 << 31, 4), ERR_ARG), ((100, 2049), ERR_LIMIT)):
        with pytest.raises(L.OgeError) as e:
            ctx.dup_sets(recs, offs, len(offs), opts, *bad)
        assert f"error {code}:" in str(e.value), bad
    d = dev(recs, offs)
    with pytest.raises(L.OgeError) as e:   # the limit is checked before anything is read
        ctx.dup_sets_dev(d[0].data_ptr(), d[1].data_ptr(), 1 << 31, opts, 100, 4)
    assert f"error {ERR_LIMIT}:" in str(e.value)
    split, keep2 = L.markdup_opts_from_header(header, len(K.REFS), split_chains=4)
    with pytest.raises(L.OgeError) as e:
        ctx.dup_sets(recs, offs, len(offs), split, 100, 4)
    assert f"error {ERR_ARG}:" in str(e.value)
    assert got_lists(ctx.dup_sets(recs, offs, len(offs), opts, 100, 4)) == (per_lib, hist)


def test_unterminated_read_group_ids_are_an_argument_error(ctx):
    """two ids in six bytes of which rg_ids_bytes declares five: refused on the host, before anything is launched"""
    header, recs, offs = packed("n0")
    ids = np.frombuffer(b"g1\0g2\0", np.uint8).copy()
    libs = np.array([1, 1, 0], np.int16)
    o = L.MarkdupOpts()
    o.n_ref, o.rg_ids, o.rg_ids_bytes, o.rg_lib, o.n_rg, o.unknown_lib = len(K.REFS), ids.ctypes.data, 5, libs.ctypes.data, 2, 2
    d = dev(recs, offs)
    with pytest.raises(L.OgeError, match=rf"error {ERR_ARG}: .*not n_rg NUL-terminated"):
        ctx.dup_sets_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), o, 100, 3)
    o.rg_ids_bytes = 6
    per_lib, hist = got_lists(ctx.dup_sets_dev(d[0].data_ptr(), d[1].data_ptr(), len(offs), o, 100, 3))
    assert per_lib == [[0] * 4] * 3 and not any(any(r) for r in hist)


def test_text_equals_the_model(ctx):
    for name, D in (("chain", 100), ("libs_rgs_tiles", 100), ("n0", 100), ("block", 100)):
        header, recs, offs = packed(name)
        rg_lib, unknown, names = DM.lib_table(header)
        counts = DM.count(DM.records_of_arena(recs, offs), rg_lib, unknown, len(names))
        per_lib, hist = want(name, D)
        rows = [(nm, counts[k], per_lib[k]) for k, nm in enumerate(names) if nm]
        assert L.dup_sets_text(rows, hist, "openge x") == M.text(rows, hist, "openge x"), name
        assert L.dup_sets_text(rows[:1], hist, "y") == M.text(rows[:1], hist, "y"), name   # one row: the ROI column when there is an estimate


# ------------------------------------------------------------------------------------------------ the reference's file
@functools.lru_cache(maxsize=None)
def yhet():
    return load_case("yhet208")


@pytest.mark.parametrize("D", [100, 2500])
def test_golden_counts_and_histograms(ctx, D):
    case = yhet()
    per_lib, hist = M.compute(case.recs, case.offs[:-1], case.header, D)
    opts, keep = L.markdup_opts_from_header(case.header, case.n_ref)
    d = dev(case.recs, case.offs[:-1])
    assert got_lists(ctx.dup_sets_dev(d[0].data_ptr(), d[1].data_ptr(), case.n, opts, D, len(per_lib))) == (per_lib, hist)
    assert sum(r[3] for r in per_lib) > 0 and sum(r[0] for r in per_lib) == 6950 and sum(r[1] for r in per_lib) == 3819
    assert ctx.counter("dupsets_wave_sets") == sum(hist[0][2:]) and ctx.counter("dupsets_host_sets") == 0


# ------------------------------------------------------------------------------------------------ the CLI
def cli(*args, env=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def command_line(*args) -> str:
    return "openge " + " ".join(map(str, args))


def model_text_of(bam_path, D, cl: str) -> bytes:
    header, _, recs, offs = bamutil.read_bam(bam_path)
    return M.text_of_records(recs, offs, header, D, cl)


def section26_text_of(bam_path, cl: str) -> bytes:
    header, _, recs, offs = bamutil.read_bam(bam_path)
    rg_lib, unknown, names = DM.lib_table(header)
    return DM.text(DM.rows(names, unknown, DM.count(DM.records_of_arena(recs, offs), rg_lib, unknown, len(names))), cl)


def body(data: bytes) -> bytes:
    """a metrics file without its command line"""
    return data.split(b"\n", 2)[2]


def test_cli_dedup_and_dupmetrics_write_the_model_text(built, tmp_path):
    src = case_input(yhet(), tmp_path)
    out, met = tmp_path / "out.bam", tmp_path / "m.txt"
    args = ("dedup", "--nopg", "-v", "--metrics", met, "--optical-distance", 100, src, "-o", out)
    r = cli(*args)
    assert r.returncode == 0, r.stderr
    assert met.read_bytes() == model_text_of(out, 100, command_line(*args))
    line = [l for l in r.stderr.decode().splitlines() if l.startswith("[openge] MarkDuplicates: duplicate sets at optical distance 100, stage dup_sets ")]
    assert len(line) == 1 and " in a wave, 0 in a workgroup, 0 on the host" in line[0]
    r2 = cli("dupmetrics", "--optical-distance", 100, out)
    assert r2.returncode == 0 and r2.stdout == model_text_of(out, 100, command_line("dupmetrics", "--optical-distance", 100, out)), r2.stderr
    assert body(r2.stdout) == body(met.read_bytes())   # the same rows and histogram
    rows = DM.parse(DM_only(met.read_bytes()))[1]
    assert sum(int(x["READ_PAIR_OPTICAL_DUPLICATES"]) for x in rows) > 0 and b"all_sets\toptical_sets\tnon_optical_sets" in met.read_bytes()
    # without the new option: exactly section 26's bytes, and the same output file
    plain = ("dedup", "--nopg", "--metrics", tmp_path / "p.txt", src, "-o", tmp_path / "plain.bam")
    r = cli(*plain)
    assert r.returncode == 0 and (tmp_path / "p.txt").read_bytes() == section26_text_of(tmp_path / "plain.bam", command_line(*plain)), r.stderr
    assert (tmp_path / "plain.bam").read_bytes() == out.read_bytes()
    r = cli("dupmetrics", out)
    assert r.returncode == 0 and r.stdout == section26_text_of(out, command_line("dupmetrics", out)), r.stderr


def DM_only(data: bytes) -> bytes:
    """the part of a metrics file dupmetrics_model.parse reads: up to the histogram block"""
    return data.split(b"## HISTOGRAM")[0]


def test_cli_fused_sort_and_sam_input(ctx, built, tmp_path):
    src = case_input(yhet(), tmp_path)
    out, met = tmp_path / "o.bam", tmp_path / "m.txt"
    args = ("sort", "-M", "--nopg", "--metrics", met, "--optical-distance", 2500, src, "-o", out)
    r = cli(*args)
    assert r.returncode == 0, r.stderr
    assert met.read_bytes() == model_text_of(out, 2500, command_line(*args))
    args = ("sort", "-R", "--nopg", "--metrics", met, "--optical-distance", 2500, src, "-o", tmp_path / "removed.bam")
    r = cli(*args)   # counted before the removal: the same rows and histogram
    assert r.returncode == 0 and body(met.read_bytes()) == body(model_text_of(out, 2500, "x")), r.stderr
    header, records, _ = CASES["libs_rgs_tiles"]
    bam, sam = tmp_path / "in.bam", tmp_path / "in.sam"
    bamutil.write_bam_py(bam, header, K.REFS, records)
    recs, offs = bamutil.pack_records(records)
    topts, keep = L.text_opts([n for n, _ in K.REFS])
    sam.write_bytes(header.encode() + ctx.text_format(recs, offs, len(offs) - 1, topts))
    for f in (bam, sam):
        r = cli("dupmetrics", "-v", "--optical-distance", 100, f)
        assert r.returncode == 0 and r.stdout == model_text_of(bam, 100, command_line("dupmetrics", "-v", "--optical-distance", 100, f)), r.stderr
        assert "duplicate sets at optical distance 100" in r.stderr.decode()


def test_cli_refusals_write_nothing(built, tmp_path):
    src, out, met = tmp_path / "in.bam", tmp_path / "out.bam", tmp_path / "m.txt"
    header, records, _ = CASES["chain"]
    bamutil.write_bam_py(src, header, K.REFS, records)
    number = "--optical-distance needs a number from 0 to 2147483647"
    for args, msg in ((("dedup", "--optical-distance", 100, src, "-o", out), "openge dedup: --optical-distance needs --metrics (the optical duplicates go into the metrics file)"),
                      (("sort", "-M", "--optical-distance", 100, src, "-o", out), "openge mergesort: --optical-distance needs --metrics (the optical duplicates go into the metrics file)"),
                      (("dedup", "--gpus", 2, "--metrics", met, "--optical-distance", 100, src, "-o", out), "openge dedup: --optical-distance is not provided with --gpus"),
                      (("sort", "-M", "--gpus", 2, "--metrics", met, "--optical-distance", 100, src, "-o", out), "openge mergesort: --optical-distance is not provided with --gpus"),
                      (("dupmetrics", "--gpus", 2, "--optical-distance", 100, src), "openge dupmetrics: --gpus is not provided"),
                      (("dedup", "--split-chains", 4, "--metrics", met, "--optical-distance", 100, src, "-o", out),
                       "openge dedup: --optical-distance is not provided with split chains or --compat-nonverbose-dedup"),
                      (("dedup", "--compat-nonverbose-dedup", "--metrics", met, "--optical-distance", 100, src, "-o", out),
                       "openge dedup: --optical-distance is not provided with split chains or --compat-nonverbose-dedup"),
                      (("dedup", "--metrics", met, "--optical-distance", "-1", src, "-o", out), "openge dedup: " + number),
                      (("dedup", "--metrics", met, "--optical-distance", "2147483648", src, "-o", out), "openge dedup: " + number),
                      (("dedup", "--metrics", met, "--optical-distance", "12x", src, "-o", out), "openge dedup: " + number),
                      (("dedup", "--metrics", met, "--optical-distance=", src, "-o", out), "openge dedup: " + number),
                      (("dupmetrics", "--optical-distance", "far", src), "openge dupmetrics: " + number)):
        r = cli(*args)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr.decode().strip().splitlines()[-1] == msg, (args, r.stderr)
        assert not out.exists() and not met.exists(), args
    # the chunked path (an input larger than HBM; here a small OGE_CHUNK_BYTES): refused before the output is opened
    r = cli("sort", "-M", "--metrics", met, "--optical-distance", 100, src, "-o", out, env={"OGE_CHUNK_BYTES": "2000"})
    assert r.returncode != 0 and "--optical-distance needs the records resident in HBM" in r.stderr.decode(), r.stderr
    assert not out.exists() and not met.exists()
    r = cli("dedup", "--metrics", met, "--optical-distance", 2147483647, src, "-o", out)   # the largest distance
    assert r.returncode == 0 and met.exists(), r.stderr
