"""GPU: `openge compare` computed on the device (csrc/compare.hip: oge_compare_dev, its host-buffer form, the lib.py
wrappers and the CLI command) equals the Python restatement (tests/compare_model.py) on every crafted case, whatever
the width of the hash, and the command's stdout, stderr and exit status equal what the reference gave
(tests/golden/compare/manifest.json) byte for byte.

Neither the symbols nor the command exist before this feature: every test here fails without it."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import compare_cases as K
import compare_model as M
from goldens import GOLDEN
from openge_amd import lib as L
from test_compare_model import CASES, MANIFEST, crafted, input_file
from test_gpu_cli import OPENGE
from test_qc_model import same

pytestmark = pytest.mark.gpu

BITS = (-1, 4, 0)  # the full hash, 4 bits, none: the result is the same
N_REF = len(K.REFS)


def dev(recs: np.ndarray, offs: np.ndarray):
    """(device records, device offsets): keep both alive while the pointers are in use."""
    return torch.from_numpy(np.ascontiguousarray(recs)).cuda(), torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()).cuda()


def regions_of(name):
    strings = CASES[name][2]
    return [M.NO_REGION] if not strings else [M.parse_region(rs, K.REFS)[0] for rs in strings]


@functools.lru_cache(maxsize=None)
def model(name, region):
    (ra, oa), (rb, ob) = crafted(name)
    return M.compare(M.elements(ra, oa, region), M.elements(rb, ob, region))


def ordered(diff):
    """the decoded image -> the model's form and order: additions first, each side by the elements' order"""
    ent = [(side, refid, pos, surplus, tuple((op >> 4, M.TYPES[op & 0xF]) for op in ops)) for side, refid, pos, surplus, ops in diff]
    return sorted(ent, key=lambda e: (-e[0], M.order_key((e[1], e[2], e[4]))))


def check(got: dict, want: dict, what):
    for k in ("n_ref", "n_other", "common", "additions", "deletions"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    if "diff" in got:
        assert ordered(got["diff"]) == M.diff_entries(want), what
        assert got["diff_entries"] == len(got["diff"])


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", list(CASES))
def test_compare_equals_the_model_in_every_form(ctx, name, bits):
    """Equal and empty sets, multiplicities 3 v 5 and 5 v 3, a pile of 200 reads with three CIGARs of one op count,
    40 such CIGARs, 70 ops that differ in the last one, 16 and 17 ops (one lane / the wave), every type at one
    length, reads without ops, refID -1 and pos -1, reads on both region bounds, overlapping regions, three contigs,
    a run over lane 64, thread 256, record 1024 and key 4096 of the sorted union, unsorted input.  Device records
    and host buffers, with and without the diff, give the model's counts and diff at every hash width."""
    (ra, oa), (rb, ob) = crafted(name)
    da, db = dev(ra, oa), dev(rb, ob)
    for rg in regions_of(name):
        want = model(name, rg)
        args = (da[0].data_ptr(), da[1].data_ptr(), len(oa), db[0].data_ptr(), db[1].data_ptr(), len(ob), N_REF)
        plain = ctx.compare_dev(*args, region=rg, hash_bits=bits)
        check(plain, want, (rg, "counts"))
        full = ctx.compare_dev(*args, region=rg, diff=True, hash_bits=bits)
        check(full, want, (rg, "diff"))
        assert full["hard_runs"] == plain["hard_runs"]
        if bits == -1:
            assert full["hard_runs"] == 0  # 47 bits: no collision among a handful of CIGARs
        check(ctx.compare(ra, oa, len(oa), rb, ob, len(ob), N_REF, region=rg, diff=True, hash_bits=bits), want, (rg, "host"))
        back = ctx.compare_dev(*args[3:6], *args[0:3], N_REF, region=rg, hash_bits=bits)  # the sets swapped
        assert (back["additions"], back["deletions"], back["common"]) == (want["deletions"], want["additions"], want["common"])


@pytest.mark.parametrize("bits", (4, 0))
def test_the_collision_path_ran(ctx, bits):
    """With the hash narrowed, runs that hold several CIGARs are decided by the ops alone: hard_runs counts them."""
    for name in ("pile200", "pile40"):
        (ra, oa), (rb, ob) = crafted(name)
        da, db = dev(ra, oa), dev(rb, ob)
        got = ctx.compare_dev(da[0].data_ptr(), da[1].data_ptr(), len(oa), db[0].data_ptr(), db[1].data_ptr(), len(ob), N_REF, diff=True, hash_bits=bits)
        assert got["hard_runs"] > 0 and ctx.counter("compare_hash_bits") == bits, (name, bits)
        check(got, model(name, M.NO_REGION), (name, bits))
    if bits == 0:
        for name in K.hard_cases():
            (ra, oa), (rb, ob) = crafted(name)
            da, db = dev(ra, oa), dev(rb, ob)
            assert ctx.compare_dev(da[0].data_ptr(), da[1].data_ptr(), len(oa), db[0].data_ptr(), db[1].data_ptr(), len(ob), N_REF,
                                   hash_bits=0)["hard_runs"] > 0, name


def test_diff_renders_to_the_model_lines(ctx):
    """The decoded and ordered image, printed once per surplus element, is the text of -p."""
    for name in ("types", "pile200", "wide70", "no_ops"):
        (ra, oa), (rb, ob) = crafted(name)
        da, db = dev(ra, oa), dev(rb, ob)
        got = ctx.compare_dev(da[0].data_ptr(), da[1].data_ptr(), len(oa), db[0].data_ptr(), db[1].data_ptr(), len(ob), N_REF, diff=True)
        names = [n for n, _ in K.REFS]
        lines = "".join(f"{'Add' if side else 'Del'}: {M.element_text((refid, pos, ops), names)}\n" * surplus
                        for side, refid, pos, surplus, ops in ordered(got["diff"]))
        want, _err, _st = M.run([("a", ra, oa), ("b", rb, ob)], K.REFS, None, True)
        assert want.startswith(lines) and want[len(lines):].count("\n") == 1, name  # then the summary line


def test_input_files_against_each_other(ctx):
    """simple.bam, 208.yhet.bam and the records of simple.sam: every ordered pair, whole and by region"""
    sets = {n: input_file(n) for n in ("simple.bam", "208.yhet.bam", "simple.sam")}
    devs = {n: dev(v[1], v[2]) for n, v in sets.items()}
    for a, (refs, ra, oa) in sets.items():
        for b, (_r, rb, ob) in sets.items():
            for rg in (M.NO_REGION, M.parse_region("YHet:0..300", refs)[0]):
                want = M.compare(M.elements(ra, oa, rg), M.elements(rb, ob, rg))
                got = ctx.compare_dev(devs[a][0].data_ptr(), devs[a][1].data_ptr(), len(oa), devs[b][0].data_ptr(), devs[b][1].data_ptr(), len(ob),
                                      len(refs), region=rg, diff=True)
                check(got, want, (a, b, rg))


def test_geometry_timing_and_nothing_carried_over(ctx):
    (ra, oa), (rb, ob) = crafted("ladder")
    da, db = dev(ra, oa), dev(rb, ob)
    args = (da[0].data_ptr(), da[1].data_ptr(), len(oa), db[0].data_ptr(), db[1].data_ptr(), len(ob), N_REF)
    first = ctx.compare_dev(*args, diff=True)
    assert (ctx.counter("compare_tile_records"), ctx.counter("compare_wide_ops")) == (K.TILE_RECORDS, K.WIDE_OPS)
    assert ctx.counter("compare_items") == len(oa) + len(ob) and ctx.timing("compare") > 0
    ctx.compare_dev(*args[:3], None, None, 0, N_REF)  # a smaller call in between
    again = ctx.compare_dev(*args, diff=True)
    assert {k: v for k, v in again.items() if k != "diff"} == {k: v for k, v in first.items() if k != "diff"}
    assert ordered(again["diff"]) == ordered(first["diff"])


def test_refusals_of_the_entry_points(ctx):
    recs, offs = K.pack([K.rec(0, 5, "4M"), K.rec(3, 5, "4M"), K.rec(-1, -1, "")])
    d = dev(recs, offs)
    args = (d[0].data_ptr(), d[1].data_ptr(), 3)
    with pytest.raises(L.OgeError, match=r"error -1: .*record 1 of the first set .*refID outside \[0, n_ref\)"):
        ctx.compare_dev(*args, *args, N_REF)
    assert ctx.compare_dev(*args, *args, N_REF, region=(0, 0, 2, 10))["common"] == 1  # outside the region: not looked at
    assert ctx.compare_dev(*args, *args, 4)["common"] == 2
    bad = bytearray(K.rec(0, 5, "4M"))
    struct.pack_into("<I", bad, 36 + 3, (4 << 4) | 9)  # name "r0\0": the first op gets code 9
    brecs, boffs = K.pack([K.rec(0, 5, "4M"), bytes(bad)])
    b = dev(brecs, boffs)
    with pytest.raises(L.OgeError, match=r"error -1: .*record 1 of the first set has a CIGAR op code above 8"):
        ctx.compare_dev(b[0].data_ptr(), b[1].data_ptr(), 2, *args, N_REF, region=(0, 0, 2, 10))
    rg, res = L.CompareRegion(*M.NO_REGION), L.CompareResult()
    call = L.lib().oge_compare_dev
    assert call(ctx.h, None, None, 0, None, None, 0, N_REF, C.byref(rg), 2, -1, C.byref(res), None, None) == -1      # unknown request bit
    assert call(ctx.h, None, None, 0, None, None, 0, N_REF, C.byref(rg), L.COMPARE_DIFF, -1, C.byref(res), None, None) == -1  # nowhere to put it
    assert call(ctx.h, None, None, 0, None, None, 0, N_REF, C.byref(rg), 0, -1, C.byref(res), None, None) == 0
    assert ctx.compare_dev(*args, *args, 4)["common"] == 2  # the context still works


# ------------------------------------------------------------------------------------------------ the CLI
def cli(*args, cwd=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env=dict(os.environ), cwd=cwd)


def check_cli(key, cwd):
    g = MANIFEST[key]
    r = cli("compare", *g["args"], cwd=cwd)
    assert r.returncode == g["status"], (key, r.returncode, r.stderr)
    assert same(g["stdout"], r.stdout), (key, r.stdout[:2000])
    assert same(g["stderr"], r.stderr), (key, r.stderr[:2000])


@pytest.mark.parametrize("key", sorted(k for k, v in MANIFEST.items() if v["dir"] == "inputs"))
def test_cli_on_the_input_files_prints_the_reference_text(key):
    """simple.bam, 208.yhet.bam and simple.sam in both orders and against themselves, three inputs, -p, regions
    (a contig, a range, a point, overlapping ones) and the region strings the reference rejects with status 255"""
    check_cli(key, GOLDEN / "inputs")


@pytest.mark.parametrize("name", ["types", "pile200", "wide70", "no_ops", "unplaced", "bounds", "contigs", "unsorted", "straddle1024", "empty_ref"])
def test_cli_on_crafted_files_prints_the_reference_text(name, tmp_path):
    ra, rb, _regions = CASES[name]
    bamutil.write_bam_py(tmp_path / "a.bam", K.header_text(), K.REFS, ra)
    bamutil.write_bam_py(tmp_path / "b.bam", K.header_text(), K.REFS, rb)
    check_cli(f"case_{name}", tmp_path)
    check_cli(f"case_{name}_print", tmp_path)


SIMPLE = GOLDEN / "inputs" / "simple.bam"


def test_cli_same_file_twice_prints_nothing():
    r = cli("compare", SIMPLE, SIMPLE)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    r = cli("compare", "-p", "-r", "YHet", SIMPLE, SIMPLE)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")


@pytest.mark.parametrize("args,msg", [
    (("compare", SIMPLE, "stdin"), "openge compare: stdin is not provided"),
    (("compare", "-", SIMPLE), "openge compare: stdin is not provided"),
    (("compare",), "openge compare: stdin is not provided"),
    (("compare", "--gpus", "2", SIMPLE, SIMPLE), "openge compare: --gpus is not provided"),
    (("compare", "-q", "3", SIMPLE, SIMPLE), "unrecognised option"),
])
def test_cli_refusals(args, msg):
    r = cli(*args)
    assert r.returncode != 0 and msg in r.stderr.decode() and r.stdout == b"", (r.returncode, r.stderr)
    assert len(r.stderr.decode().strip().splitlines()) == 1


def test_cli_verbose_reports_the_split_and_a_differing_dictionary_warns(tmp_path):
    r = cli("compare", "-v", SIMPLE, GOLDEN / "inputs" / "208.yhet.bam")
    assert r.returncode == 0 and r.stdout == b"\t   15409 added\t       0 removed\n"
    assert b"[openge] compare: read + inflate" in r.stderr and b"on the device" in r.stderr
    bamutil.write_bam_py(tmp_path / "a.bam", K.header_text(), K.REFS, [K.rec(0, 1, "4M")])
    bamutil.write_bam_py(tmp_path / "b.bam", K.header_text(K.REFS[:2]), K.REFS[:2], [K.rec(0, 1, "4M")])
    r = cli("compare", "a.bam", "b.bam", cwd=tmp_path)  # the reference compares file 0's dictionary with itself: silent
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    r = cli("compare", "-v", "a.bam", "b.bam", cwd=tmp_path)
    assert (r.returncode, r.stdout) == (0, b"")
    assert b"Sequence dictionaries between a.bam and b.bam differ. This may produce inconsistent results.\n" in r.stderr
    missing = cli("compare", SIMPLE, tmp_path / "missing.bam")
    assert missing.returncode != 0 and missing.stdout == b""
