"""GPU: `openge stats`, `count` and `coverage` computed on the device (csrc/qc.hip: oge_stats_dev, oge_coverage_dev,
their host-buffer and whole-file forms, the CLI commands and the lib.py wrappers) equal the Python restatement
(tests/qc_model.py) on every crafted case, on the two input BAMs and on synthetic sets, and the commands' text
equals what the reference printed (tests/golden/qc/manifest.json) byte for byte.

None of the symbols or commands exist before this feature: every test here fails without it."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import qc_cases as K
import qc_model as M
from goldens import GOLDEN, load_case
from openge_amd import lib as L
from test_gpu_cli import OPENGE
from test_qc_model import FILES, MANIFEST, file_case, same

pytestmark = pytest.mark.gpu

WALK_LIMIT = 10_000  # the whole-file entry points' record walk takes records up to this many bytes
STATS = K.stats_cases()
COVER = K.coverage_cases()


def dev(recs: np.ndarray, offs: np.ndarray):
    """(device records, device offsets): keep both alive while the pointers are in use."""
    return torch.from_numpy(np.ascontiguousarray(recs)).cuda(), torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64).copy()).cuda()


def check_stats(got: dict, want: dict, inserts: bool, lengths: bool, what=""):
    for k in M.COUNTERS + ("sorted", "n_insert", "insert_sum"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    if inserts:
        assert (got["insert_mid_lo"], got["insert_mid_hi"]) == (want["insert_mid_lo"], want["insert_mid_hi"]), what
    if lengths:
        assert np.array_equal(got["lengths"][0], want["lengths"][0]) and np.array_equal(got["lengths"][1], want["lengths"][1]), what


@functools.lru_cache(maxsize=None)
def stats_case(name):
    refs, records = STATS[name]
    recs, offs = K.pack(records)
    return refs, records, recs, offs, M.stats(recs, offs)


def small(records) -> bool:
    return all(len(r) <= WALK_LIMIT for r in records)


# ------------------------------------------------------------------------------------------------ stats
@pytest.mark.parametrize("name", list(STATS))
def test_stats_equal_the_model_in_every_form(ctx, name, tmp_path):
    """n = 0, 1, 63..65, 255..257 and one more than a workgroup's records; all 512 flag combinations; violating
    triples, run starts and refID decreases on every wave-step, wave-range and workgroup edge, with predecessors a
    whole workgroup back; l_seq 0 / 1, 3000 distinct lengths, 70,000 bases; 0..4 inserts, ties, radix digit edges,
    2^31.  Device records, host buffers and the whole file give the model's result."""
    refs, records, recs, offs, want = stats_case(name)
    d_recs, d_off = dev(recs, offs)
    for ins, lens in ((False, False), (True, True), (True, False), (False, True)):
        check_stats(ctx.stats_dev(d_recs.data_ptr(), d_off.data_ptr(), len(offs), inserts=ins, lengths=lens), want, ins, lens, (ins, lens))
    check_stats(ctx.stats(recs, offs, len(offs), inserts=True, lengths=True), want, True, True, "host")
    if small(records):
        bam = K.bam_bytes(refs, records, tmp_path)
        check_stats(ctx.bam_stats(bam, inserts=True, lengths=True), want, True, True, "file")
        assert ctx.bam_count(bam) == len(records)
        if name in MANIFEST["stats"]:  # ... and renders to the reference's bytes
            out, err = M.stats_text(ctx.bam_stats(bam, inserts=True, lengths=True), True, True)
            assert same(MANIFEST["stats"][name]["stdout"], out.encode()) and same(MANIFEST["stats"][name]["stderr"], err.encode())


def test_kernel_geometry_is_what_the_cases_assume(ctx):
    _refs, _records, recs, offs, _w = stats_case("n1")
    d_recs, d_off = dev(recs, offs)
    ctx.stats_dev(d_recs.data_ptr(), d_off.data_ptr(), 1)
    assert (ctx.counter("qc_wave_records"), ctx.counter("qc_block_records"), ctx.counter("qc_length_table")) == (K.WAVE_RECS, K.BLOCK_RECS,
                                                                                                              K.LEN_TAB)
    assert ctx.timing("qc_stats") > 0
    ctx.coverage_dev(d_recs.data_ptr(), d_off.data_ptr(), 1, [1 << 29], 100)
    assert (ctx.counter("qc_cov_tile_records"), ctx.counter("qc_cov_window")) == (K.COV_TILE, K.COV_WIN)
    assert ctx.timing("qc_coverage") > 0


@pytest.fixture(scope="module")
def inputs():
    """{name: (refs, recs, offs)} of the two input BAMs and two synthetic sets, shared and never changed."""
    out = {k: file_case(k) for k in FILES}
    for k in ("mix3k", "c2_20k"):
        c = load_case(k)
        refs = [tuple(f.split(":", 1)[1] for f in line.split("\t")[1:3]) for line in c.header.splitlines() if line.startswith("@SQ")]
        out[k] = ([(n, int(ln)) for n, ln in refs], c.recs, c.offs[:-1])
    return out


@pytest.mark.parametrize("name", ["simple", "yhet208", "mix3k", "c2_20k"])
def test_stats_of_input_files_and_synthetic_sets(ctx, inputs, name):
    _refs, recs, offs = inputs[name]
    want = M.stats(recs, offs)
    d_recs, d_off = dev(recs, offs)
    a = ctx.stats_dev(d_recs.data_ptr(), d_off.data_ptr(), len(offs), inserts=True, lengths=True)
    check_stats(a, want, True, True)
    b = ctx.stats_dev(d_recs.data_ptr(), d_off.data_ptr(), len(offs), inserts=True, lengths=True)  # nothing carried over
    check_stats(b, want, True, True)
    if name in FILES:
        data = (GOLDEN / "inputs" / FILES[name]).read_bytes()
        check_stats(ctx.bam_stats(data, inserts=True, lengths=True), want, True, True)
        assert ctx.bam_count(data) == len(offs)
        assert ctx.last_refs()[0] == [n for n, _ in _refs]


def test_stats_rejects_unknown_request_bits(ctx):
    st = L.BamStats()
    assert L.lib().oge_stats_dev(ctx.h, None, None, 0, 4, C.byref(st), None, None) == -1
    assert L.lib().oge_stats_dev(ctx.h, None, None, 0, L.STATS_LENGTHS, C.byref(st), None, None) == -1  # nowhere to put them


# ------------------------------------------------------------------------------------------------ coverage
def device_sparse(ctx, ptr: int, nb: int):
    """Non-zero bins of a device bin array, found on the device."""
    t = torch.empty(max(nb, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the copy runs on the context's stream, not on torch's
    L.check(L.lib().oge_memcpy(ctx.h, t.data_ptr(), ptr, 4 * nb, 3), ctx.h)
    nz = torch.nonzero(t[:nb]).flatten()
    return nz.cpu().numpy(), (t[:nb][nz].cpu().numpy().astype(np.int64) & 0xFFFFFFFF)


def check_coverage_dev(ctx, recs, offs, lens, bs):
    g, v, sk = M.coverage_sparse(M.cores(recs, offs), lens, bs)
    d_recs, d_off = dev(recs, offs)
    for _ in range(2):  # the second call starts from clean bins
        ptr, nb, gsk, ov = ctx.coverage_dev(d_recs.data_ptr(), d_off.data_ptr(), len(offs), lens, bs, fetch=False)
        assert nb == int(M.coverage_layout(lens, bs)[-1]) and gsk == sk and not ov
        gg, gv = device_sparse(ctx, ptr, nb)
        assert np.array_equal(gg, g) and np.array_equal(gv, v), (bs, gg[:5], g[:5], gv[:5], v[:5])
    return g, v, sk


@pytest.mark.parametrize("bs", K.BINSIZES)
@pytest.mark.parametrize("name", list(COVER))
def test_coverage_equals_the_model_in_every_form(ctx, name, bs, tmp_path):
    """Bin sizes 1, 7, 100, larger than a contig and 2^30; pos 0, the contig's last bin, a read past it and one at a
    negative position (dropped), l_seq 0, 5000 identical reads, 70,000 bases at bin size 1, unsorted reads over
    more bins than one window, a sorted set with one wide tile, placed unmapped reads, header order chrB chrA,
    a contig without reads, n_ref 0."""
    refs, records, _d = COVER[name]
    recs, offs = K.pack(records)
    names, lens = [n for n, _ in refs], [ln for _, ln in refs]
    g, v, sk = check_coverage_dev(ctx, recs, offs, lens, bs)
    nb = int(M.coverage_layout(lens, bs)[-1])
    want = M.dense(g, v, nb)
    bins, gsk, ov = ctx.coverage(recs, offs, len(offs), lens, bs)
    assert np.array_equal(bins, want) and gsk == sk and not ov
    if small(records):
        fn, fl, base, bins, gsk, ov = ctx.bam_coverage(K.bam_bytes(refs, records, tmp_path), bs)
        assert fn == names and fl.tolist() == lens and base.tolist() == M.coverage_layout(lens, bs).tolist()
        assert np.array_equal(bins, want) and gsk == sk and not ov
        key = f"{bs}_nz"
        if name in MANIFEST["coverage"] and key in MANIFEST["coverage"][name]:
            tsv, err = M.coverage_text(names, lens, bs, bins, gsk, omit_uncovered=True)
            assert same(MANIFEST["coverage"][name][key]["tsv"], tsv.encode()) and same(MANIFEST["coverage"][name][key]["stderr"], err.encode())


@pytest.mark.parametrize("bs", [1, 7, 100])
@pytest.mark.parametrize("name", ["simple", "yhet208", "mix3k", "c2_20k"])
def test_coverage_of_input_files_and_synthetic_sets(ctx, inputs, name, bs):
    refs, recs, offs = inputs[name]
    check_coverage_dev(ctx, recs, offs, [ln for _, ln in refs], bs)


def test_coverage_overflow_is_flagged(ctx):
    """Four reads of 2^30 positions in one bin of 2^30 bases reach 2^32: flagged; three do not and are exact."""
    def reads(k):
        out = []
        for i in range(k):
            r = bytearray(K.rec(i, 0, 0, lseq=4))
            struct.pack_into("<i", r, 4 + 16, (1 << 30) - 1)  # l_seq: only the record core is read
            out.append(bytes(r))
        return K.pack(out)
    for k, flagged in ((3, False), (4, True)):
        recs, offs = reads(k)
        d_recs, d_off = dev(recs, offs)
        bins, sk, ov = ctx.coverage_dev(d_recs.data_ptr(), d_off.data_ptr(), k, [(1 << 31) - 1], 1 << 30)
        assert ov == flagged and sk == 0
        if not flagged:
            assert bins.tolist() == [3 << 30, 0]


def test_coverage_refusals(ctx, tmp_path):
    recs, offs = K.pack([K.rec(0, 0, 5), K.rec(1, 3, 5)])
    d_recs, d_off = dev(recs, offs)
    with pytest.raises(L.OgeError, match="error -1: .*binsize"):
        ctx.coverage_dev(d_recs.data_ptr(), d_off.data_ptr(), 2, [1000], 0)
    with pytest.raises(L.OgeError, match=r"error -1: .*record 1 has a refID outside"):
        ctx.coverage_dev(d_recs.data_ptr(), d_off.data_ptr(), 2, [1000], 100)
    with pytest.raises(L.OgeError, match="error -3: .*--binsize"):   # 300 contigs of 2^31-1 bases: 2.6 TB of bins
        ctx.coverage_dev(d_recs.data_ptr(), d_off.data_ptr(), 1, [(1 << 31) - 1] * 300, 1)
    bins, sk, ov = ctx.coverage_dev(d_recs.data_ptr(), d_off.data_ptr(), 1, [1000], 100)  # the context still works
    assert bins.tolist() == [11] + [0] * 9
    dup = K.bam_bytes([("c", 1000), ("d", 1000), ("c", 500)], [K.rec(0, 0, 5)], tmp_path)
    with pytest.raises(L.OgeError, match="error -1: .*two contigs are named c"):
        ctx.bam_coverage(dup, 100)
    with pytest.raises(L.OgeError, match="error -1"):
        ctx.bam_coverage(dup, 0)


# ------------------------------------------------------------------------------------------------ the CLI
def cli(*args):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, timeout=300, env=dict(os.environ))


def case_file(kind: str, name: str, tmp_path):
    if name in FILES:
        return GOLDEN / "inputs" / FILES[name]
    refs, records = STATS[name] if kind == "stats" else COVER[name][:2]
    p = tmp_path / "in.bam"
    bamutil.write_bam_py(p, K.header_text(refs), refs, records)
    return p


@pytest.mark.parametrize("name", ["simple", "yhet208", "flags512", "n1", f"n{K.BLOCK_RECS + 1}", "sorted_three_ok", "sorted_three_bad",
                                  "sorted_block_back_bad", "len_3000", "ins_ties", "ins_n0"])
def test_cli_stats_and_count_print_the_reference_text(name, tmp_path):
    src = case_file("stats", name, tmp_path)
    g = MANIFEST["stats"][name]
    r = cli("stats", "-I", "-L", src)
    assert r.returncode == 0, r.stderr
    assert same(g["stdout"], r.stdout), r.stdout.decode()
    assert same(g["stderr"], r.stderr), r.stderr.decode()
    plain = cli("stats", src)
    assert plain.returncode == 0 and plain.stderr == b""
    head = r.stdout[:r.stdout.index(b"\n", r.stdout.index(b"Sorted:")) + 1]  # without -I / -L: up to the Sorted line
    assert plain.stdout == head
    total = int(r.stdout.split(b"\n")[0].split()[-1])
    c = cli("count", src)
    assert (c.returncode, c.stdout, c.stderr) == (0, b"%d\n" % total, b"")


def test_cli_stats_of_an_empty_file(tmp_path):
    """Zero reads: status 0 and the counters (the reference's -nan% is not pinned)."""
    p = tmp_path / "e.bam"
    bamutil.write_bam_py(p, K.header_text(K.REFS1), K.REFS1, [])
    r = cli("stats", "-I", "-L", p)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(b"Total reads:                0\n") and b"Sorted:                   Yes\n" in r.stdout
    assert r.stdout.endswith(b"Insert size (absolute value):\n") and b"'Proper-pairs'" not in r.stdout
    assert cli("count", p).stdout == b"0\n"


@pytest.mark.parametrize("name", ["simple", "yhet208", "basic", "name_order", "unsorted_wide", "n_ref0"])
def test_cli_coverage_writes_the_reference_table(name, tmp_path):
    src = case_file("coverage", name, tmp_path)
    for key, g in MANIFEST["coverage"][name].items():
        bs, mode = key.split("_")
        if name == "yhet208" and key not in ("100_zero", "100_nz", "1_nz"):
            continue
        out = tmp_path / "cov.tsv"
        r = cli("coverage", "-b", bs, *(["--omituncoveredbases"] if mode == "nz" else []), "-o", out, src)
        assert r.returncode == 0, r.stderr
        assert same(g["tsv"], out.read_bytes()), key
        assert same(g["stderr"], r.stderr), (key, r.stderr.decode())
        assert r.stdout == b""
    r = cli("coverage", src)  # no -o: only the summary, bin size 100
    assert r.returncode == 0 and r.stdout == b"" and same(MANIFEST["coverage"][name]["100_nz"]["stderr"], r.stderr)
    r = cli("coverage", "--binsize=7", "-o", "stdout", src)
    assert r.returncode == 0 and r.stdout == b"" and same(MANIFEST["coverage"][name]["7_nz"]["stderr"], r.stderr)


SIMPLE = GOLDEN / "inputs" / "simple.bam"


@pytest.mark.parametrize("args,msg", [
    (("stats",), "openge stats: one BAM file is required"),
    (("stats", SIMPLE, SIMPLE), "openge stats: one BAM file is required"),
    (("stats", "-"), "openge stats: one BAM file is required"),
    (("count", "stdin"), "openge count: one BAM file is required"),
    (("count", "--gpus", "2", SIMPLE), "openge count: --gpus is not provided"),
    (("coverage",), "openge coverage: one BAM file is required"),
    (("coverage", "-V", SIMPLE), "are not provided"),
    (("coverage", "--strict", SIMPLE), "are not provided"),
    (("coverage", "-b", "0", SIMPLE), "--binsize must be at least 1"),
    (("stats", "--gpus=3", SIMPLE), "openge stats: --gpus is not provided"),
    (("count", "-I", SIMPLE), "unrecognised option"),
])
def test_cli_refusals(args, msg):
    r = cli(*args)
    assert r.returncode != 0 and msg in r.stderr.decode() and r.stdout == b"", (r.returncode, r.stderr)
    assert len(r.stderr.decode().strip().splitlines()) == 1


def test_cli_coverage_failed_write_is_an_error(tmp_path):
    r = cli("coverage", "-o", tmp_path / "no_such_dir" / "c.tsv", SIMPLE)
    assert r.returncode != 0 and b"error writing" in r.stderr
    missing = cli("stats", tmp_path / "missing.bam")
    assert missing.returncode != 0 and missing.stdout == b""
