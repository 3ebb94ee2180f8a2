"""GPU: the BAM index built on the device (oge_bai_build_dev, oge_bam_index_dev, the chain's build_index, the
CLI's --index and `openge index`) equals the Python restatement of its definition (tests/bai_model.py) byte
for byte, and finds the records a brute-force scan finds."""
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import bai_cases as K
import bai_model as M
from goldens import GOLDEN, load_case
from openge_amd import lib as L
from test_gpu_cli import OPENGE, case_input

pytestmark = pytest.mark.gpu


def dev_u64(a) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def build_dev(ctx, raw: bytes, offs, n_ref: int, base: int, uoff, cstart) -> bytes:
    """oge_bai_build_dev on the records raw[offs[i]:] (record 0 at stream position `base`)."""
    d_recs = torch.from_numpy(np.frombuffer(raw + b"\0" * 16, np.uint8).copy()).cuda()
    d_off, d_u, d_c = dev_u64(list(offs) or [0]), dev_u64(uoff), dev_u64(cstart)
    return ctx.bai_build_dev(d_recs.data_ptr(), d_off.data_ptr(), len(offs), n_ref, base, d_u.data_ptr(), d_c.data_ptr(),
                             len(uoff) - 1)


def build_dev_from_bam(ctx, bam: bytes) -> bytes:
    raw = M.inflate_all(bam)
    n_ref, base, offs = M.stream_layout(raw)
    uoff, cstart = M.block_table(bam)
    return build_dev(ctx, raw, offs, n_ref, base, uoff, cstart)


def check_queries(bai: bytes, bam: bytes, n_ref: int, regions: int = 40) -> None:
    M.check_invariants(bai)
    idx, rd, rng = M.parse(bai), M.Reader(bam), random.Random(7)
    for r in range(n_ref):
        assert M.query(idx, bam, r, 0, 1 << 29, rd) == M.brute(bam, r, 0, 1 << 29)
    for _ in range(regions if n_ref else 0):
        r, beg = rng.randrange(n_ref), rng.randrange(0, 3_000_000)
        end = beg + rng.choice((1, 500, 30_000, 1_000_000))
        assert M.query(idx, bam, r, beg, end, rd) == M.brute(bam, r, beg, end), (r, beg, end)


# ------------------------------------------------------------------------------ crafted cases
@pytest.mark.parametrize("payload", [700, 65280])
@pytest.mark.parametrize("name", list(K.CRAFTED))
def test_crafted_cases_equal_the_model(ctx, name, payload):
    """Empty (n = 0, 3 references), one record, unmapped only; records straddling every bin level's edge via N
    and D, pos 0, rend == 2^29, 10I5S, a 0x4 record on a reference; references without reads first, in the
    middle and last; empty linear windows leading and inside; one record over 40 windows."""
    refs, recs = K.CRAFTED[name]()
    bam = K.make_bam(refs, recs, payload)
    want = M.build_from_bam(bam)
    assert build_dev_from_bam(ctx, bam) == want
    assert ctx.bam_index(bam) == want            # the whole-file entry point: same image
    assert ctx.last_bai() == want
    check_queries(want, bam, len(refs))


def test_host_buffer_form_equals_the_model(ctx):
    refs, recs = K.refs_and_gaps()
    bam = K.make_bam(refs, recs, 700)
    raw = M.inflate_all(bam)
    n_ref, base, offs = M.stream_layout(raw)
    uoff, cstart = M.block_table(bam)
    a = np.frombuffer(raw[base:] + b"\0" * 16, np.uint8).copy()
    got = ctx.bai_build(a, np.array(offs, np.uint64) - np.uint64(base), len(offs), n_ref, base, uoff, cstart)
    assert got == M.build_from_bam(bam)


def test_record_past_the_bai_limit_fails(ctx):
    refs, recs = K.over_limit()  # rend == 2^29 + 1
    with pytest.raises(L.OgeError, match=r"error -3: .*record 1 "):
        build_dev_from_bam(ctx, K.make_bam(refs, recs))
    with pytest.raises(L.OgeError, match="no index"):
        ctx.last_bai()
    refs, recs = K.one_record()
    bam = K.make_bam(refs, recs)
    raw = M.inflate_all(bam)
    _n, base, offs = M.stream_layout(raw)
    with pytest.raises(L.OgeError, match="error -3"):   # n_ref < 0
        build_dev(ctx, raw, offs, -1, base, *M.block_table(bam))


@pytest.mark.parametrize("payload", [700, 4096, 65280])
def test_block_layouts_equal_the_model(ctx, payload):
    """A record ending exactly on a payload boundary, a record over three blocks, a bin revisited within one
    block (merged) and in a later block (not merged) -- tests/test_bai_model.py checks that the files are
    what they claim."""
    refs, recs, _idx = K.block_layout(payload, 140_000 if payload == 65280 else None)
    bam = K.make_bam(refs, recs, payload)
    want = M.build_from_bam(bam)
    bins = M.parse(want)["refs"][0]["bins"]
    assert len(bins[4681]) == 1 and len(bins[4682]) == 2
    assert build_dev_from_bam(ctx, bam) == want
    if payload < 65280:  # the record walk of the whole-file entry point takes records up to 10,000 bytes
        assert ctx.bam_index(bam) == want
    check_queries(want, bam, 1, regions=20)


# ------------------------------------------------------------------------------ sizes across tile edges
@pytest.fixture(scope="module")
def sorted_sets(ctx):
    """Synthetic c1 sets through oge_sort_markdup_dev: {pairs: (device records, device offsets, host records,
    host offsets)}; shared by the size cases, never changed."""
    out = {}
    for pairs in (513, 35_001):
        p = L.synth_params(pairs, preset="c1", seed=77)
        recs, offs, hdr = L.synth_host(p)
        n = 2 * pairs
        d_recs = torch.from_numpy(recs).cuda()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        d_perm = torch.empty(n, dtype=torch.int32, device="cuda")
        d_out = torch.zeros(int(offs[-1]) + 16, dtype=torch.uint8, device="cuda")
        d_oo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        opts, keep = L.markdup_opts_from_header(hdr, p.n_ref)
        ctx.sort_markdup_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_perm.data_ptr(), d_out.data_ptr(), d_oo.data_ptr())
        ctx.sync()
        out[pairs] = (d_out, d_oo, d_out.cpu().numpy().tobytes(), d_oo.cpu().numpy().view(np.uint64))
    return out


def irregular_table(total: int, seed: int):
    """A block table with payloads of 1..65536 bytes and uneven compressed sizes covering `total` bytes."""
    rng = random.Random(seed)
    uoff, cstart, u, c = [], [], 0, 0
    while u < total:
        uoff.append(u)
        cstart.append(c)
        u += rng.choice((1, 700, 65280, 65536, rng.randint(1, 65536)))
        c += rng.randint(30, 70_000)
    return uoff + [u], cstart + [c]


@pytest.mark.parametrize("n", [255, 256, 257, 1025, 70_001])
def test_sizes_across_tile_edges(ctx, sorted_sets, n):
    """The first n sorted reads of a synthetic set: 255 / 256 / 257 around one workgroup, 1025 just past one
    tile of the running maximum, 70,001 with more runs than one workgroup handles; the block table is
    irregular, and the records start at a stream position of their own."""
    d_out, d_oo, raw, oo = sorted_sets[513 if n <= 1026 else 35_001]
    base = 4321
    end = int(oo[n])
    uoff, cstart = irregular_table(base + end, seed=n)
    d_u, d_c = dev_u64(uoff), dev_u64(cstart)
    got = ctx.bai_build_dev(d_out.data_ptr(), d_oo.data_ptr(), n, 1, base, d_u.data_ptr(), d_c.data_ptr(), len(uoff) - 1)
    want = M.build(raw, oo[:n], 1, base, uoff, cstart)
    assert got == want
    M.check_invariants(got)
    if n == 70_001:
        assert sum(len(c) for c in M.parse(got)["refs"][0]["bins"].values()) > 256
        # nothing proportional to the records, runs or windows is still held: the image, the 32-byte error
        # words and the per-reference tables (9 u64 for the reference and 9 for the end entry), each with the
        # workspace's 64 bytes of slack
        held = ctx.counter("bai_ws_held")
        assert held is not None and held <= len(got) + 32 + 9 * 2 * 8 + 3 * 64, held
        free0, _ = ctx.mem_info()
        ctx.bai_build_dev(d_out.data_ptr(), d_oo.data_ptr(), n, 1, base, d_u.data_ptr(), d_c.data_ptr(), len(uoff) - 1)
        free1, _ = ctx.mem_info()
        assert free0 - free1 < 4 << 20, (free0, free1)   # a second build keeps no more than the first


def test_unsorted_input_fails_with_the_record_index(ctx):
    refs, recs = K.bin_edges()
    recs[3], recs[4] = recs[4], recs[3]
    with pytest.raises(L.OgeError, match=r"error -1: .*record 4 is out of order"):
        build_dev_from_bam(ctx, K.make_bam(refs, recs))
    refs, recs = K.refs_and_gaps()  # a placed read behind the unplaced ones
    with pytest.raises(L.OgeError, match=rf"error -1: .*record {len(recs)} is out of order"):
        build_dev_from_bam(ctx, K.make_bam(refs, recs + [K.rec("late", 4, 5)]))


# ------------------------------------------------------------------------------ the chain
def chain(ctx, z: bytes, **over):
    dz = torch.from_numpy(np.frombuffer(z + b"\0" * 8, np.uint8).copy()).cuda()
    d, ob, nr, nd = ctx.mergesort_bgzf_dev(dz.data_ptr(), len(z), L.mergesort_opts(program_line=None, **over))
    return ctx._fetch(d, ob), nr


@pytest.mark.parametrize("dedup", [False, True], ids=["sort", "-M-R"])
@pytest.mark.parametrize("name", ["c2_20k", "simple", "yhet208"])
def test_chain_builds_the_index_of_the_file_it_returns(ctx, name, dedup, tmp_path):
    z = open(case_input(load_case(name), tmp_path), "rb").read()
    over = dict(mark_duplicates=1, remove_duplicates=1) if dedup else {}
    plain, _ = chain(ctx, z, **over)
    with pytest.raises(L.OgeError, match="no index"):
        ctx.last_bai()
    out, n = chain(ctx, z, build_index=1, **over)
    bai = ctx.last_bai()
    assert out == plain                                  # the file does not change
    assert bai == M.build_from_bam(out)
    assert ctx.timing("bai_build") > 0
    assert ctx.bam_index(out) == bai
    raw = M.inflate_all(out)
    n_ref, _b, offs = M.stream_layout(raw)
    assert len(offs) == n
    check_queries(bai, out, n_ref, regions=30)


def test_chain_paths_without_an_index_refuse(ctx):
    z = (GOLDEN / "inputs" / "simple.bam").read_bytes()
    hz = np.frombuffer(z, np.uint8).copy()
    out = np.empty(1 << 22, np.uint8)
    with pytest.raises(L.OgeError, match="error -1: index not provided on this path"):
        ctx.mergesort_bgzf_host(hz.ctypes.data, len(z), L.mergesort_opts(program_line=None, build_index=1), out.ctypes.data, out.nbytes)


# ------------------------------------------------------------------------------ the CLI
def cli(*args, env=None):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, text=True, timeout=300, env={**os.environ, **(env or {})})


def test_cli_index_option_and_index_command(tmp_path):
    src = case_input(load_case("c2_20k"), tmp_path)
    seg = {"OGE_WRITE_SEG_BLOCKS": "1"}  # several deflate segments for 40,000 reads
    for extra, tag in (((), "s"), (("-M", "-R"), "r")):
        a, b = tmp_path / f"{tag}_plain.bam", tmp_path / f"{tag}_index.bam"
        assert cli("mergesort", "--nopg", *extra, src, "-o", a, env=seg).returncode == 0
        r = cli("mergesort", "--nopg", "--index", *extra, src, "-o", b, env=seg)
        assert r.returncode == 0, r.stderr
        bam = b.read_bytes()
        assert bam == a.read_bytes() and not (tmp_path / f"{tag}_plain.bam.bai").exists()
        want = M.build_from_bam(bam)
        assert (tmp_path / f"{tag}_index.bam.bai").read_bytes() == want
        r = cli("index", b, "-o", tmp_path / "x.bai")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "x.bai").read_bytes() == want
    # dedup of the sorted file, default name of `openge index`
    d = tmp_path / "d.bam"
    r = cli("dedup", "--nopg", "--index", tmp_path / "s_index.bam", "-o", d)
    assert r.returncode == 0, r.stderr
    want = M.build_from_bam(d.read_bytes())
    assert (tmp_path / "d.bam.bai").read_bytes() == want
    os.remove(tmp_path / "d.bam.bai")
    assert cli("index", d).returncode == 0
    assert (tmp_path / "d.bam.bai").read_bytes() == want


@pytest.mark.parametrize("args,env", [
    (("mergesort", "--index"), None),                                   # output to stdout
    (("mergesort", "--index", "--gpus", "2", "-o", "OUT"), None),
    (("mergesort", "--index", "-b", "-o", "OUT"), None),                # sort by name
    (("mergesort", "--index", "-o", "OUT"), {"OGE_CHUNK_BYTES": "200000"}),   # chunked output
    (("mergesort", "--index", "-o", "OUT"), {"OGE_BGZF_CODEC": "libdeflate"}),  # the host writer
], ids=["stdout", "gpus", "byname", "chunked", "host-writer"])
def test_cli_index_refused_combinations(tmp_path, args, env):
    out = tmp_path / "o.bam"
    r = cli(*[out if a == "OUT" else a for a in args], "--nopg", GOLDEN / "inputs" / "simple.bam", env=env)
    assert r.returncode != 0 and "--index is not provided" in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / "o.bam.bai").exists() and not out.exists()


def test_cli_failed_write_leaves_no_index(tmp_path):
    out = tmp_path / "o.bam"
    r = cli("mergesort", "--index", "--nopg", GOLDEN / "inputs" / "simple.bam", "-o", out, env={"OGE_TEST_FAIL": "write_device"})
    assert r.returncode != 0 and not (tmp_path / "o.bam.bai").exists()
