"""GPU: duplicate marking at real-genome contig and library counts (markdup_wide_cases.py).

The packed group keys of the device MarkDuplicates (md_keys.h: frag_key; markdup.hip: pair_entry and the
windowed readers k_frag_win / k_pair_win / k_win_collect) place the library and refID fields by sb = bits
for n_ref and lb = bits for the largest library id, sb + lb <= 13.  Every path is run on the sets below
(sb + lb = 12), at (11+2, 10+3, 12+1) and above (12+2, 11+3) that limit and compared exactly with the oracle:
sort permutation, dup bytes, the count and the output records.  test_markdup_wide_cases.py shows, without a
GPU, that the oracle's marks on these sets change when any twin pair of groups is merged."""
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch

import bamutil
import markdup_wide_cases as W
import oracle
from goldens import load_case
from openge_amd import lib as L

pytestmark = pytest.mark.gpu
OPENGE = str(L.PKG / "openge")
LIMIT_MSG = "references x libraries"
ERR_LIMIT, ERR_ARG = -3, -1


class Ref:
    """One set with its oracle results, computed once."""

    def __init__(self, name):
        s = W.get(name)
        self.s, self.n, self.header, self.n_ref = s, len(s.records), s.header, s.n_ref
        self.recs, self.offs = bamutil.pack_records(s.records)
        self.operm = oracle.sort_perm(self.recs, self.offs, self.n)
        self.srecs, self.soffs = bamutil.pack_records([s.records[i] for i in self.operm])
        self.odup, self.ond = oracle.markdup(self.srecs, self.soffs[:-1], self.n, s.header)
        self.odup_in, self.ond_in = oracle.markdup(self.recs, self.offs[:-1], self.n, s.header)
        self.sorted_marked = stream_with_marks(self.srecs, self.soffs, self.n, self.odup)

    def opts(self, **kw):
        return L.markdup_opts_from_header(self.header, self.n_ref, **kw)


def stream_with_marks(recs, offs, n, dup):
    """the records with 0x400 set where dup == 1 and cleared where dup == 0, bin zeroed (the gather recomputes it)"""
    out = recs[:int(offs[n])].copy()
    for k in range(n):
        o = int(offs[k])
        out[o + 14:o + 16] = 0
        if dup[k] != 2:
            out[o + 19] = (int(out[o + 19]) & 0xFB) | (0x04 if dup[k] == 1 else 0)
    return out.tobytes()


def no_bin(buf: bytes, offs, n) -> bytes:
    out = np.frombuffer(buf, np.uint8).copy()
    for k in range(n):
        o = int(offs[k])
        out[o + 14:o + 16] = 0
    return out.tobytes()


_refs = {}


def ref_of(name) -> Ref:
    if name not in _refs:
        _refs[name] = Ref(name)
    return _refs[name]


@pytest.fixture(scope="module", params=W.ACCEPTED)
def wide(request, built):
    return ref_of(request.param)


def test_sets_are_the_checked_ones(wide):
    """the sets the CPU test vouches for: construction == oracle, here once more on the sorted stream"""
    assert np.array_equal(wide.odup, np.array(wide.s.expect, np.uint8)[wide.operm])
    assert np.array_equal(wide.odup_in, np.array(wide.s.expect, np.uint8))
    assert wide.s.sb + wide.s.lb in (12, 13) and 0 < wide.ond < wide.n


def test_markdup_host_entry_sorted_and_unsorted(ctx, wide):
    opts, keep = wide.opts()
    dup, nd = ctx.markdup(wide.srecs, wide.soffs, wide.n, opts)
    assert nd == wide.ond and np.array_equal(dup, wide.odup)
    dup, nd = ctx.markdup(wide.recs, wide.offs, wide.n, opts)
    assert nd == wide.ond_in and np.array_equal(dup, wide.odup_in)


def _inplace(ctx, recs, offs, n, opts):
    d_recs = torch.from_numpy(recs.copy()).cuda()
    d_offs = torch.from_numpy(offs[:n + 1].astype(np.int64)).cuda()
    d_dup = torch.full((n + 1,), 0xAB, dtype=torch.uint8, device="cuda")
    nd = ctx.markdup_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_dup.data_ptr(), apply=True)
    ctx.sync()
    return nd, d_dup[:n].cpu().numpy(), d_recs.cpu().numpy(), ctx.counter("md_inplace_window")


def test_markdup_dev_in_place_windowed_and_sorted_paths(ctx, wide, monkeypatch):
    opts, keep = wide.opts()
    tot = int(wide.soffs[wide.n])
    nd1, dup1, out1, win1 = _inplace(ctx, wide.srecs, wide.soffs, wide.n, opts)
    assert win1 == 1
    monkeypatch.setenv("OGE_MD_INPLACE_WINDOW", "0")
    nd0, dup0, out0, win0 = _inplace(ctx, wide.srecs, wide.soffs, wide.n, opts)
    monkeypatch.delenv("OGE_MD_INPLACE_WINDOW")
    assert not win0
    for nd, dup, out in ((nd1, dup1, out1), (nd0, dup0, out0)):
        assert nd == wide.ond and np.array_equal(dup, wide.odup)
        assert no_bin(out[:tot].tobytes(), wide.soffs, wide.n) == wide.sorted_marked
    assert out1.tobytes() == out0.tobytes()


def _fused(ctx, recs, offs, n, opts):
    tot = int(offs[n])
    d_recs = torch.from_numpy(recs.copy()).cuda()
    d_offs = torch.from_numpy(offs[:n + 1].astype(np.int64)).cuda()
    d_perm = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_out = torch.full((tot + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((n + 1,), -9, dtype=torch.int64, device="cuda")
    nd = ctx.sort_markdup_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_perm.data_ptr(), d_out.data_ptr(),
                              d_oo.data_ptr())
    ctx.sync()
    return nd, d_perm.cpu().numpy().view(np.uint32), d_out[:tot].cpu().numpy().tobytes(), d_oo.cpu().numpy().view(np.uint64)


def _check_fused(wide, res):
    nd, perm, out, oo = res
    assert np.array_equal(perm, wide.operm)
    assert np.array_equal(oo, wide.soffs)
    assert nd == wide.ond
    fl = bamutil.flags_of(np.frombuffer(out, np.uint8), oo[:wide.n])
    assert np.array_equal((fl & 0x400) != 0, wide.odup == 1)
    assert no_bin(out, oo, wide.n) == wide.sorted_marked


def test_fused_chain_four_modes(ctx, wide, monkeypatch):
    """windowed mate join + windowed groups (default), the sort-based groups, the window-overflow path and
    the sort-based mate join: one answer"""
    opts, keep = wide.opts()
    res = {"default": _fused(ctx, wide.recs, wide.offs, wide.n, opts)}
    opts.debug_sort_groups = 1
    res["sort_groups"] = _fused(ctx, wide.recs, wide.offs, wide.n, opts)
    opts.debug_sort_groups = 0
    for env in ("OGE_MD_WINCAP=1", "OGE_MD_MATEWIN=0"):
        k, v = env.split("=")
        monkeypatch.setenv(k, v)
        res[env] = _fused(ctx, wide.recs, wide.offs, wide.n, opts)
        monkeypatch.delenv(k)
    for mode, r in res.items():
        _check_fused(wide, r)
        assert r[0] == res["default"][0] and r[2] == res["default"][2], mode
        assert np.array_equal(r[1], res["default"][1]) and np.array_equal(r[3], res["default"][3]), mode


def test_split_chains_at_the_limit(ctx, built):
    """w13a with the reference's split-by-chromosome chains (refID % 3): the chain id joins the packed keys"""
    w = ref_of("w13a")
    odup, ond = oracle.markdup(w.srecs, w.soffs[:-1], w.n, w.header, split_chains=3)
    opts, keep = w.opts(split_chains=3)
    dup, nd = ctx.markdup(w.srecs, w.soffs, w.n, opts)
    assert nd == ond and np.array_equal(dup, odup)
    nd, perm, out, oo = _fused(ctx, w.recs, w.offs, w.n, opts)
    assert nd == ond and np.array_equal(perm, w.operm)
    assert no_bin(out, oo, w.n) == stream_with_marks(w.srecs, w.soffs, w.n, odup)


# ------------------------------------------------------------------------------------------- refusals
def _raises(match, code):
    return pytest.raises(L.OgeError, match=rf"error {code}: .*{match}")


def _refused_everywhere(ctx, recs, offs, n, opts, match, code):
    """the three entry points refuse with the message, and leave every output buffer as it was"""
    with _raises(match, code):
        ctx.markdup(recs, offs, n, opts)
    tot = int(offs[n])
    d_recs = torch.from_numpy(recs.copy()).cuda()
    d_offs = torch.from_numpy(offs[:n + 1].astype(np.int64)).cuda()
    d_dup = torch.full((n + 1,), 0xAB, dtype=torch.uint8, device="cuda")
    with _raises(match, code):
        ctx.markdup_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_dup.data_ptr(), apply=True)
    ctx.sync()
    assert bool((d_dup == 0xAB).all()) and d_recs.cpu().numpy().tobytes() == recs.tobytes()
    d_perm = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_out = torch.full((tot + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((n + 1,), -9, dtype=torch.int64, device="cuda")
    with _raises(match, code):
        ctx.sort_markdup_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_perm.data_ptr(), d_out.data_ptr(),
                             d_oo.data_ptr())
    ctx.sync()
    assert bool((d_perm == -7).all()) and bool((d_out == 0xCD).all()) and bool((d_oo == -9).all())
    assert d_recs.cpu().numpy().tobytes() == recs.tobytes()


def _w12_still_works(ctx):
    w = ref_of("w12")
    opts, keep = w.opts()
    dup, nd = ctx.markdup(w.srecs, w.soffs, w.n, opts)
    assert nd == w.ond and np.array_equal(dup, w.odup)
    _check_fused(w, _fused(ctx, w.recs, w.offs, w.n, opts))


@pytest.mark.parametrize("name", W.REFUSED)
def test_layouts_past_the_limit_are_refused(ctx, name):
    s = W.get(name)
    assert s.sb + s.lb == 14
    recs, offs = bamutil.pack_records(s.records)
    opts, keep = L.markdup_opts_from_header(s.header, s.n_ref)
    _refused_everywhere(ctx, recs, offs, len(s.records), opts, LIMIT_MSG, ERR_LIMIT)
    _w12_still_works(ctx)


def test_read_group_table_refusals(ctx):
    w = ref_of("w12")
    opts, keep = w.opts()
    big = 32768
    ids = np.frombuffer(b"".join(b"g%05d\0" % i for i in range(big)) + b"\0", np.uint8).copy()
    libs = np.ones(big + 1, np.int16)
    o = L.MarkdupOpts()
    o.n_ref, o.rg_ids, o.rg_ids_bytes, o.rg_lib, o.n_rg, o.unknown_lib = w.n_ref, ids.ctypes.data, len(ids) - 1, libs.ctypes.data, big, 2
    _refused_everywhere(ctx, w.recs, w.offs, w.n, o, "more than 32767 read groups", ERR_LIMIT)
    o.n_rg = 2
    libs[1] = -1
    _refused_everywhere(ctx, w.recs, w.offs, w.n, o, "negative library id", ERR_ARG)
    libs[1] = 1
    o.unknown_lib = -1
    _refused_everywhere(ctx, w.recs, w.offs, w.n, o, "negative library id", ERR_ARG)
    # ids that end before the second one's NUL: the backing array keeps that byte, nothing outside it is read
    ids2 = np.frombuffer(b"g1\0g2\0", np.uint8).copy()
    o.unknown_lib, o.rg_ids, o.rg_ids_bytes = 2, ids2.ctypes.data, 5
    _refused_everywhere(ctx, w.recs, w.offs, w.n, o, "not n_rg NUL-terminated", ERR_ARG)
    _w12_still_works(ctx)


# ------------------------------------------------------------------------------------------------ CLI
def _cli(*args):
    return subprocess.run([OPENGE, *map(str, args)], capture_output=True, text=True, timeout=300, env=dict(os.environ))


def _digests(path):
    h, _, recs, offs = bamutil.read_bam(path)
    hm, tail = hashlib.sha256(), []
    for o in offs:
        rb = bamutil.rec_bytes(recs, o)
        (tail.append(rb) if int.from_bytes(rb[4:8], "little", signed=True) == -1 else hm.update(rb))
    return h, hm.hexdigest(), hashlib.sha256(b"".join(sorted(tail))).hexdigest()


def _write_set(name, path):
    s = W.get(name)
    bamutil.write_bam_py(path, s.header, s.refs, s.records)
    return s


def test_cli_at_the_limit_equals_the_reference(built, tmp_path):
    """`openge dedup` (input order) and `openge mergesort -M` on w13a against the reference's own outputs"""
    case = load_case("wide2047")
    _write_set("w13a", tmp_path / "in.bam")
    for args, key in ((("dedup", "--nopg"), "dedup_input_v"), (("mergesort", "-M", "--nopg"), "sortdedup_v")):
        out = tmp_path / f"{key}.bam"
        r = _cli(*args, tmp_path / "in.bam", "-o", out)
        assert r.returncode == 0, r.stderr
        h, m, t = _digests(out)
        g = case.meta[key]
        assert h == g["header"] and m == g["mapped_sha256"] and t == g["tail_multiset_sha256"], key
        _, _, recs, offs = bamutil.read_bam(out)
        assert np.array_equal(np.nonzero(bamutil.flags_of(recs, offs) & 0x400)[0], case.arrays[key])


def test_cli_past_the_limit(built, tmp_path):
    """dedup and mergesort -M fail cleanly on w14a; sort alone does not inherit the dedup limit"""
    s = _write_set("w14a", tmp_path / "in.bam")
    for args in (("dedup", "--nopg"), ("mergesort", "-M", "--nopg")):
        out = tmp_path / f"{args[0]}.bam"
        r = _cli(*args, tmp_path / "in.bam", "-o", out)
        assert r.returncode != 0 and LIMIT_MSG in r.stderr, (r.returncode, r.stderr)
        assert not out.exists() and not list(tmp_path.glob(f"{args[0]}.bam*"))
    r = _cli("sort", "--nopg", tmp_path / "in.bam", "-o", tmp_path / "s.bam")
    assert r.returncode == 0, r.stderr
    _, _, srecs, soffs = bamutil.read_bam(tmp_path / "s.bam")
    recs, offs = bamutil.pack_records(s.records)
    n = len(s.records)
    assert len(soffs) == n
    assert np.array_equal(bamutil.perm_of(srecs, soffs, recs, offs[:-1]), oracle.sort_perm(recs, offs, n))
