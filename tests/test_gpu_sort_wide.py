"""GPU: the coordinate sort key at the ends of its fields (sort.hip k_keypack, records.hip parse_input).

Key = size << 50 | refID << 33 | (pos + 1) << 1 | reverse, refID == -1 mapped to n_ref, n_ref < 131072,
block_size in [32, 10000].  The cases put refIDs above 2^16, positions at the top of 32 bits, ties at the
largest key, keys that vary in one bit or none (the varying-bits reduction picks the radix digits from
them), names on both sides of the 32-byte name slot and the extreme record sizes through ctx.sort_coord,
the device sort + gather, and (where the dedup layout takes the contig count) the fused sort + dedup
chain; all compared exactly with oracle.sort_perm / oracle.markdup.  Refusals are built from records that
are whole inside the buffer."""
import struct

import numpy as np
import pytest
import torch

import bamutil
import oracle
from bamutil import make_record, pack_records
from openge_amd import lib as L
from test_gpu_markdup_wide import LIMIT_MSG, _fused, no_bin, stream_with_marks

pytestmark = pytest.mark.gpu
NREF_MAX = 131071
INT_MAX = 2**31 - 1


def header(n_ref):
    return "@HD\tVN:1.4\tSO:unsorted\n" + "".join(f"@SQ\tSN:{i:x}\tLN:{INT_MAX}\n" for i in range(n_ref))


def placed(name, ref, pos, rev=False, flag=0, n=20):
    """an unmapped read placed at (ref, pos): the sort sees the coordinate, the dedup passes it through"""
    return make_record(name, 0x4 | flag | (0x10 if rev else 0), ref, pos, "", "A" * n, mapq=0)


def _gather(ctx, recs, offs, n, n_ref):
    tot = int(offs[n])
    d_recs = torch.from_numpy(recs.copy()).cuda()
    d_offs = torch.from_numpy(offs[:n + 1].astype(np.int64)).cuda()
    d_perm = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    d_out = torch.full((tot + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((n + 1,), -9, dtype=torch.int64, device="cuda")
    ctx.sort_coord_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, n_ref, d_perm.data_ptr())
    ctx.gather_records_dev(d_recs.data_ptr(), d_offs.data_ptr(), d_perm.data_ptr(), n, d_out.data_ptr(), d_oo.data_ptr())
    ctx.sync()
    return d_perm[:n].cpu().numpy().view(np.uint32), d_out[:tot].cpu().numpy().tobytes(), d_oo.cpu().numpy().view(np.uint64)


def check_sort(ctx, records, n_ref, fused=True):
    recs, offs = pack_records(records)
    n = len(records)
    operm = oracle.sort_perm(recs, offs, n)
    assert np.array_equal(ctx.sort_coord(recs, offs, n, n_ref), operm)
    srecs, soffs = pack_records([records[i] for i in operm])
    perm, out, oo = _gather(ctx, recs, offs, n, n_ref)
    assert np.array_equal(perm, operm) and np.array_equal(oo, soffs)
    assert no_bin(out, oo, n) == no_bin(srecs[:int(soffs[n])].tobytes(), soffs, n)
    hdr = header(min(n_ref, 4))  # no @RG: one library
    opts, keep = L.markdup_opts_from_header(hdr, n_ref)
    if not fused:  # the dedup's packed group key has no room for this many contigs; the sort alone has
        with pytest.raises(L.OgeError, match=LIMIT_MSG):
            _fused(ctx, recs, offs, n, opts)
        return operm
    odup, ond = oracle.markdup(srecs, soffs[:-1], n, hdr)
    nd, perm, out, oo = _fused(ctx, recs, offs, n, opts)
    assert np.array_equal(perm, operm) and np.array_equal(oo, soffs) and nd == ond
    assert no_bin(out, oo, n) == stream_with_marks(srecs, soffs, n, odup)
    return operm


def shuffled(records, seed):
    rng = np.random.default_rng(seed)
    return [records[i] for i in rng.permutation(len(records))]


POS_EDGES = [-1, 0, 2**29 - 1, 2**31 - 3, 2**31 - 2]


def test_refids_above_2_16_and_the_largest_key(ctx):
    """n_ref = 131071: refIDs on both sides of bit 16 and at the top, the refID -1 tail (mapped to n_ref, all 17
    bits set), every edge position on both strands, and ties at the largest key of all"""
    R = []
    for ref in (0, 65535, 65536, 131070):
        for pos in POS_EDGES:
            for rev in (False, True):
                for j in range(3):
                    R.append(placed(f"r{ref}p{pos}{'-+'[rev]}{j}", ref, pos, rev))
    # ties at the largest key (refID 131070, pos 2^31-2, reverse): by name, then flag, then input index
    for nm in ("t", "t1", "t10", "t2", "s", "u" * 40):
        for fl in (0, 0x1 | 0x40, 0x1 | 0x80, 0x200):
            for j in range(2):  # the same name and flag twice: input order decides
                R.append(placed(nm, 131070, 2**31 - 2, True, fl, n=10 + j))
    for j in range(40):
        R.append(placed(f"tail{j % 7}", -1, -1, bool(j & 1)))
    check_sort(ctx, shuffled(R, 1), NREF_MAX, fused=False)


def test_pos_edges_through_the_fused_chain(ctx):
    R = []
    for ref in (0, 2):
        for pos in POS_EDGES:
            for rev in (False, True):
                for j in range(4):
                    R.append(placed(f"p{ref}_{pos}_{int(rev)}_{j % 3}", ref, pos, rev, n=10 + j))
        for pos in (0, 2**29 - 1):  # mapped duplicates too: the dedup reads the same sorted keys as anchors
            for j in range(3):
                R.append(make_record(f"m{ref}_{pos}_{j}", 0, ref, pos, "30M", "C" * 30, bytes([20 + j] * 30)))
                R.append(make_record(f"n{ref}_{pos}_{j}", 0x10, ref, pos, "30M", "G" * 30, bytes([20 + j] * 30)))
    for j in range(9):
        R.append(placed(f"tail{j}", -1, -1))
    check_sort(ctx, shuffled(R, 2), 3)


@pytest.mark.parametrize("bit", [0, 32, 33, 49, None])
def test_keys_that_vary_in_one_bit_or_none(ctx, bit):
    """The radix sort takes its digits from the bits that vary over the input (OR ^ AND of the keys): one bit
    gives one digit, none gives no pass at all; the name / flag / index order inside the runs still holds."""
    a, b, n_ref = {None: ((1, 500, False), (1, 500, False), 3),
                   0: ((1, 500, False), (1, 500, True), 3),
                   32: ((1, -1, True), (1, INT_MAX, True), 3),      # pos + 1 = 0 and 2^31
                   33: ((0, 77, True), (1, 77, True), 3),
                   49: ((0, 77, False), (65536, 77, False), NREF_MAX)}[bit]
    rng = np.random.default_rng(5)
    R = []
    for j in range(150):
        ref, pos, rev = b if rng.integers(0, 2) else a
        R.append(placed(f"q{int(rng.integers(0, 60)):03d}", ref, pos, rev, int(rng.choice([0, 0x1 | 0x40, 0x1 | 0x80]))))
    operm = check_sort(ctx, R, n_ref, fused=n_ref == 3)
    assert not np.array_equal(operm, np.arange(len(R)))


def test_names_across_the_slot_edge_in_one_run(ctx):
    """name lengths 1, 31, 32, 33 and 254 (l_read_name 2 .. 255) with shared prefixes: the tie order compares the
    32-byte name slot when the name fits it and the record's bytes when it does not"""
    names = ["a", "b", "a" * 31, "a" * 30 + "b", "a" * 32, "a" * 31 + "b", "a" * 33, "a" * 32 + "b", "a" * 100,
             "a" * 253 + "b", "a" * 254, "a" * 31 + "\x7f", "a" * 32 + "\x01"]
    assert {len(x) for x in names} >= {1, 31, 32, 33, 254}
    R = []
    for k, nm in enumerate(names):
        for fl in (0, 0x1 | 0x40):
            R.append(placed(nm, 0, 1000, False, fl, n=8 + k % 3))
            R.append(placed(nm, 0, 1000, False, fl, n=12))  # full tie: input order
    R += [placed(f"bg{j}", 0, 900 + j * 7 % 200, bool(j & 1)) for j in range(60)]
    check_sort(ctx, shuffled(R, 3), 1)
    check_sort(ctx, shuffled(R[:len(names) * 4], 4), 1)  # the run alone: no key bit varies


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_inputs(ctx, n):
    R = [placed("x", 0, 5, True), placed("x", 0, 5, False)][:n]
    check_sort(ctx, R, 1)


def sized_record(name, ref, pos, block_size):
    """a mapped, well-formed record of exactly block_size bytes after the size word: one M op over the read"""
    fits = lambda nm: [x for x in range(block_size) if 32 + len(nm) + 1 + 4 + (x + 1) // 2 + x == block_size]
    if not fits(name):  # bases + qualities take 3 bytes per 2 reads: one more name byte reaches the sizes in between
        name += "_"
    ln = fits(name)[0]
    rec = make_record(name, 0, ref, pos, f"{ln}M", "ACGT" * (ln // 4) + "A" * (ln % 4), bytes([30] * ln))
    assert struct.unpack_from("<I", rec)[0] == block_size == len(rec) - 4
    return rec


def bare_record(ref, pos):
    """block_size 32: the fixed fields alone (no name, CIGAR, bases or tags); unmapped, placed"""
    body = struct.pack("<iiBBHHHiiii", ref, pos, 0, 0, 4680, 0, 0x4, 0, -1, -1, 0)
    return struct.pack("<I", len(body)) + body


def ordinary(n, seed):
    rng = np.random.default_rng(seed)
    return [make_record(f"o{j}", 0x10 * int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 5000)), "100M",
                        "ACGT" * 25, bytes(rng.integers(16, 40, 100, dtype=np.uint8).tolist()), tags=b"XAZ" + b"x" * 10 + b"\0")
            for j in range(n)]


def test_largest_and_smallest_record_among_ordinary_ones(ctx):
    """block_size 10000 and 32: the size payload in key bits [50, 64) gives the output offsets, and the gather
    moves a 10 KB record between 200-byte ones"""
    R = ordinary(300, 6)
    assert 180 <= len(R[0]) <= 220
    R.insert(100, sized_record("big", 0, 2500, 10000))
    R.insert(200, sized_record("big2", 1, 0, 10000))
    R.insert(50, bare_record(0, 2500))
    R.insert(250, bare_record(1, 4999))
    R.append(bare_record(-1, -1))
    check_sort(ctx, R, 2)


# ------------------------------------------------------------------------------------------- refusals
def _refused(ctx, records, n_ref, match, code, fused=True):
    recs, offs = pack_records(records)
    n = len(records)
    with pytest.raises(L.OgeError, match=rf"error {code}: .*{match}"):
        ctx.sort_coord(recs, offs, n, n_ref)
    with pytest.raises(L.OgeError, match=rf"error {code}: .*{match}"):
        _gather(ctx, recs, offs, n, n_ref)
    if fused:
        opts, keep = L.markdup_opts_from_header(header(1), n_ref)
        with pytest.raises(L.OgeError, match=rf"error {code}: .*{match}"):
            _fused(ctx, recs, offs, n, opts)


BAD = {
    "refid_eq_n_ref": (lambda: placed("bad", 2, 10), "refID outside"),
    "refid_minus_2": (lambda: placed("bad", -2, 10), "refID outside"),
    "pos_minus_2": (lambda: placed("bad", 1, -2), "pos < -1"),
    "block_size_10001": (lambda: sized_record("bad", 1, 10, 10001), "block_size outside"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_records_are_refused(ctx, what):
    make, match = BAD[what]
    good = ordinary(40, 7)
    _refused(ctx, good[:20] + [make()] + good[20:], 2, match, -1)
    check_sort(ctx, good, 2)  # the context works afterwards


def test_too_many_contigs_for_the_sort_key(ctx):
    good = ordinary(40, 8)
    _refused(ctx, good, 131072, "n_ref outside", -3, fused=False)
    check_sort(ctx, good, 2)
    check_sort(ctx, good, NREF_MAX, fused=False)
