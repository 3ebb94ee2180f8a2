"""How the inflate cuts a stream into phase-1 launches: chunks of whole rounds of the resident decoder lanes
(oge_infl_plan; the context counters infl_chunks / infl_rounds / infl_lanes report what a call ran).

Rounds show at small sizes through the per-call knobs OGE_INFL_WGS (caps the phase-1 workgroups: 2 -> 128 lanes)
and OGE_INFL_BUDGET (the workspace budget in blocks).  Every expected output is the input data itself; the BGZF
blocks are made with host zlib and hold 300..2,000 payload bytes, so hundreds of blocks are well under a MB."""
import re
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as D

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
LANES = 128
NBLKS = [1, 127, 128, 129, 256, 257, 3 * 128 + 17]


def _member(payload: bytes, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return D.bgzf_member(payload, c.compress(payload) + c.flush())


_SMALL = {}


def _small():
    """401 blocks of 300..2,000 bytes (text-like, ~4 bits a byte): -> (payloads, members)."""
    if not _SMALL:
        rng = np.random.default_rng(401)
        src = bytes(rng.integers(0, 16, 900_000, dtype=np.uint8) + 65)
        pay, at = [], 0
        for n in rng.integers(300, 2_001, max(NBLKS)):
            pay.append(src[at:at + int(n)])
            at += int(n)
        _SMALL["pay"], _SMALL["mem"] = pay, [_member(p) for p in pay]
    return _SMALL["pay"], _SMALL["mem"]


def _stream(n: int) -> tuple[bytes, bytes]:
    pay, mem = _small()
    return b"".join(pay[:n]), b"".join(mem[:n]) + EOF_BLOCK


def _rounds(sizes, lanes=LANES):
    """Sum over launches of ceil(nb / min(lanes, 64 * workgroups launched))."""
    return sum(-(-nb // min(lanes, 64 * -(-nb // 64))) for nb in sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [128, 256])
@pytest.mark.parametrize("nblk", NBLKS)
def test_whole_round_shapes(ctx, monkeypatch, budget, nblk):
    from openge_amd import lib as L
    monkeypatch.setenv("OGE_INFL_WGS", str(LANES // 64))
    monkeypatch.setenv("OGE_INFL_BUDGET", str(budget))
    monkeypatch.delenv("OGE_INFL_PLAN", raising=False)
    data, z = _stream(nblk)
    got = ctx.bgzf_inflate(z)
    lanes, chunks, rounds = ctx.counter("infl_lanes"), ctx.counter("infl_chunks"), ctx.counter("infl_rounds")
    print(f"nblk {nblk} budget {budget}: lanes {lanes} chunks {chunks} rounds {rounds}")
    assert got == data
    plan = L.infl_plan(nblk, LANES, budget)
    assert lanes == LANES
    assert rounds == -(-nblk // LANES)
    assert chunks == len(plan) == -(-nblk // budget)
    # the same stream under the plan of before: the same bytes, its own chunking
    monkeypatch.setenv("OGE_INFL_PLAN", "balanced")
    assert ctx.bgzf_inflate(z) == data
    old = L.infl_plan(nblk, LANES, budget, balanced=True)
    assert ctx.counter("infl_chunks") == len(old)
    assert ctx.counter("infl_rounds") == _rounds(old) >= rounds


@pytest.mark.gpu
def test_unknown_plan_is_an_error(ctx, monkeypatch):
    from openge_amd import lib as L
    monkeypatch.setenv("OGE_INFL_PLAN", "fastest")
    with pytest.raises(L.OgeError, match="OGE_INFL_PLAN"):
        ctx.bgzf_inflate(_stream(3)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["whole", "balanced"])
def test_mixed_block_lengths(ctx, monkeypatch, plan):
    """Full 65,280-byte payloads among tiny ones in one stream, three rounds of 128 lanes: the queue hands a
    lane that finished a tiny block the next one while its neighbours are still in a full block."""
    monkeypatch.setenv("OGE_INFL_WGS", str(LANES // 64))
    monkeypatch.setenv("OGE_INFL_BUDGET", "256")
    monkeypatch.setenv("OGE_INFL_PLAN", plan)
    rng = np.random.default_rng(65280)
    full = bytes(rng.integers(0, 16, 65_280 + 300 * 64, dtype=np.uint8) + 97)
    pay, _ = _small()
    data, z = [], []
    for k in range(300):
        p = full[64 * k:64 * k + 65_280] if k % 9 == 4 or k in (0, 127, 128, 299) else pay[k][:1 + k % 700]
        data.append(p)
        z.append(_member(p, 1))
    assert sum(len(p) == 65_280 for p in data) >= 34
    assert ctx.bgzf_inflate(b"".join(z) + EOF_BLOCK) == b"".join(data)
    assert ctx.counter("infl_rounds") == (3 if plan == "whole" else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [130, 255, 390, 400])
def test_error_names_the_block_of_a_later_chunk(ctx, monkeypatch, bad):
    """401 blocks in chunks of 128, 128, 128 and 17: a flipped stored CRC in the second chunk (130, 255) and in
    the last (390, 400) is reported with the block's index in the stream, and the next call decodes."""
    from openge_amd import lib as L
    monkeypatch.setenv("OGE_INFL_WGS", str(LANES // 64))
    monkeypatch.setenv("OGE_INFL_BUDGET", "128")
    monkeypatch.delenv("OGE_INFL_PLAN", raising=False)
    pay, mem = _small()
    assert L.infl_plan(401, LANES, 128) == [128, 128, 128, 17]
    m = bytearray(mem[bad])
    m[-8] ^= 0x10  # the stored CRC-32
    z = b"".join(mem[:bad]) + bytes(m) + b"".join(mem[bad + 1:401]) + EOF_BLOCK
    with pytest.raises(L.OgeError) as e:
        ctx.bgzf_inflate(z)
    got = re.search(r"BGZF block (\d+) failed", str(e.value))
    assert got and int(got.group(1)) == bad, str(e.value)
    assert "CRC" in str(e.value)
    data, good = _stream(401)
    assert ctx.bgzf_inflate(good) == data


@pytest.mark.gpu
def test_consecutive_calls_on_one_context(built, monkeypatch):
    """A larger stream, a smaller one and the larger one again on a context of their own, with unequal chunks
    (256 + 145, then 128 + 1 in the same buffers, then 128 + 128 + 128 + 17): phase 1 of each call and chunk
    relies on the bitmap words the launches before it left clear."""
    from openge_amd import lib as L
    monkeypatch.setenv("OGE_INFL_WGS", str(LANES // 64))
    monkeypatch.delenv("OGE_INFL_PLAN", raising=False)
    c = L.Context(0)
    try:
        for nblk, budget, chunks in [(401, 256, 2), (129, 128, 2), (401, 128, 4), (257, 256, 2), (401, 256, 2)]:
            monkeypatch.setenv("OGE_INFL_BUDGET", str(budget))
            data, z = _stream(nblk)
            assert c.bgzf_inflate(z) == data, (nblk, budget)
            assert c.counter("infl_chunks") == chunks
            assert c.counter("infl_rounds") == -(-nblk // LANES)
    finally:
        c.close()


@pytest.mark.parametrize("lanes", [1, 3, 4])
def test_plan_function(built, lanes):
    """oge_infl_plan alone (host arithmetic, no device): the sizes sum to nblk, every chunk but the last is
    R * lanes blocks with R = clamp(budget // lanes, 1, max per lane), the last holds the rest, and the rounds
    -- the sum of ceil(size / lanes) -- are ceil(nblk / lanes), the fewest possible, for any budget."""
    from openge_amd import lib as L
    for per_lane in (1, 2, 4):
        for budget in (0, 1, lanes, lanes + 1, 2 * lanes, 3 * lanes - 1, 3 * lanes, 100 * lanes):
            r = min(max(budget // lanes, 1), per_lane)
            for nblk in range(0, 5 * lanes + 2):
                sizes = L.infl_plan(nblk, lanes, budget, per_lane)
                what = (lanes, per_lane, budget, nblk, sizes)
                assert sum(sizes) == nblk, what
                assert all(s == r * lanes for s in sizes[:-1]), what
                assert not sizes or 1 <= sizes[-1] <= r * lanes, what
                assert len(sizes) == -(-nblk // (r * lanes)), what
                assert sum(-(-s // lanes) for s in sizes) == -(-nblk // lanes), what
                # the plan of before: equal chunks within the budget; never fewer rounds
                old = L.infl_plan(nblk, lanes, budget, per_lane, balanced=True)
                most = max(lanes, min(per_lane * lanes, budget))
                assert sum(old) == nblk and all(1 <= s <= most for s in old), (what, old)
                assert len(old) == -(-nblk // most), (what, old)
                assert sum(-(-s // lanes) for s in old) >= -(-nblk // lanes), (what, old)
    assert L.infl_plan(1_306_019, 196_608, 343_565) == [196_608] * 6 + [126_371]
    assert L.infl_plan(1_306_019, 196_608, 10 ** 9) == [786_432, 519_587]  # max_per_lane 0: the build's four
    assert L.infl_plan(1_306_019, 196_608, 343_565, balanced=True) == [326_505] * 3 + [326_504]
