"""GPU: the input side of inflate phase 1 (k_infl_huff's bit reservoir: registers topped up inside a decode
iteration, memory read at one wave-wide reload point per iteration, the chunk taken one iteration later).

Every expected output is the input data itself, and every crafted deflate stream is first inflated on the
CPU (zlib.decompressobj(-15)), so a bad fixture fails as a fixture.  All cases run with the header pre-pass
off and on (OGE_INFL_PREP)."""
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as D

pytestmark = pytest.mark.gpu

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
PREPS = ["0", "1"]


def _deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def _member(payload: bytes, body: bytes) -> bytes:
    """One BGZF block; the body is checked on the CPU first."""
    assert zlib.decompressobj(-15).decompress(body) == payload, "fixture: the deflate body does not give the payload"
    return D.bgzf_member(payload, body)


def _bgzf(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, pay=65280, eof=True) -> bytes:
    out = [_member(data[i:i + pay], _deflate(data[i:i + pay], level, strategy)) for i in range(0, len(data), pay)]
    return b"".join(out) + (EOF_BLOCK if eof else b"")


# ---------------------------------------------------------------------------- greediest iterations
LEN_BASE = {284: 227}   # length symbol 284: 227..257, 5 extra bits
DIST_BASE = {28: 16385, 29: 24577}  # 13 extra bits each


def _greedy_block(seed: int, size: int = 40_000) -> tuple[bytes, bytes]:
    """A dynamic-Huffman block whose iterations consume close to the 120-bit maximum, many in a row: six
    6-bit literals, a match whose length code (symbol 284, 5 extra bits) and distance code (symbols 28 / 29,
    13 extra bits) are 15 bits long, six 6-bit literals.  The literal/length code is Kraft-complete: 56
    6-bit literals, one code each of 4..13 bits (unused), and four 15-bit codes -- a literal, the length
    symbol 284, 285 (unused) and end of block; the distance code has the lengths 1, 2, ..., 14, 15, 15 with
    the two 15-bit codes on the symbols 28 and 29.  -> (payload, deflate body)."""
    rng = np.random.default_rng(seed)
    lits6 = [int(x) for x in rng.permutation(250)[:56]]
    rest = [s for s in range(250) if s not in lits6]
    ll = [0] * 286
    for s in lits6:
        ll[s] = 6
    for k, s in zip(range(4, 14), rest):  # fillers: one code of every length 4..13
        ll[s] = k
    lit15 = 255
    ll[lit15] = ll[284] = ll[285] = ll[256] = 15
    assert abs(D.kraft(ll) - 1.0) < 1e-12
    dl = list(range(1, 15)) + [0] * 14 + [15, 15]  # symbols 0..13: 1..14 bits, 28 / 29: 15 bits
    assert len(dl) == 30 and abs(D.kraft(dl) - 1.0) < 1e-12
    lc, dc = D.canonical_codes(ll), D.canonical_codes(dl)

    w = D.BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(286 - 257, 5)
    w.put(30 - 1, 5)
    w.put(19 - 4, 4)
    cl_len = [4 if s < 16 else 0 for s in range(19)]
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        w.put(cl_len[s], 3)
    clc = D.canonical_codes(cl_len)
    for L in ll + dl:
        w.put(clc[L], 4)

    out = bytearray()

    def lit(b):
        w.put(lc[b], ll[b])
        out.append(b)

    # the window: 16,500 literal bytes, a 15-bit literal now and then
    while len(out) < 16_500:
        lit(lit15 if rng.random() < 0.02 else lits6[int(rng.integers(56))])
    n_match = 0
    while len(out) + 12 + 257 <= size:
        for _ in range(6):
            lit(lits6[int(rng.integers(56))])
        length = int(rng.integers(227, 258))
        dsym = 28 + int(rng.integers(2))
        dist = DIST_BASE[dsym] + int(rng.integers(0, 8192))
        dist = min(dist, len(out))
        if dist < DIST_BASE[dsym]:
            dsym, dist = 28, max(dist, DIST_BASE[28])
        assert DIST_BASE[dsym] <= dist <= len(out)
        w.put(lc[284], 15)
        w.put(length - LEN_BASE[284], 5)
        w.put(dc[dsym], 15)
        w.put(dist - DIST_BASE[dsym], 13)
        for _ in range(length):
            out.append(out[-dist])
        n_match += 1
        for _ in range(6):
            lit(lits6[int(rng.integers(56))])
    assert n_match >= 80
    w.put(lc[256], 15)
    return bytes(out), w.bytes()


_GREEDY = {}


def _greedy():
    if not _GREEDY:
        payload, body = _greedy_block(seed=21)
        _GREEDY["payload"], _GREEDY["member"] = payload, _member(payload, body)
    return _GREEDY["payload"], _GREEDY["member"]


@pytest.mark.parametrize("prep", PREPS)
@pytest.mark.parametrize("copies", [1, 130])
def test_greediest_iterations(ctx, monkeypatch, prep, copies):
    """One block, and the same block 130 times (three waves run it in lockstep: every lane of a wave drains
    its reservoir at the maximum rate in the same iterations)."""
    monkeypatch.setenv("OGE_INFL_PREP", prep)
    payload, member = _greedy()
    assert 38_000 <= len(payload) <= 40_000
    assert ctx.bgzf_inflate(member * copies + EOF_BLOCK) == payload * copies


# ---------------------------------------------------------------------------- leanest iterations
@pytest.mark.parametrize("prep", PREPS)
@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED])
def test_leanest_iterations(ctx, monkeypatch, prep, strategy):
    """200,000 zero bytes: 258-byte matches at 1-2 bits a symbol (dynamic) or the fixed code.  The reservoir is
    almost never consumed and must not overfill."""
    monkeypatch.setenv("OGE_INFL_PREP", prep)
    data = bytes(200_000)
    assert ctx.bgzf_inflate(_bgzf(data, 6, strategy)) == data


# ---------------------------------------------------------------------------- divergent lanes
def _divergent_stream() -> tuple[bytes, bytes, list[int]]:
    from openge_amd import lib as L
    rng = np.random.default_rng(77)
    p = L.synth_params(3_000, preset="mix", seed=9)
    recs, offs, _ = L.synth_host(p)
    bam = recs[: int(offs[-1])].tobytes()
    text = b"the quick brown fox jumps over the lazy dog; " * 200
    rnd = rng.integers(0, 256, 8_000, dtype=np.uint8).tobytes()
    kinds = [bytes(4_000), rnd, text, bam]
    modes = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
             (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)]
    sizes = [1, 4_000] + [int(x) for x in rng.integers(1, 4_001, 238)]
    data, z, starts, at = [], [], [], 0
    for k, n in enumerate(sizes):
        src = kinds[k % 4]
        o = int(rng.integers(0, len(src) - n + 1))
        payload = src[o:o + n]
        level, strategy = modes[(k // 4) % 5]
        m = _member(payload, _deflate(payload, level, strategy))
        starts.append(at)
        at += len(m)
        data.append(payload)
        z.append(m)
    return b"".join(data), b"".join(z) + EOF_BLOCK, starts


@pytest.mark.parametrize("prep", PREPS)
def test_divergent_lanes(ctx, monkeypatch, prep):
    """240 BGZF blocks of 1..4,000 payload bytes -- zeros, random bytes, text and BAM records at levels 0, 1, 6, 9
    and with the fixed code -- so neighbouring lanes reload at different rates; the blocks start at all 16
    residues mod 16."""
    monkeypatch.setenv("OGE_INFL_PREP", prep)
    data, z, starts = _divergent_stream()
    assert len(starts) >= 192
    assert {s % 16 for s in starts} == set(range(16)), "fixture: block starts must cover every residue mod 16"
    assert ctx.bgzf_inflate(z) == data


# ---------------------------------------------------------------------------- end of buffer
def _tail_streams() -> dict[int, tuple[bytes, bytes]]:
    """Streams without the EOF block, one per length residue mod 16: the last block's deflate data ends 9..24
    bytes before the end of the file, i.e. within the last 1..16 bytes of some 16-byte chunk at every offset."""
    text = bytes(np.random.default_rng(5).integers(0, 16, 14_000, dtype=np.uint8) + 65)  # ~4 bits a byte
    head = _bgzf(text[:5_000], 6, eof=False)
    got = {}
    n = 4_000
    while len(got) < 16 and n < 9_000:
        payload = text[1_000:1_000 + n]
        z = head + _member(payload, _deflate(payload, 6))
        got.setdefault(len(z) % 16, (text[:5_000] + payload, z))
        n += 1
    assert sorted(got) == list(range(16)), "fixture: one stream per length residue"
    return got


@pytest.mark.parametrize("prep", PREPS)
def test_end_of_buffer(ctx, monkeypatch, prep):
    from openge_amd import lib as L
    monkeypatch.setenv("OGE_INFL_PREP", prep)
    for res, (data, z) in sorted(_tail_streams().items()):
        assert ctx.bgzf_inflate(z) == data, f"length residue {res}"
        for cut in (1, 8, 17):
            with pytest.raises(L.OgeError):
                ctx.bgzf_inflate(z[:-cut])


# ---------------------------------------------------------------------------- budget guard
def _overrunning_stream() -> bytes:
    """Block A's BSIZE is shortened: its deflate data (a fixed-code literal block, then a final stored block)
    runs on past the end BSIZE claims, through the 8 bytes the index takes for A's CRC and ISIZE and through the
    whole of the next block B, and produces exactly ISIZE bytes -- only the end-of-data test (E_PAST) sees it."""
    lits = bytes(range(97, 123)) * 12
    b_payload = b"next block " * 30
    block_b = _member(b_payload, _deflate(b_payload, 6))
    isize = len(lits) + 8 + len(block_b)
    trailer = struct.pack("<II", 0x12345678, isize)
    stored = trailer + block_b
    w = D.BitWriter()
    w.put(0, 1)
    w.put(1, 2)  # fixed codes, not final
    for b in lits:  # literals 0..143: 8 bits, 0x30 + b, MSB first
        w.put(int(format(0x30 + b, "08b")[::-1], 2), 8)
    w.put(0, 7)  # end of block
    w.put(1, 1)
    w.put(0, 2)  # stored, final
    head = w.bytes()
    body = head + struct.pack("<HH", len(stored), len(stored) ^ 0xFFFF) + stored
    assert zlib.decompressobj(-15).decompress(body) == lits + stored, "fixture: A's deflate data"
    n1 = len(head) + 4  # BSIZE claims the body ends where the stored bytes begin
    z = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + n1 + 8 - 1) + body
    assert z[18 + n1 + 8:] == block_b
    return z + EOF_BLOCK


@pytest.mark.parametrize("prep", PREPS)
def test_budget_guard(ctx, monkeypatch, prep):
    from openge_amd import lib as L
    monkeypatch.setenv("OGE_INFL_PREP", prep)
    with pytest.raises(L.OgeError):
        ctx.bgzf_inflate(_overrunning_stream())
    data = bytes(np.random.default_rng(6).integers(0, 16, 60_001, dtype=np.uint8) + 65)  # ~4 bits a byte
    good = _bgzf(data, 6)
    assert len(good) > 20_000
    bad = bytearray(good)
    for k in range(300, 340):
        bad[k] ^= 0xFF
    with pytest.raises(L.OgeError):
        ctx.bgzf_inflate(bytes(bad))
    assert ctx.bgzf_inflate(good) == data
