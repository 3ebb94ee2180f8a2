"""GPU: the two instances of the deflate block writer (k_defl_emit): blocks of at most oge_defl_emit_cap()
bytes are assembled three workgroups to a CU in a small LDS image, larger ones in the full-size image.

The oracle is zlib (split_blocks / check_roundtrip of test_gpu_bgzf.py): every block inflates to its payload
with the right CRC-32 and ISIZE.  Beyond that the class of a block must not show in the bytes: the stream
with OGE_DEFL_EMIT_CAP=0 (every block through the large instance, the path before the split) equals the
stream with the compiled cap and with a cap moved by the knob, and the counters defl_emit_small /
defl_emit_big say which instance wrote how many blocks."""
import struct

import numpy as np
import pytest

from test_gpu_bgzf import CASES, PAY, check_roundtrip

pytestmark = pytest.mark.gpu

KNOB = "OGE_DEFL_EMIT_CAP"


def emit_cap() -> int:
    from openge_amd import lib as L
    return int(L.lib().oge_defl_emit_cap())


def bsizes(z: bytes) -> list[int]:
    """The blocks' sizes (BSIZE + 1) and, implicitly, their offsets in the stream."""
    out, p = [], 0
    while p < len(z):
        out.append(struct.unpack_from("<H", z, p + 16)[0] + 1)
        p += out[-1]
    assert p == len(z)
    return out


def deflate(ctx, monkeypatch, data: bytes, level: int, cap, search=None):
    """The stream and its (small, big) block counts with the knob at cap (None: unset)."""
    if cap is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(cap))
    z = ctx.bgzf_deflate(data, level, search)
    return z, (ctx.counter("defl_emit_small"), ctx.counter("defl_emit_big"))


def check_counts(z: bytes, counts, cap: int):
    sizes = bsizes(z)
    small = sum(1 for s in sizes if s <= cap)
    assert counts == (small, len(sizes) - small)


def lead_random(r: int, seed: int) -> bytes:
    """One payload: r random bytes, then zeros (its block is about r bytes plus the header)."""
    return np.random.default_rng(seed).integers(0, 256, r, dtype=np.uint8).tobytes() + bytes(PAY - r)


_memo = {}


def sweep_data() -> bytes:
    """128 payloads whose block sizes step by about 32 bytes across the compiled cap: payload i starts with
    the first cap - 2048 + 32 i bytes of one random string (so the sizes rise evenly) and continues with zeros."""
    if "sweep" not in _memo:
        cap = emit_cap()
        rnd = np.random.default_rng(100).integers(0, 256, cap + 2048, dtype=np.uint8).tobytes()
        _memo["sweep"] = b"".join(rnd[:r] + bytes(PAY - r) for r in range(cap - 2048, cap + 2048, 32))
    return _memo["sweep"]


def c2_data() -> bytes:
    if "c2" not in _memo:
        from openge_amd import lib as L
        recs, offs, _ = L.synth_host(L.synth_params(20_000, preset="c2", seed=77))
        _memo["c2"] = recs[: int(offs[-1])].tobytes()
    return _memo["c2"]


def payload_sets() -> dict:
    d = {"sweep": sweep_data(), "c2": c2_data()}
    d.update(CASES)
    return d


def test_boundary_sweep_at_the_compiled_cap(ctx, monkeypatch):
    """The 128 payloads under the default search and under NEAR.  The default's candidate rounds leave the
    zeros of the round in which the random bytes end as literals, so its block sizes rise by about 8 bytes per
    payload and jump by about 400 where the random bytes cross a round of 1024 positions -- a jump that can
    straddle the cap (it does at 47,104: 46,971, then above 47,360).  NEAR matches the zeros of a round among
    themselves: its sizes rise by the 32 random bytes a payload adds, so it puts blocks next to the cap on both
    sides.  Every check holds for both streams; the two blocks next to the cap may come from either."""
    cap = emit_cap()
    assert cap % 1024 == 0 and 8352 <= cap < 65536
    data = sweep_data()
    seen = []
    for search in ("fast", "near"):
        z, counts = deflate(ctx, monkeypatch, data, 6, None, search)
        check_roundtrip(data, z)
        sizes = bsizes(z)
        assert len(sizes) == 128
        print(f"\n{search}: cap {cap}; block sizes {min(sizes)}..{max(sizes)}; around the cap "
              f"{sorted(s for s in sizes if abs(s - cap) <= 256)}; small / big {counts}")
        assert counts[0] + counts[1] == 128 and counts[0] > 0 and counts[1] > 0
        check_counts(z, counts, cap)
        assert z == deflate(ctx, monkeypatch, data, 6, 0, search)[0]
        seen += sizes
    assert any(cap - 128 <= s <= cap for s in seen), "no block within 128 B at or below the cap"
    assert any(cap < s <= cap + 128 for s in seen), "no block within 128 B above the cap"


@pytest.mark.parametrize("level", [6, 9])
def test_same_bytes_as_the_single_instance_path(ctx, monkeypatch, level):
    cap = emit_cap()
    for name, data in payload_sets().items():
        z0, c0 = deflate(ctx, monkeypatch, data, level, 0)
        z1, c1 = deflate(ctx, monkeypatch, data, level, None)
        assert z0 == z1, f"{name}: the stream depends on the block's class"
        assert c0 == (0, (len(data) + PAY - 1) // PAY), name
        check_counts(z1, c1, cap)


@pytest.mark.parametrize("level", [6, 9])
def test_cap_moved_by_the_knob(ctx, monkeypatch, level):
    total = [0, 0]
    for name, data in payload_sets().items():
        z0, _ = deflate(ctx, monkeypatch, data, level, 0)
        z2, c2 = deflate(ctx, monkeypatch, data, level, 20000)
        assert z0 == z2, f"{name}: the stream depends on the cap"
        check_counts(z2, c2, 20000)
        total[0] += c2[0]
        total[1] += c2[1]
    assert total[0] > 0 and total[1] > 0  # the sets hold blocks on both sides of 20,000 bytes


def test_cap_above_the_compiled_one_is_clamped(ctx, monkeypatch):
    data = sweep_data()
    z, counts = deflate(ctx, monkeypatch, data, 6, 1 << 20)
    assert z == deflate(ctx, monkeypatch, data, 6, None)[0]
    check_counts(z, counts, emit_cap())


def test_edge_one_byte(ctx, monkeypatch):
    z, counts = deflate(ctx, monkeypatch, b"A", 6, None)
    check_roundtrip(b"A", z)
    assert counts == (1, 0)


def test_edge_short_random_last_payload_is_stored_small(ctx, monkeypatch):
    data = CASES["exact_block"] + np.random.default_rng(11).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    z, counts = deflate(ctx, monkeypatch, data, 6, None)
    blocks = check_roundtrip(data, z)
    assert blocks[1][1][0] == 1 and len(blocks[1][1]) == 1000 + 5  # a stored block
    assert bsizes(z)[1] == 18 + 5 + 1000 + 8 and counts == (2, 0)


def test_edge_full_random_payload_is_stored_big(ctx, monkeypatch):
    data = np.random.default_rng(12).integers(0, 256, PAY, dtype=np.uint8).tobytes()
    z, counts = deflate(ctx, monkeypatch, data, 6, None)
    blocks = check_roundtrip(data, z)
    assert blocks[0][1][0] == 1 and len(blocks[0][1]) == PAY + 5
    assert bsizes(z) == [18 + 5 + PAY + 8] and counts == (0, 1)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_edge_block_off_dword_alignment(ctx, monkeypatch, off):
    """A block of either class that starts 1, 2 or 3 bytes off a dword: one to three compressible payloads in
    front of it, chosen by their own block sizes so that they end at that offset."""
    cap = emit_cap()
    fillers = [lead_random(j, 200 + j) for j in range(1, 13)]
    fsz = bsizes(deflate(ctx, monkeypatch, b"".join(fillers), 6, None)[0])
    front = None
    for k in (1, 2, 3):  # k fillers whose sizes add up to off modulo 4
        for i in range(len(fillers) - k + 1):
            if sum(fsz[i:i + k]) % 4 == off:
                front = b"".join(fillers[i:i + k])
                break
        if front:
            break
    assert front, f"no filler blocks end {off} bytes off a dword (sizes {fsz})"
    nf = len(front) // PAY
    tail = {"small": lead_random(3000, 31), "big": lead_random(cap + 1000, 32),
            "stored_small": np.random.default_rng(33).integers(0, 256, 999, dtype=np.uint8).tobytes()}
    for name, last in tail.items():
        data = front + last
        z, counts = deflate(ctx, monkeypatch, data, 6, None)
        check_roundtrip(data, z)
        sizes = bsizes(z)
        assert sum(sizes[:nf]) % 4 == off, name
        assert (sizes[nf] <= cap) == (name != "big"), name
        check_counts(z, counts, cap)
        assert z == deflate(ctx, monkeypatch, data, 6, 0)[0], name
