"""GPU: the deflate's selectable match searches (oge_ctx_set_deflate_search: NEAR = same-round
candidates, SPAN = matches across 64-byte segment edges).  The default search is untouched (and stays
pinned by test_gpu_bgzf.py::test_deflate_bytes_pinned); the new ones round-trip through host zlib, are
deterministic, produce exactly the token list of the serial model (tests/deflate_search_model.py), reach
the emitter's code paths for lengths above 64, and pay on real reads."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_parse as DP
import deflate_search_model as M
from test_gpu_bgzf import CASES, PAY, _bam_bytes, check_roundtrip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rnd(seed, n, hi=256):
    return np.random.default_rng(seed).integers(0, hi, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def crafted():
    return M.crafted()


@pytest.fixture(scope="module")
def fixture_bytes():
    return b"".join(M.fixture_stream())


@pytest.fixture(scope="module")
def model():
    cache = {}

    def get(name, data, level, search):
        k = (name, level, search)
        if k not in cache:
            cache[k] = M.search_tokens(data, level, search)
        return cache[k]
    return get


# ------------------------------------------------------------------------------------ 1. default untouched
@pytest.mark.parametrize("level", [6, 8, 9])
def test_default_is_fast(ctx, level, crafted):
    assert ctx.deflate_search == 0
    data = _bam_bytes(3_000, seed=9) + crafted["motif257"]
    assert ctx.bgzf_deflate(data, level) == ctx.bgzf_deflate(data, level, search="fast")
    assert ctx.bgzf_deflate(data, level, search=0) == ctx.bgzf_deflate(data, level)
    assert ctx.deflate_search == 0  # the keyword restores the context's setting


def test_bad_search_is_an_error(ctx):
    from openge_amd import lib as L
    for bad in (4, -1, "lazy"):
        with pytest.raises(L.OgeError):
            ctx.set_deflate_search(bad)
    assert ctx.deflate_search == 0
    ctx.set_deflate_search("near+span")
    assert ctx.deflate_search == 3
    ctx.set_deflate_search(0)
    # level 0 ignores the search
    data = _bam_bytes(500)
    assert ctx.bgzf_deflate(data, 0, search=3) == ctx.bgzf_deflate(data, 0)


@pytest.mark.parametrize("word,want", [("near+span", "3"), ("span", "2"), ("fast", "0"), ("best", "error"), ("", "error")])
def test_environment_word(built, word, want):
    """OGE_DEFLATE_SEARCH is read when a context is created; an unknown word fails the creation."""
    code = ("from openge_amd import lib as L\n"
            "try:\n    print(L.Context(0).deflate_search)\n"
            "except L.OgeError as e:\n    assert 'OGE_DEFLATE_SEARCH' in str(e), e\n    print('error')\n")
    env = dict(os.environ, OGE_DEFLATE_SEARCH=word, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [want]


# ------------------------------------------------------------------------- 2. round trip and determinism
LENGTHS = [3, 4, 63, 64, 65, 1023, 1024, 1025, 32767, 32768, 32769, 65279, 65281]


def _roundtrip_inputs(crafted):
    d = dict(CASES)
    for n in LENGTHS:  # compressible (4 letters) and with repeats, so the parse has work at every length
        d[f"len{n}"] = bytes(np.random.default_rng(n).integers(0, 4, n, dtype=np.uint8) + ord("A"))
        d[f"rep{n}"] = (_rnd(n, 97) * (n // 97 + 1))[:n]
    d.update(crafted)
    return d


@pytest.mark.parametrize("level", [6, 8, 9])
@pytest.mark.parametrize("search", [1, 2, 3])
def test_roundtrip_and_determinism(ctx, crafted, search, level):
    for name, data in _roundtrip_inputs(crafted).items():
        z = ctx.bgzf_deflate(data, level, search=search)
        assert z == ctx.bgzf_deflate(data, level, search=search), name
        check_roundtrip(data, z)


@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("search", [1, 2, 3])
def test_unaligned_source(ctx, crafted, search, shift):
    import torch
    from openge_amd import lib as L
    data = crafted["gapped"] + _bam_bytes(3_000, seed=9)[: 2 * PAY + 777]
    dev = torch.device("cuda", 0)
    buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    buf[shift:shift + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    cap = int(L.lib().oge_bgzf_bound(len(data)))
    dst = torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for level in (6, 8):
        got = ctx.bgzf_deflate_dev(buf.data_ptr() + shift, len(data), level, dst.data_ptr(), cap, search=search)
        torch.cuda.synchronize()
        z = dst[:got].cpu().numpy().tobytes()
        check_roundtrip(data, z)
        assert z == ctx.bgzf_deflate(data, level, search=search)  # the same bytes as from an aligned source


# ------------------------------------------------------------------------------------------ 3. exactness
EXACT = ["ladder", "motif65", "motif257", "motif700", "motif1000", "fixture0", "fixture1"]


@pytest.mark.parametrize("level", [6, 8])
@pytest.mark.parametrize("search", [0, 1, 2, 3])
def test_tokens_equal_the_serial_model(ctx, crafted, fixture_bytes, model, search, level):
    """The GPU's blocks decode to exactly the model's token list: the speculative entry iteration gives
    the serial parse, NEAR picks the round's earliest same-prefix position, and the headers are still the
    restated builder's for the decoded counts."""
    inputs = dict(crafted, fixture0=fixture_bytes[:PAY], fixture1=fixture_bytes[PAY:2 * PAY])
    for name in EXACT:
        data = inputs[name]
        assert len(data) <= PAY
        (payload, body), = check_roundtrip(data, ctx.bgzf_deflate(data, level, search=search))
        blocks = M.block_tokens(body)
        assert [b["type"] for b in blocks] == [2], name
        assert blocks[0]["tokens"] == model(name, data, level, search), (name, search, level)
        b, = DP.parse_block(body)
        lit, dist, cl = DP.header_lengths(b["lit_count"], b["dist_count"])
        assert b["lit"] == lit and b["dist"] == dist and b["cl"] == cl


# ----------------------------------------------------------------------------- 4. the new code actually ran
def _gpu_matches(ctx, data, level, search):
    out = []
    for payload, body in check_roundtrip(data, ctx.bgzf_deflate(data, level, search=search)):
        out.append(M.matches([t for b in M.block_tokens(body) for t in b["tokens"]]))
    return out


@pytest.mark.parametrize("search", [2, 3])
def test_ladder_uses_every_length_symbol(ctx, crafted, search):
    (payload, body), = check_roundtrip(crafted["ladder"], ctx.bgzf_deflate(crafted["ladder"], 6, search=search))
    b, = DP.parse_block(body)
    assert b["type"] == 2
    assert all(b["lit_count"][s] > 0 for s in range(257, 286)), [s for s in range(257, 286) if not b["lit_count"][s]]


def test_modes_reach_what_they_name(ctx, crafted):
    data = crafted["gapped"]
    mm = {s: _gpu_matches(ctx, data, 6, s)[0] for s in range(4)}
    assert any(map(M.source_in_own_round, mm[1])) and not any(map(M.crosses_segment, mm[1]))
    assert any(map(M.crosses_segment, mm[2])) and not any(map(M.source_in_own_round, mm[2]))
    assert any(map(M.crosses_segment, mm[3])) and any(map(M.source_in_own_round, mm[3]))
    assert not any(map(M.crosses_segment, mm[0])) and not any(map(M.source_in_own_round, mm[0]))
    assert max(ln for _, ln, _ in mm[0]) <= 64 < max(ln for _, ln, _ in mm[2])


# --------------------------------------------------------------------------------- 5. it pays on real reads
def test_real_reads_get_smaller(ctx, fixture_bytes):
    """The inflated 208.yhet.bam fixture (3.59 MB, 55 payloads).  The bounds are the CPU model's predicted
    ratios (0.897 / 0.863 at level 6, 0.855 at level 8) plus three to four points."""
    data = fixture_bytes
    ref = sum(len(zlib.compress(data[i:i + PAY], 6)) - 6 + 26 for i in range(0, len(data), PAY))
    size = {}
    for level in (6, 8):
        for s in range(4):
            z = ctx.bgzf_deflate(data, level, search=s)
            if s == 3:
                check_roundtrip(data, z)
            size[level, s] = len(z)
            print(f"\nfixture {len(data)} B level {level} search {M.SEARCH_NAMES[s]}: {len(z)} B, ratio {len(z) / len(data):.4f}, "
                  f"vs fast {len(z) / size[level, 0]:.4f}, vs zlib-6 ({ref} B) {len(z) / ref:.4f}", end="")
    assert size[6, 3] < size[6, 1] < size[6, 0]
    assert size[6, 1] <= 0.93 * size[6, 0]
    assert size[6, 3] <= 0.90 * size[6, 0]
    assert size[8, 3] <= 0.90 * size[8, 0]


# ------------------------------------------------------------------------------------- 6. synthetic records
def test_synthetic_records_span_is_no_larger(ctx):
    data = _bam_bytes(40_000, seed=9)
    size = {s: len(ctx.bgzf_deflate(data, 6, search=s)) for s in range(4)}
    print(f"\nsynthetic records {len(data)} B, level 6: " + ", ".join(f"{M.SEARCH_NAMES[s]} {size[s]}" for s in range(4)))
    assert size[2] <= size[0]


# ------------------------------------------------------------------------------------------------- 7. CLI
def test_cli_deflate_search(built, tmp_path, monkeypatch):
    import bamutil
    from goldens import GOLDEN
    from openge_amd import lib as L
    monkeypatch.setenv("OGE_WRITE_DEVICE", "1")
    src = GOLDEN / "inputs" / "208.yhet.bam"
    outs = {}
    for name, extra in (("plain", []), ("both", ["--deflate-search", "near+span"])):
        out = tmp_path / f"{name}.bam"
        r = subprocess.run([str(L.PKG / "openge"), "mergesort", "--nopg", *extra, str(src), "-o", str(out)],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ))
        assert r.returncode == 0, r.stderr
        outs[name] = out
    a, b = bamutil.read_bam(outs["plain"]), bamutil.read_bam(outs["both"])
    assert a[0] == b[0] and bytes(a[2]) == bytes(b[2]) and list(a[3]) == list(b[3])
    assert outs["both"].stat().st_size < outs["plain"].stat().st_size
    r = subprocess.run([str(L.PKG / "openge"), "mergesort", "--deflate-search", "best", str(src), "-o", str(tmp_path / "x.bam")],
                       capture_output=True, text=True, timeout=60, env=dict(os.environ))
    assert r.returncode != 0 and "deflate-search" in r.stderr
