"""Test-side model of the GPU deflate's match search (openge_amd/csrc/bgzf.hip: k_defl_parse for search 0,
k_defl_parse_x for the NEAR / SPAN searches) and an RFC 1951 token walker to compare it with.

`block_tokens(raw)` walks one raw deflate stream and returns, per deflate block, its tokens in stream
order: an int for a literal byte, `(pos, length, distance)` for a match that starts at payload offset pos.

`search_tokens(payload, level, search)` restates the search serially, in plain Python, for one payload of
at most 65,280 bytes and returns the same kind of token list:
  hash      bucket = top 12 bits of (4-byte little-endian word * 2654435761) mod 2^32; levels 1-7 keep a
            15-bit tag (the next 15 bits) in the table entry and accept a bucket entry by tag alone -- a tag
            collision is found where the parse visits the position and costs a literal; levels 8 / 9 verify
            the 4 bytes at the lookup, so every candidate is a same-prefix predecessor.
  rounds    1024 consecutive positions look the table up as the rounds before left it, then enter it (the
            latest position of a bucket wins); candidates reach back 32,768 bytes at most.
  NEAR      bucket' = top 11 bits of the same hash; the earliest position e of the round with p's bucket'
            replaces p's candidate when e < p and their 4-byte words are equal.
  chains    levels 8 / 9 walk candidate-of-candidate up to 8 / 32 deep inside the sub-block of 32,768
            positions and keep the longest match, the nearest of equal lengths.
  lazy      levels 8 / 9: a match of 3..31 bytes gives way to a literal when the next position is a
            candidate with a longer match (SPAN: the next position of the sub-block, else of the segment).
  cut       a match ends at its 64-byte segment's edge, with SPAN at its sub-block's end; without SPAN
            every segment is parsed from its first byte, with SPAN from where the last match ended.
"""
from __future__ import annotations

import numpy as np

import deflate_parse as DP

PAY = 65280
SUB, ROUND, SEG = 32768, 1024, 64
FAST, NEAR, SPAN = 0, 1, 2
SEARCH_NAMES = {0: "fast", 1: "near", 2: "span", 3: "near+span"}


def block_tokens(raw: bytes) -> list[dict]:
    """Deflate blocks of one raw deflate stream: [{type, tokens}] (stored blocks: their bytes as literals)."""
    bits = DP._Bits(raw)
    blocks, pos = [], 0
    while True:
        fin, typ = bits.get(1), bits.get(2)
        toks: list = []
        if typ == 0:
            bits.p = (bits.p + 7) & ~7
            n, nn = bits.get(16), bits.get(16)
            assert n ^ 0xFFFF == nn
            q = bits.p >> 3
            toks = list(bits.b[q:q + n])
            bits.p += 8 * n
            pos += n
        else:
            if typ == 1:
                lit, dist = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                assert typ == 2
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * DP.KCL
                for i in range(hclen):
                    cl[DP.CL_ORDER[i]] = bits.get(3)
                ct = DP._table(cl)
                lens: list[int] = []
                while len(lens) < hlit + hdist:
                    s = DP._dec(bits, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.get(3))
                    else:
                        lens += [0] * (11 + bits.get(7))
                lit, dist = lens[:hlit], lens[hlit:]
            lt, dt = DP._table(lit), DP._table(dist)
            while True:
                s = DP._dec(bits, lt)
                if s < 256:
                    toks.append(s)
                    pos += 1
                elif s == 256:
                    break
                else:
                    c = s - 257
                    ln = DP.LBASE[c] + bits.get(DP.LEXT[c])
                    ds = DP._dec(bits, dt)
                    dd = ds + 1 if ds < 4 else ((2 + (ds & 1)) << ((ds - 2) >> 1)) + 1 + bits.get(DP.DEXT[ds])
                    toks.append((pos, ln, dd))
                    pos += ln
        blocks.append({"type": typ, "tokens": toks})
        if fin:
            break
    return blocks


def replay(tokens: list) -> bytes:
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            pos, ln, dd = t
            assert pos == len(out) and 1 <= dd <= pos
            for _ in range(ln):
                out.append(out[-dd])
        else:
            out.append(t)
    return bytes(out)


def matches(tokens: list) -> list[tuple]:
    return [t for t in tokens if isinstance(t, tuple)]


def crosses_segment(m: tuple) -> bool:
    """The match runs over a 64-byte segment edge (offsets inside the payload's 32,768-byte sub-block)."""
    pos, ln, _ = m
    return pos // SEG != (pos + ln - 1) // SEG


def source_in_own_round(m: tuple) -> bool:
    """The match's source starts in the same round of 1024 positions as the match."""
    pos, _, dd = m
    return (pos - dd) // ROUND == pos // ROUND


def length_symbol(ln: int) -> int:
    return 257 + max(i for i, b in enumerate(DP.LBASE) if b <= ln)


def search_tokens(payload: bytes, level: int, search: int) -> list:
    n = len(payload)
    assert 0 < n <= PAY and 1 <= level <= 9 and 0 <= search <= 3
    near, span = bool(search & NEAR), bool(search & SPAN)
    depth = 32 if level >= 9 else 8 if level == 8 else 1
    chain = lazy = depth > 1
    pad = np.frombuffer(payload + bytes(4), dtype=np.uint8).astype(np.uint32)
    wa = pad[:n] | pad[1:n + 1] << 8 | pad[2:n + 2] << 16 | pad[3:n + 3] << 24
    xa = (wa.astype(np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    w, h, hl, tg = wa.tolist(), (xa >> 20).tolist(), (xa >> 21).tolist(), ((xa >> 5) & 0x7FFF).tolist()
    htab = [0] * 4096
    cand = [0] * n  # candidate position + 1
    tokens: list = []

    def ext(p, j, max_len):
        a, b = payload[p:p + max_len], payload[j:j + max_len]
        if a == b:
            return max_len
        k = 0
        while a[k] == b[k]:
            k += 1
        return k

    for base in range(0, n, SUB):
        end = min(n, base + SUB)
        for r in range(base, end, ROUND):
            rend = min(end, r + ROUND, n - 3)  # positions with four bytes left take part
            first: dict[int, int] = {}
            for p in range(r, rend):
                e = htab[h[p]]
                if chain:
                    j1 = e
                    ok = j1 and p - (j1 - 1) <= 32768 and w[j1 - 1] == w[p]
                else:
                    j1 = e >> 15
                    ok = j1 and p - (j1 - 1) <= 32768 and (e & 0x7FFF) == tg[p]
                c = j1 if ok else 0
                if near:
                    e = first.setdefault(hl[p], p)
                    if e < p and w[e] == w[p]:
                        c = e + 1
                cand[p] = c
            for p in range(r, rend):  # increasing positions: the last one of a bucket stays
                htab[h[p]] = p + 1 if chain else (p + 1) << 15 | tg[p]

        def best(p, s1):
            max_len = min(258, (end if span else s1) - p)
            j = cand[p] - 1
            if not chain and w[p] != w[j]:
                return 0, j
            ln, bj = ext(p, j, max_len), j
            d = 1
            while d < depth and ln < max_len:
                if j < base:
                    break
                nx = cand[j]
                if not nx or p - (nx - 1) > 32768:
                    break
                j = nx - 1
                lj = ext(p, j, max_len)
                if lj > ln:
                    ln, bj = lj, j
                d += 1
            return ln, bj

        p = base
        for s0 in range(base, end, SEG):
            s1 = min(end, s0 + SEG)
            p = max(p, s0) if span else s0
            while p < s1:
                if not cand[p]:
                    tokens.append(payload[p])
                    p += 1
                    continue
                ln, j = best(p, s1)
                if lazy and 3 <= ln < 32 and p + 1 < (end if span else s1) and cand[p + 1] and best(p + 1, s1)[0] > ln:
                    tokens.append(payload[p])
                    p += 1
                    continue
                if ln >= 3:
                    tokens.append((p, ln, p - j))
                    p += ln
                else:
                    tokens.append(payload[p])
                    p += 1
    return tokens


# ------------------------------------------------------------------------------------------- inputs
LADDER_LENGTHS = list(range(3, 11)) + [11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 162, 163,
                                        194, 195, 226, 227, 257, 258]


def ladder(seed: int = 1) -> bytes:
    """For each L of LADDER_LENGTHS a fresh random 258-byte motif that ends at a round boundary, then its
    first L bytes between unique separators (the source lies in the round before, a few hundred positions
    back: its table entries are still there).  A match needs a 4-byte prefix, so length 3 only comes from a
    cut: the rung for L = 3 puts an 8-byte copy 3 bytes before the sub-block's end (offset 32,768).
    A rung only gives its exact length while no later position has taken its prefix's bucket (4096 buckets);
    with the default seed none has, which tests/test_deflate_search_model.py checks on the model."""
    rng = np.random.default_rng(seed)
    out = bytearray()

    def rnd(k):
        return rng.integers(0, 256, k, dtype=np.uint8).tobytes()

    def rung(ln, copy_at=None):
        # motif up to the next round boundary that leaves room, the copy right after it (or at copy_at)
        start = (len(out) + 258 + ROUND - 1) // ROUND * ROUND - 258
        out.extend(rnd(start - len(out)))
        motif = rnd(258)
        out.extend(motif)
        if copy_at is not None:
            out.extend(rnd(copy_at - len(out)))
        out.extend(motif[:ln])
        nxt = motif[ln] if ln < 258 else 0
        out.append((nxt + 1 + int(rng.integers(0, 254))) % 256 if ln < 258 else int(rng.integers(0, 256)))
        assert ln == 258 or out[-1] != nxt
        out.extend(rnd(7))

    cut = False
    for ln in LADDER_LENGTHS[1:]:
        if not cut and len(out) > SUB - 2 * ROUND:  # a rung takes one round: the last but one of the sub-block
            rung(8, copy_at=SUB - 3)
            cut = True
        rung(ln)
    assert cut and len(out) <= PAY
    return bytes(out)


def motifs(k: int, total: int = 40_000, seed: int = 12) -> bytes:
    """A random k-byte motif repeated back to back: in-round sources, matches over several segments."""
    m = np.random.default_rng(seed + k).integers(0, 256, k, dtype=np.uint8).tobytes()
    return (m * (total // k + 1))[:total]


def gapped(seed: int = 13, total: int = 40_000) -> bytes:
    """A 300-byte motif repeated with random gaps of 0..50 random bytes."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    out = bytearray()
    while len(out) < total:
        out += m + rng.integers(0, 256, int(rng.integers(0, 51)), dtype=np.uint8).tobytes()
    return bytes(out[:total])


def tail_copy(seed: int = 14) -> bytes:
    """A 200-byte copy that runs to the payload's last byte."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    return a + a[100:300]


def straddle(seed: int = 15) -> bytes:
    """A 200-byte copy over byte 32,768 (the sub-block edge cuts it)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, SUB - 100, dtype=np.uint8).tobytes()
    return a + a[30000:30200] + rng.integers(0, 256, 500, dtype=np.uint8).tobytes()


def crafted() -> dict[str, bytes]:
    d = {"ladder": ladder(), "gapped": gapped(), "tail_copy": tail_copy(), "straddle": straddle()}
    for k in (65, 257, 700, 1000):
        d[f"motif{k}"] = motifs(k)
    return d


def fixture_payloads(k: int = 2) -> list[bytes]:
    """The first k 65,280-byte payloads of the inflated real-data fixture (tests/golden/inputs/208.yhet.bam)."""
    return [p for p in fixture_stream(k * PAY)]


def fixture_stream(limit: int | None = None):
    import gzip
    from pathlib import Path
    data = gzip.decompress((Path(__file__).parent / "golden" / "inputs" / "208.yhet.bam").read_bytes())
    if limit is not None:
        data = data[:limit]
    return [data[i:i + PAY] for i in range(0, len(data), PAY)]
