"""CPU: the test-side model of the GPU deflate's searches (tests/deflate_search_model.py) is a valid
parse in every mode and level, and its modes differ the way the searches are specified: search 0 never
matches across a 64-byte segment edge nor from a source in the match's own round of 1024 positions,
NEAR does the second, SPAN the first.  tests/test_gpu_deflate_search.py holds the GPU to this model."""
import pytest

import deflate_search_model as M


@pytest.fixture(scope="module")
def inputs():
    d = {k: v[:M.PAY] for k, v in M.crafted().items()}
    for i, p in enumerate(M.fixture_payloads(2)):
        d[f"fixture{i}"] = p
    return d


@pytest.fixture(scope="module")
def parsed(inputs):
    return {(name, level, search): M.search_tokens(data, level, search)
            for name, data in inputs.items() for level in (6, 8, 9) for search in range(4)}


def test_tokens_replay_to_the_input(inputs, parsed):
    for (name, level, search), tokens in parsed.items():
        assert M.replay(tokens) == inputs[name], (name, level, search)
        for pos, ln, dd in M.matches(tokens):
            assert 3 <= ln <= 258 and 1 <= dd <= 32768


def test_fast_stays_inside_segments_and_earlier_rounds(parsed):
    for (name, level, search), tokens in parsed.items():
        mm = M.matches(tokens)
        if not search & M.SPAN:
            assert not any(map(M.crosses_segment, mm)), (name, level, search)
        if not search & M.NEAR:
            assert not any(map(M.source_in_own_round, mm)), (name, level, search)
        assert not any(pos // M.SUB != (pos + ln - 1) // M.SUB for pos, ln, _ in mm)  # every mode: cut at 32,768


def test_near_and_span_both_show_on_the_fixture(parsed):
    for level in (6, 8, 9):
        for name in ("fixture0", "fixture1"):
            mm = M.matches(parsed[name, level, 3])
            assert any(map(M.crosses_segment, mm)) and any(map(M.source_in_own_round, mm))
            # fewer tokens with either mechanism (the estimate the compressed size follows)
            n = [len(parsed[name, level, s]) for s in range(4)]
            assert n[3] < n[1] < n[0] and n[3] < n[2] < n[0]


def test_ladder_rungs_give_every_length_symbol(parsed):
    """The ladder's rungs match at exactly their lengths under SPAN, so every RFC 1951 length symbol
    257..285 is used (257, length 3, by the cut at the sub-block's end)."""
    for level in (6, 8):
        for search in (2, 3):
            mm = M.matches(parsed["ladder", level, search])
            assert {ln for _, ln, dd in mm if dd == 258} >= set(M.LADDER_LENGTHS[1:])
            assert {M.length_symbol(ln) for _, ln, _ in mm} == set(range(257, 286))


def test_walker_reads_zlib_streams(inputs):
    """block_tokens against host zlib: the tokens of zlib's own streams replay to the input."""
    import zlib
    for name in ("fixture0", "ladder", "motif257"):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = c.compress(inputs[name]) + c.flush()
        tokens = [t for b in M.block_tokens(raw) for t in b["tokens"]]
        assert M.replay(tokens) == inputs[name]
