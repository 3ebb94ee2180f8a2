"""GPU: phase B of localrealign on the device (realign_prep.hip) on the crafted cases of tests/realign_cases.py
-- trailing / hard / double clips, indels next to a read's end, homopolymer slides to the first base
(cleanUpCigar), windows clamped at a contig's start and end, reads running past the end, irregular inserted
bases, a '*' SEQ, consensuses first kept in the second and third 64-read chunk, a duplicate search past 64
candidates, exactly kCandCap and kCandCap + 1 candidates, reads of 8 and 9 cigar operations, a 5-operation
new cigar, device and host intervals interleaved, more contexts than intervals.

Every case: host-thread phase B and device phase B give the same bytes and counts; both equal the REFERENCE's
output (tests/golden/rl_craft, absent only for eq_x_ops, on which the reference aborts); the device run hands
back to the host exactly the intervals the case declares (realign_cases.Built.work / .host)."""
import pytest

import realign_cases as RC
import realign_util as R

pytestmark = pytest.mark.gpu

HOST_CASES = {"cap_2049": 1, "nine_ops": 1, "five_op_newcigar": 1, "mixed": 2}


@pytest.mark.parametrize("name", list(RC.CASES))
def test_gpu_crafted_case_device_equals_host_and_reference(ctx, tmp_path, monkeypatch, name):
    b, meta, h, recs, offs = RC.load_case(name, tmp_path)
    out, oo, st0, st1 = R.realign_both(ctx, monkeypatch, h, recs, offs, b.fasta, b.intervals)
    print(name, {k: st1[k] for k in ("prep_device_intervals", "prep_host_intervals", "scan_pairs", "scan_ops",
                                     "intervals_cleaned", "reads_realigned")})
    assert (meta is not None) == b.golden
    if meta:
        RC.check_golden(meta, out, oo)  # (the host-phase run gave the same bytes: realign_both)
    assert b.host == HOST_CASES.get(name, 0)
    assert st1["prep_host_intervals"] == b.host
    assert st1["prep_device_intervals"] == b.work - b.host
    assert st0["prep_host_intervals"] == b.work and st0["prep_device_intervals"] == 0
    assert st1["scan_pairs"] > 0 and st1["intervals_cleaned"] > 0


def _multi(ctx, G, h, recs, offs, b):
    from openge_amd import lib as L
    more = [L.Context(0) for _ in range(G - 1)]
    try:
        out, oo, st = ctx.localrealign(h, recs, offs, len(offs) - 1, b.fasta, b.intervals, more=more)
        return bytes(out), list(oo), st
    finally:
        for c in more:
            c.close()


@pytest.mark.parametrize("G", [2, 3, 7])
def test_gpu_crafted_mixed_sharded_over_contexts(ctx, tmp_path, G):
    """Device and host intervals interleaved, over G contexts by interval ranges; with G = 7 there are more
    contexts than work intervals, so at least one rank has none (the empty-batch return of the device prep)."""
    import numpy as np
    b, meta, h, recs, offs = RC.load_case("mixed", tmp_path)
    out, oo, st = _multi(ctx, G, h, recs, offs, b)
    RC.check_golden(meta, np.frombuffer(out, np.uint8), np.array(oo, np.uint64))
    print(G, {k: v for k, v in st.items() if k.startswith("prep_") or k == "scan_pairs"})
    assert st["prep_devices"] == G
    assert st["prep_host_intervals"] == b.host and st["prep_device_intervals"] == b.work - b.host
    assert sum(st[f"prep_rank{g}_intervals"] for g in range(G)) == b.work - b.host
    assert sum(st[f"prep_rank{g}_pairs"] for g in range(G)) + b.host_pairs == st["scan_pairs"]
    assert 0 < b.host_pairs < st["scan_pairs"]  # both halves of the stitched pair table
    if G > b.work:
        assert any(st[f"prep_rank{g}_reads"] == 0 for g in range(G))


@pytest.mark.parametrize("name", ["many_consensuses", "late_kept"])
def test_gpu_crafted_case_over_two_contexts(ctx, tmp_path, name):
    import numpy as np
    b, meta, h, recs, offs = RC.load_case(name, tmp_path)
    out, oo, st = _multi(ctx, 2, h, recs, offs, b)
    RC.check_golden(meta, np.frombuffer(out, np.uint8), np.array(oo, np.uint64))
    assert st["prep_devices"] == 2 and st["prep_host_intervals"] == 0
    assert sum(st[f"prep_rank{g}_intervals"] for g in range(2)) == b.work
    assert sum(st[f"prep_rank{g}_pairs"] for g in range(2)) == st["scan_pairs"] > 0
