"""CPU: the crafted local-realignment cases (tests/realign_cases.py: clips, early indels, homopolymer slides,
contig edges, irregular insertions, the candidate cap, host hand-back shapes) -- the builder is pinned to the
inputs the goldens were made from, and the product's host phases (with the oracle scan) give the REFERENCE's
own output (tests/golden/rl_craft/*.json, made by make_realign_craft_goldens.py).  The host path is the GPU
tests' second reference (test_gpu_realign_craft.py)."""
from pathlib import Path

import pytest

import realign_cases as RC
import realign_util as R


@pytest.mark.parametrize("name", RC.GOLDEN_CASES)
def test_host_phases_match_reference_on_crafted_case(built, tmp_path, name):
    b, meta, h, recs, offs = RC.load_case(name, tmp_path)  # (asserts the input digests)
    st = {}
    out, oo = R.realign_cpu(h, recs, offs, len(offs) - 1, b.fasta, b.intervals, stats=st)
    RC.check_golden(meta, out, oo)
    assert st["prep_host_intervals"] == b.work  # (no device here: every work interval)


def test_every_shape_but_eq_x_has_a_golden():
    assert RC.NO_GOLDEN == ("eq_x_ops",)
    assert sorted(p.stem for p in RC.GOLDEN_DIR.glob("*.json")) == sorted(RC.GOLDEN_CASES)


def test_mixed_declared_host_pairs(built, tmp_path):
    """The pairs the mixed case declares for its two host intervals are what the host path scans when it is given
    those two intervals alone."""
    b, meta, h, recs, offs = RC.load_case("mixed", tmp_path)
    assert len(b.host_intervals) == b.host == 2
    iv = tmp_path / "host.intervals"
    iv.write_text("".join(b.host_intervals))
    st = {}
    R.realign_cpu(h, recs, offs, len(offs) - 1, b.fasta, str(iv), stats=st)
    assert st["scan_pairs"] == b.host_pairs and st["prep_host_intervals"] == 2
    lines = Path(b.intervals).read_text().splitlines(keepends=True)
    assert len(lines) == 6 and [lines.index(x) for x in b.host_intervals] == [1, 3]
