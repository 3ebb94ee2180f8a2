"""bench.py as the driver runs it: a plain `--gpus 1 --steps N --warmup W` run does only the headline
steps and prints the result line; --dump-outputs DIR writes what the last timed step returned (the counts
and the output BAM file's bytes, here small enough to be dumped whole); every other leg needs --full."""
import gzip
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bamutil

ROOT = Path(__file__).resolve().parent.parent
PAIRS, STEPS = 5000, 2
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def test_leg_selectors_need_full():
    """--realign-only / --kernel-only pick a leg of --full: without it the arguments are refused (before
    anything touches a GPU)."""
    for sel in ("--realign-only", "--kernel-only"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), sel], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-500:]


@pytest.fixture(scope="module")
def plain_run(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("bench") / "dump"  # not there yet: the benchmark makes it
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--pairs", str(PAIRS), "--seed", "99", "--steps", str(STEPS),
           "--warmup", "1", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), d


@pytest.mark.gpu
def test_plain_run_result_line(plain_run):
    line, _ = plain_run
    assert line["unit"] == "Mreads/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["metric"] and line["n_gpus"] == 1
    assert line["steps"] == STEPS and line["warmup"] == 1 and len(line["warmup_ms"]) == 1
    assert line["ms_per_step"] > 0
    # value = reads per step / time per step; both are rounded to 2 decimals on the line (a step of a few ms
    # and a value of a few Mreads/s: each rounding is below 0.5 %)
    assert line["value"] == pytest.approx(2 * PAIRS / (line["ms_per_step"] / 1e3) / 1e6, rel=1e-2)
    # only the headline steps ran
    assert line["kernel_step"] == {"skipped": True} and line["pcie_inclusive"] is None
    assert "realign" not in line and "cpu_baseline" not in line
    assert line["config"]["deflate"]["zlib6_sample"] is None and line["config"]["deflate"]["level9_same_records"] is None
    assert set(line["stages_ms"]) >= {"bgzf_inflate", "sort_radix", "gather_records", "bgzf_deflate"}


@pytest.mark.gpu
def test_dump_outputs_is_the_last_steps_output_file(plain_run, tmp_path):
    line, d = plain_run
    files = {f.name: np.load(f) for f in d.iterdir()}
    assert set(files) == {"counts.npy", "output_file_sample.npy", "sample_offsets.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 1000 * 1000
    out_bytes, nr, nd = (int(x) for x in files["counts.npy"])
    cfg = line["config"]
    assert (out_bytes, nr, nd) == (cfg["output_file_bytes"], 2 * PAIRS, cfg["duplicates_flagged"])
    rows, offs = files["output_file_sample.npy"], files["sample_offsets.npy"]
    # a file this small is dumped whole: consecutive pieces, the last one zero-padded
    assert rows.ndim == 2 and out_bytes <= rows.size < out_bytes + rows.shape[1]
    assert np.array_equal(offs, np.arange(rows.shape[0]) * rows.shape[1])
    assert np.array_equal(rows, rows.astype(np.uint8))
    flat = rows.astype(np.uint8).ravel()
    assert not flat[out_bytes:].any()
    z = flat[:out_bytes].tobytes()
    assert z[-28:] == EOF_BLOCK
    (tmp_path / "out.bam").write_bytes(z)
    assert gzip.decompress(z)[:4] == b"BAM\1"
    _, _, recs, roffs = bamutil.read_bam(tmp_path / "out.bam")
    assert len(roffs) == nr
    assert int(np.count_nonzero(bamutil.flags_of(recs, roffs) & 0x400)) == nd
    # coordinate order: (refID, pos) never decreases, unmapped (-1) last
    key = [(f["refid"] if f["refid"] >= 0 else 1 << 31, f["pos"])
           for f in (bamutil.fields(bamutil.rec_bytes(recs, o)) for o in roffs)]
    assert key == sorted(key)
