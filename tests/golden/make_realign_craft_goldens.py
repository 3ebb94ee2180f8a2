"""Generate the goldens of the crafted local-realignment cases from the REFERENCE itself (build container only).

For each case of tests/realign_cases.py that has a defined reference result, the builder writes ref.fa /
targets.intervals / reads.bam; oracle/_ref/ref_driver (the reference's own LocalRealignment +
ConstrainedMateFixingManager) realigns it three times (its consensus order is random, SURVEY Q19: the three
outputs must agree, else another seed is tried, up to 20); the output record stream is reduced to a SHA-256
and, for cases of at most 1000 output records, one 64-bit digest per record so a mismatch can be located.
The builder's inputs are pinned by their own digests.  Only tests/golden/rl_craft/<case>.json is written.

Usage:  python tests/golden/make_realign_craft_goldens.py [case ...]
"""
from __future__ import annotations

import hashlib
import inspect
import json
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bamutil  # noqa: E402
import oracle  # noqa: E402
import realign_cases as RC  # noqa: E402
import realign_util as R  # noqa: E402

OUT = HERE / "rl_craft"
PER_RECORD_MAX = 1000


def sha(path) -> str:
    return hashlib.sha256(Path(path).read_bytes()).hexdigest()


def input_digests(b: RC.Built) -> dict:
    h, _, recs, offs = bamutil.read_bam(b.bam)
    return {"fasta_sha256": sha(b.fasta), "fai_sha256": sha(b.fasta + ".fai"), "intervals_sha256": sha(b.intervals),
            "header": h, "records_sha256": R.digest(recs, offs)["stream_sha256"], "n": int(len(offs))}


def main(names):
    driver = oracle.build_ref()
    assert driver and driver.exists(), "reference harness could not be built"
    OUT.mkdir(exist_ok=True)
    for name in names or RC.GOLDEN_CASES:
        seed0 = inspect.signature(RC.CASES[name]).parameters["seed"].default
        with tempfile.TemporaryDirectory() as td:
            for bump in range(20):
                seed = seed0 + 1000 * bump
                b = RC.build_case(name, f"{td}/{bump}", seed)
                outs, msg = [], ""
                for rep in range(3):
                    ob = f"{td}/{bump}/out{rep}.bam"
                    r = subprocess.run([str(driver), "realign", "-R", b.fasta, "-L", b.intervals, b.bam, ob],
                                       capture_output=True, timeout=600)
                    if r.returncode:
                        msg = f"reference exit {r.returncode}: {r.stderr.decode(errors='replace')[-300:]}"
                        break
                    outs.append(bamutil.read_bam(ob))
                if not msg:
                    ds = [R.digest(o[2], o[3]) for o in outs]
                    if len({d["stream_sha256"] for d in ds}) == 1:
                        break
                    msg = "a consensus tie (SURVEY Q19)"
                print(f"{name}: seed {seed}: {msg}, trying another")
            else:
                raise SystemExit(f"{name}: no seed with a defined reference result")
            d0 = ds[0]
            meta = {"case": name, "seed": seed, "input": input_digests(b), "output_header": outs[0][0],
                    "n_out": int(len(outs[0][3])), "stream_sha256": d0["stream_sha256"]}
            if meta["n_out"] <= PER_RECORD_MAX:
                meta["per_record"] = [int(x) for x in d0["per_record"]]
            (OUT / f"{name}.json").write_text(json.dumps(meta, indent=1, sort_keys=True) + "\n")
            print(f"{name}: seed={seed} n={meta['n_out']} sha={meta['stream_sha256'][:16]}")


if __name__ == "__main__":
    main(sys.argv[1:])
