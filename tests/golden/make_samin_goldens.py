"""Fixtures for SAM input from the REFERENCE itself (build container only; not called by build() nor by any test).

Builds the reference chain of tests/golden/make_view_goldens.py (view_ref_driver, unchanged) and runs
`view_ref_driver in.sam bam -o out.bam` (FileReader -> Filter -> FileWriter, no @PG line) on every crafted text of
tests/samin_cases.py that the reference defines (samin_cases.reference_subset: no f, B or H tag, no `*` SEQ / QUAL, no
lowercase base, fewer than 100 CIGAR ops, lines well below 10,240 characters, integers inside int32, a newline behind
the last line -- the reference cuts the last character of a last line without one --, no error case) and on
the reference's own test/data/simple.sam, which is also copied to tests/golden/inputs/simple.sam.
Each case runs three times and must give identical output with as many records as lines (the reference's reader can
drop lines); a case that does not is printed and left out, not recorded.
tests/golden/samin/manifest.json: per case the records back to back as hex up to 4096 bytes, SHA-256 and length
beyond, and the record count.

Usage:  python tests/golden/make_samin_goldens.py
"""
from __future__ import annotations

import hashlib
import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(HERE))

import bamutil  # noqa: E402
import make_view_goldens as V  # noqa: E402
import samin_cases as K  # noqa: E402
import samin_model as M  # noqa: E402

SIMPLE = Path("/root/reference/openge/test/data/simple.sam")
HEX_LIMIT = 4096


def blob(data: bytes) -> dict:
    if len(data) <= HEX_LIMIT:
        return {"hex": data.hex()}
    return {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}


def run_once(sam: Path, out: Path) -> tuple[bytes, int] | None:
    out.unlink(missing_ok=True)
    r = subprocess.run([str(V.DRIVER), str(sam), "bam", "-o", str(out)], capture_output=True, timeout=120)
    if r.returncode != 0 or not out.exists():
        return None
    _, _, recs, offs = bamutil.read_bam(out)
    return recs.tobytes(), len(offs)


def main() -> None:
    V.build_driver()
    man, left_out = {}, []
    texts = dict(K.reference_subset())
    texts["simple_sam"] = SIMPLE.read_bytes()
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        for name, text in sorted(texts.items()):
            sam = tmp / "in.sam"
            sam.write_bytes(text)
            lines = len(M.split_text(text)[1])
            runs = [run_once(sam, tmp / "out.bam") for _ in range(3)]
            if any(r is None for r in runs) or len(set(runs)) != 1 or runs[0][1] != lines:
                left_out.append((name, lines, [None if r is None else r[1] for r in runs]))
                continue
            man[name] = {"records": blob(runs[0][0]), "n": lines}
    (HERE / "samin").mkdir(exist_ok=True)
    (HERE / "samin" / "manifest.json").write_text(json.dumps(man, indent=1, sort_keys=True) + "\n")
    shutil.copyfile(SIMPLE, HERE / "inputs" / "simple.sam")
    print(f"recorded {len(man)} cases")
    for name, lines, got in left_out:
        print(f"LEFT OUT {name}: {lines} lines, the three runs gave {got} records")


if __name__ == "__main__":
    main()
