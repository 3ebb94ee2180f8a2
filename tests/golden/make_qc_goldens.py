"""Fixtures for `openge stats` / `count` / `coverage` from the REFERENCE itself (build container only; not called
by build() nor by any test).

Compiles the reference's algorithms/statistics.cpp and algorithms/measure_coverage.cpp in place with the flags
of oracle/Makefile.ref, links them with tests/golden/qc_ref_driver.cpp and the objects under oracle/_ref/obj
into oracle/_ref/qc/ (git-ignored), and runs
  FileReader -> Statistics          with both summaries on                       (stats -I -L)
  FileReader -> MeasureCoverage     at bin sizes 1, 7 and 100, with and without uncovered bins (the table with
                                    every bin only up to 2,000,000 rows, so that a test can write and hash it)
on tests/golden/inputs/simple.bam, 208.yhet.bam and the crafted cases of tests/qc_cases.py.  stdout, stderr and
the TSV go to tests/golden/qc/manifest.json: short texts as they are, long ones as their SHA-256 and length.
Only inputs the reference defines are recorded: n >= 1, no tlen of INT32_MIN, no record beyond the 64 KiB its
reader takes ("Invalid BAM block size"), and every counted position inside its contig's bins; the cases outside that are checked against tests/qc_model.py alone.

Usage:  python tests/golden/make_qc_goldens.py
"""
from __future__ import annotations

import hashlib
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
import qc_cases as K  # noqa: E402
import qc_model as M  # noqa: E402

REF = Path("/root/reference/openge/src")
OUT = ROOT / "oracle" / "_ref" / "qc"
OBJ = ROOT / "oracle" / "_ref" / "obj"
DRIVER = OUT / "qc_ref_driver"
FLAGS = ("-std=gnu++98 -O2 -w -DCOMMANDS_H -include sstream -include fstream -include set -include map -include climits "
         "-include cstdio -include cstring -include cerrno -include algorithm -include sys/time.h -include sys/resource.h").split()
FLAGS += [f"-I{REF}", f"-I{REF}/util"]
BINSIZES = (1, 7, 100)
TEXT_LIMIT = 4096
ZERO_MODE_BINS = 2_000_000  # the table with every bin is recorded up to this many rows: a test has to write and hash it
FILES = {"simple": "simple.bam", "yhet208": "208.yhet.bam"}


def build_driver() -> None:
    oracle.build_ref()
    OUT.mkdir(parents=True, exist_ok=True)
    objs = []
    for src in (REF / "algorithms" / "statistics.cpp", REF / "algorithms" / "measure_coverage.cpp", HERE / "qc_ref_driver.cpp"):
        o = OUT / (src.stem + ".o")
        subprocess.run(["g++", *FLAGS, "-c", str(src), "-o", str(o)], check=True)
        objs.append(str(o))
    rest = [str(p) for p in OBJ.rglob("*.o") if p.name != "ref_driver.o"]
    subprocess.run(["g++", "-o", str(DRIVER), *objs, *rest, "-Wl,--wrap=pthread_cond_wait", "-lz", "-lpthread"], check=True)


def blob(data: bytes) -> dict:
    if len(data) <= TEXT_LIMIT:
        return {"text": data.decode()}
    return {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}


def run(*args) -> tuple[bytes, bytes]:
    r = subprocess.run([str(DRIVER), *map(str, args)], capture_output=True, check=True, timeout=600)
    return r.stdout, r.stderr


def readable(records) -> bool:
    return all(len(r) <= 0xFFFF for r in records)


def record_stats(bam: Path) -> dict:
    out, err = run("stats", bam)
    return {"stdout": blob(out), "stderr": blob(err)}


def record_coverage(bam: Path, tmp: Path, lens) -> dict:
    res = {}
    for bs in BINSIZES:
        for mode in ("zero", "nz"):
            if mode == "zero" and int(M.coverage_layout(lens, bs)[-1]) > ZERO_MODE_BINS:
                continue
            tsv = tmp / "cov.tsv"
            _o, err = run("coverage", bam, tsv, bs, mode)
            res[f"{bs}_{mode}"] = {"tsv": blob(tsv.read_bytes()), "stderr": blob(err)}
    return res


def main() -> None:
    build_driver()
    man = {"stats": {}, "coverage": {}}
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        for name, fn in FILES.items():
            bam = HERE / "inputs" / fn
            _t, refs, recs, offs = bamutil.read_bam(bam)
            c = M.cores(recs, offs)
            assert len(offs) >= 1 and all(M.defined_by_reference(c, [ln for _, ln in refs], bs) for bs in BINSIZES), name
            man["stats"][name] = record_stats(bam)
            man["coverage"][name] = record_coverage(bam, tmp, [ln for _, ln in refs])
        for name, (refs, records) in K.stats_cases().items():
            recs, offs = K.pack(records)
            if not len(offs) or (M.cores(recs, offs)["tlen"] == -(1 << 31)).any() or not readable(records):
                continue
            bam = tmp / "in.bam"
            bamutil.write_bam_py(bam, K.header_text(refs), refs, records)
            man["stats"][name] = record_stats(bam)
        for name, (refs, records, defined) in K.coverage_cases().items():
            recs, offs = K.pack(records)
            ok = readable(records) and all(M.defined_by_reference(M.cores(recs, offs), [ln for _, ln in refs], bs) for bs in BINSIZES)
            assert ok == defined, name
            if not defined:
                continue
            bam = tmp / "in.bam"
            bamutil.write_bam_py(bam, K.header_text(refs), refs, records)
            man["coverage"][name] = record_coverage(bam, tmp, [ln for _, ln in refs])
    (HERE / "qc").mkdir(exist_ok=True)
    (HERE / "qc" / "manifest.json").write_text(json.dumps(man, indent=1, sort_keys=True) + "\n")
    print(f"recorded {len(man['stats'])} stats and {len(man['coverage'])} coverage cases")


if __name__ == "__main__":
    main()
