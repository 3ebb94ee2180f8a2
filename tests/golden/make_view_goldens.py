"""Fixtures for `openge view` / -F sam|fastq from the REFERENCE itself (build container only; not called by
build() nor by any test).

Compiles the reference's algorithms/file_writer.cpp, util/sam_writer.cpp and util/fastq_writer.cpp in place with
the flags of oracle/Makefile.ref, links them with tests/golden/view_ref_driver.cpp and the objects under
oracle/_ref/obj into oracle/_ref/view/ (git-ignored), and runs FileReader -> Filter -> FileWriter with no @PG line
  as SAM     on tests/golden/inputs/simple.bam, 208.yhet.bam and every crafted case of tests/sam_cases.py that the
             reference defines, and on the two files with the filters of FILTERS
  as FASTQ   (single stream: stdout) on the two files and the crafted FASTQ reads at every trim window
stdout goes to tests/golden/view/manifest.json: texts up to 4096 bytes as they are (latin-1: QUAL + 33 passes
127), longer ones as SHA-256 and length; SAM is recorded as its header lines and its body.
FASTQ is recorded without a trim window only.  With -B / -E the reference cuts QUAL twice (Filter::trim,
filter.cpp:188-189): fewer qualities than bases, or bytes from behind them (tags, newlines among them), and an
exception on reads its second cut does not fit; its text there is not a function of the record, so tests pin the
trimmed text by tests/sam_model.py alone.
Only what the reference defines is recorded: no B array and no unknown tag type, no record beyond the block_size of
10,000 its reader takes, pos and mpos below INT32_MAX, CIGAR op codes 0-8 (sam_cases.defined_by_reference).

Usage:  python tests/golden/make_view_goldens.py
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
import sam_cases as K  # noqa: E402
import sam_model as M  # noqa: E402

REF = Path("/root/reference/openge/src")
OUT = ROOT / "oracle" / "_ref" / "view"
OBJ = ROOT / "oracle" / "_ref" / "obj"
DRIVER = OUT / "view_ref_driver"
FLAGS = ("-std=gnu++98 -O2 -w -DCOMMANDS_H -include sstream -include fstream -include set -include map -include climits "
         "-include cstdio -include cstring -include cerrno -include algorithm -include sys/time.h -include sys/resource.h").split()
FLAGS += [f"-I{REF}", f"-I{REF}/util"]
TEXT_LIMIT = 4096
FILES = {"simple": "simple.bam", "yhet208": "208.yhet.bam"}
# name -> the driver's (and the CLI's) filter arguments, per input file
FILTERS = {
    "simple": {"n5": ["-n", "5"], "q30": ["-q", "30"], "l50_100": ["-l", "50-100"], "lplus65": ["-l", "+65"], "lminus64": ["-l", "-64"],
               "l64": ["-l", "64"], "n3_q30": ["-n", "3", "-q", "30"], "r_contig": ["-r", "YHet"], "r_range": ["-r", "YHet:60..100"],
               "r_point_q": ["-r", "YHet:100", "-q", "30"]},
    "yhet208": {"n5": ["-n", "5"], "q30": ["-q", "30"], "l50_100": ["-l", "50-100"], "n100_q30_l": ["-n", "100", "-q", "30", "-l", "+50"],
                "r_contig": ["-r", "YHet"], "r_range": ["-r", "YHet:10000..20000"], "r_range_q": ["-r", "YHet:10000..200000", "-q", "30"]},
}


def build_driver() -> None:
    oracle.build_ref()
    OUT.mkdir(parents=True, exist_ok=True)
    # what the reference's CMake configure step makes of openge_constants.h.in (version 0.3, build type dev:
    # the @PG VN the product writes), into the git-ignored build directory
    template = (REF / "openge_constants.h.in").read_text()
    (OUT / "openge_constants.h").write_text(template.replace("@OPENGE_VERSION@", "0.3").replace("@OPENGE_BUILD_TYPE@", "dev"))
    objs = []
    for src in (REF / "algorithms" / "file_writer.cpp", REF / "util" / "sam_writer.cpp", REF / "util" / "fastq_writer.cpp",
                HERE / "view_ref_driver.cpp"):
        o = OUT / (src.stem + ".o")
        subprocess.run(["g++", *FLAGS, f"-I{OUT}", "-c", str(src), "-o", str(o)], check=True)
        objs.append(str(o))
    rest = [str(p) for p in OBJ.rglob("*.o") if p.name != "ref_driver.o"]
    subprocess.run(["g++", "-o", str(DRIVER), *objs, *rest, "-Wl,--wrap=pthread_cond_wait", "-lz", "-lpthread"], check=True)


def blob(data: bytes) -> dict:
    if len(data) <= TEXT_LIMIT:
        return {"text": data.decode("latin-1")}
    return {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}


def run(bam, fmt: str, *args) -> bytes:
    r = subprocess.run([str(DRIVER), str(bam), fmt, *map(str, args)], capture_output=True, check=True, timeout=60)
    return r.stdout


def sam_entry(bam, *args) -> dict:
    header, body = M.split_header(run(bam, "sam", *args))
    return {"header": blob(header), "body": blob(body)}


def main() -> None:
    build_driver()
    man = {"sam": {}, "filters": {}, "fastq": {}}
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        for name, fn in FILES.items():
            bam = HERE / "inputs" / fn
            man["sam"][name] = sam_entry(bam)
            man["filters"][name] = {}
            for key, args in FILTERS[name].items():
                man["filters"][name][key] = {"args": args, **sam_entry(bam, *args)}
            man["fastq"][name] = blob(run(bam, "fastq"))
        bam = tmp / "in.bam"
        for name, records in K.sam_cases().items():
            if not records or not K.defined_by_reference(records):
                continue
            bamutil.write_bam_py(bam, K.header_text(), K.REFS, records)
            man["sam"][name] = sam_entry(bam)
        bamutil.write_bam_py(bam, K.header_text(), K.REFS, K.fastq_records())
        man["fastq"]["crafted"] = blob(run(bam, "fastq"))
    (HERE / "view").mkdir(exist_ok=True)
    (HERE / "view" / "manifest.json").write_text(json.dumps(man, indent=1, sort_keys=True) + "\n")
    print(f"recorded {len(man['sam'])} SAM cases, {sum(map(len, man['filters'].values()))} filtered runs, "
          f"{len(man['fastq'])} FASTQ runs")


if __name__ == "__main__":
    main()
