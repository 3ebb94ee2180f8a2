"""Fixtures for `openge compare` from the REFERENCE itself (build container only; not called by build() nor by
any test).

The reference's commands/command_compare.cpp lives in its Boost CLI layer, and Boost is not installed.  The file
compiles in place with the flags of oracle/Makefile.ref minus -DCOMMANDS_H (so commands/commands.h is read) plus
`-include iterator`, against the stand-in tests/golden/compare_shim/boost/program_options.hpp (own code: only the
names commands.h and that file use).  It is linked with tests/golden/compare_ref_driver.cpp (own code: fills the
option map from argv, defines the base class's members that live in the uncompiled commands.cpp) and the reference
objects under oracle/_ref/obj into oracle/_ref/compare/ (git-ignored).

Recorded into tests/golden/compare/manifest.json, per run: the directory the command ran in ("inputs" =
tests/golden/inputs, else the crafted case of tests/compare_cases.py whose files are a.bam and b.bam), its
arguments (file names relative to that directory: they appear in stderr), stdout, stderr and the exit status.
Texts up to 4096 bytes are stored as they are, longer ones as SHA-256 and length.

Usage:  python tests/golden/make_compare_goldens.py
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
import compare_cases as K  # noqa: E402
import oracle  # noqa: E402

REF = Path("/root/reference/openge/src")
OUT = ROOT / "oracle" / "_ref" / "compare"
OBJ = ROOT / "oracle" / "_ref" / "obj"
DRIVER = OUT / "compare_ref_driver"
FLAGS = ("-std=gnu++98 -O2 -w -include iterator -include sstream -include fstream -include set -include map -include climits "
         "-include cstdio -include cstring -include cerrno -include algorithm -include sys/time.h -include sys/resource.h").split()
FLAGS += [f"-I{REF}", f"-I{REF}/util", f"-I{HERE / 'compare_shim'}"]
TEXT_LIMIT = 4096
S, Y, T = "simple.bam", "208.yhet.bam", "simple.sam"
# name -> arguments, run in tests/golden/inputs
FILE_RUNS = {f"{a.split('.')[0]}_{a.split('.')[-1]}__{b.split('.')[0]}_{b.split('.')[-1]}": [a, b] for a in (S, Y, T) for b in (S, Y, T)}
FILE_RUNS.update({
    "one_input": [S],
    "three": [S, Y, T],
    "three_other_order": [Y, T, S],
    "three_region": ["-r", "YHet:0..300", S, Y, T],
    "three_regions_print": ["-p", "-r", "YHet:0..120", "-r", "YHet", S, Y, T],
    "print_sam_vs_bam": ["-p", T, S],
    "print_simple_vs_yhet_region": ["-p", "-r", "YHet:0..300", S, Y],
    "print_yhet_vs_simple": ["-p", Y, S],
    "print_all_added": ["-p", S, Y],
    "r_contig": ["-r", "YHet", S, Y],
    "r_range": ["-r", "YHet:0..300", S, Y],
    "r_point": ["-r", "YHet:100", S, Y],
    "r_overlapping": ["-r", "YHet:0..300", "-r", "YHet:200..500", "-r", "YHet:100", Y, S],
    "r_unknown_contig": ["-r", "YHet:5..9", "-r", "chrNope:1..2", S, Y],
    "r_two_colons": ["-r", "YHet:1..2:3", S, Y],
    "r_start_past_end": ["-r", "YHet:999999999", S, Y],
    "r_stop_past_end": ["-r", "YHet:5..999999999", S, Y],
})


def build_driver() -> None:
    oracle.build_ref()
    OUT.mkdir(parents=True, exist_ok=True)
    objs = []
    for src in (REF / "commands" / "command_compare.cpp", HERE / "compare_ref_driver.cpp"):
        o = OUT / (src.stem + ".o")
        subprocess.run(["g++", *FLAGS, "-c", str(src), "-o", str(o)], check=True)
        objs.append(str(o))
    rest = [str(p) for p in OBJ.rglob("*.o") if p.name != "ref_driver.o"]
    subprocess.run(["g++", "-o", str(DRIVER), *objs, *rest, "-Wl,--wrap=pthread_cond_wait", "-lz", "-lpthread"], check=True)


def blob(data: bytes) -> dict:
    if len(data) <= TEXT_LIMIT:
        return {"text": data.decode("latin-1")}
    return {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}


def run(cwd, where: str, args: list[str]) -> dict:
    r = subprocess.run([str(DRIVER), *args], capture_output=True, cwd=cwd, timeout=120)
    return {"dir": where, "args": args, "stdout": blob(r.stdout), "stderr": blob(r.stderr), "status": r.returncode}


def main() -> None:
    build_driver()
    man = {}
    for name, args in FILE_RUNS.items():
        man[name] = run(HERE / "inputs", "inputs", args)
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        for name, (ra, rb, regions) in K.cases().items():
            bamutil.write_bam_py(tmp / "a.bam", K.header_text(), K.REFS, ra)
            bamutil.write_bam_py(tmp / "b.bam", K.header_text(), K.REFS, rb)
            rargs = [x for rs in (regions or []) for x in ("-r", rs)]
            man[f"case_{name}"] = run(tmp, name, [*rargs, "a.bam", "b.bam"])
            man[f"case_{name}_print"] = run(tmp, name, ["-p", *rargs, "a.bam", "b.bam"])
    (HERE / "compare").mkdir(exist_ok=True)
    (HERE / "compare" / "manifest.json").write_text(json.dumps(man, indent=1, sort_keys=True) + "\n")
    bad = [k for k, v in man.items() if v["status"] not in (0, 255)]
    print(f"recorded {len(man)} runs" + (f"; unexpected status in {bad}" if bad else ""))


if __name__ == "__main__":
    main()
