"""CPU: the per-tile and per-line code the SAM input kernels run (openge_amd/csrc/sam_parse.h: line index, size pass and
emit pass, run lane by lane by tests/native/sam_parse_main.cpp) and the host's record builder
(openge_amd/csrc/sam_host.cpp) reproduce tests/samin_model.py byte for byte on every crafted case and the two real
files, in a stand-alone program built with -fsanitize=address,undefined whose text buffer is exactly the text and
whose record buffer is exactly the computed size plus the arena's 16 bytes of slack."""
import fcntl
import functools
import os
import struct
import subprocess
from pathlib import Path

import pytest

import bamutil
import sam_model
import samin_cases as K
import samin_model as M

ROOT = Path(__file__).resolve().parent.parent
NATIVE = ROOT / "tests" / "native"
GOLDEN = ROOT / "tests" / "golden"
SRCS = [NATIVE / "sam_parse_main.cpp", ROOT / "openge_amd/csrc/sam_host.cpp"]
CASES = K.cases()
ERRORS = K.error_cases()
# the model's field -> the kernel's error code (sam_parse.h)
CODE = {"short": 1, "fields": 2, "QNAME": 3, "FLAG": 4, "RNAME": 5, "POS": 6, "MAPQ": 7, "CIGAR": 8, "CIGAR ops": 9, "PNEXT": 10, "TLEN": 11,
        "QUAL": 12, "tag": 13, "tag type": 14, "tag integer": 15}


@functools.lru_cache(maxsize=None)
def program() -> Path:
    out = NATIVE / "_build" / "sam_parse_asan"
    out.parent.mkdir(exist_ok=True)
    with open(out.parent / ".sam_parse.lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        deps = SRCS + [ROOT / "openge_amd/csrc" / h for h in ("sam_parse.h", "sam_host.h", "bam_layout.h")] + [ROOT / "include/openge_hip.h"]
        if not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps):
            tmp = out.with_suffix(".tmp")
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", str(tmp), *map(str, SRCS)], check=True)
            os.replace(tmp, out)
    return out


def case_file(path: Path, text: bytes, names=None, expect_bad=-1, code=0) -> None:
    header, lines = M.split_text(text)
    if names is None:
        names = M.contigs(header)
    blob = "".join(names).encode()
    offs = [0]
    for nm in names:
        offs.append(offs[-1] + len(nm.encode()))
    loff = M.line_offsets(text)
    if expect_bad < 0:
        recs, warns, hosts = M.parse_text(text, names)
    else:
        recs, warns, hosts = [b""] * len(lines), [0] * len(lines), [0] * len(lines)
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(names), len(blob)) + struct.pack(f"<{len(offs)}I", *offs) + blob)
        f.write(struct.pack("<Q", len(text)) + text + struct.pack("<qI", expect_bad, code))
        f.write(struct.pack("<Q", len(lines)) + struct.pack(f"<{len(loff)}Q", *loff) + bytes(map(int, hosts)) + bytes(map(int, warns)))
        f.write(struct.pack(f"<{len(recs)}Q", *map(len, recs)) + b"".join(recs))


def run(path: Path):
    env = {"PATH": "/usr/bin:/bin", "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([str(program()), str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_code_and_host_builder_equal_the_model(name, tmp_path):
    """Line counts around the wave and workgroup sizes, lines around the 64-character chunks and the 4096-byte tiles, a
    tab at every chunk edge, every decimal width, the contig rules with 1 and 3,000 contigs, CIGARs up to 300 ops,
    SEQ / QUAL from 0 to 501 bases, every integer tag boundary, A / Z / H tags, f and B tags (host lines)."""
    case_file(tmp_path / "c.bin", CASES[name])
    out = run(tmp_path / "c.bin")
    _, _, hosts = M.parse_text(CASES[name])
    assert out.startswith(f"ok: {len(hosts)} lines") and out.rstrip().endswith(f" {sum(hosts)} host lines"), out


@pytest.mark.parametrize("fn", ["simple.bam", "208.yhet.bam"])
def test_the_sam_text_of_the_real_files(fn, tmp_path):
    htext, refs, recs, offs = bamutil.read_bam(GOLDEN / "inputs" / fn)
    names = [n for n, _ in refs]
    records = sam_model.split_records(recs, offs)
    text = htext.encode() + b"".join(sam_model.sam_line(r, names) for r in records)
    assert M.parse_text(text, names)[0] == records
    case_file(tmp_path / "c.bin", text, names)
    assert run(tmp_path / "c.bin").rstrip().endswith(" 0 host lines")


def test_simple_sam(tmp_path):
    case_file(tmp_path / "c.bin", (GOLDEN / "inputs" / "simple.sam").read_bytes())
    run(tmp_path / "c.bin")


@pytest.mark.parametrize("name", list(ERRORS))
def test_bad_lines_are_refused_by_both(name, tmp_path):
    text, line, field = ERRORS[name]
    hl = M.split_text(text)[0].count(b"\n")
    case_file(tmp_path / "c.bin", text, expect_bad=line - 1 - hl, code=CODE[field])
    assert f"line {line - 1 - hl} refused" in run(tmp_path / "c.bin")
