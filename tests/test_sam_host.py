"""CPU: the per-record code the SAM / FASTQ kernels run (openge_amd/csrc/sam_format.h: the size pass and the
emit pass, run lane by lane by tests/native/sam_format_main.cpp) and the host formatter of the fallback lines
(openge_amd/csrc/sam_host.cpp) reproduce tests/sam_model.py byte for byte on every crafted case, in a stand-alone
program built with -fsanitize=address,undefined whose buffers are exactly as large as the size pass says."""
import fcntl
import functools
import os
import struct
import subprocess
from pathlib import Path

import pytest

import sam_cases as K
import sam_model as M

ROOT = Path(__file__).resolve().parent.parent
NATIVE = ROOT / "tests" / "native"
SRCS = [NATIVE / "sam_format_main.cpp", ROOT / "openge_amd/csrc/sam_host.cpp"]
CASES = K.sam_cases()


@functools.lru_cache(maxsize=None)
def program() -> Path:
    out = NATIVE / "_build" / "sam_format_asan"
    out.parent.mkdir(exist_ok=True)
    with open(out.parent / ".sam_format.lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        deps = SRCS + [ROOT / "openge_amd/csrc" / h for h in ("sam_format.h", "sam_host.h", "bam_layout.h")] + [ROOT / "include/openge_hip.h"]
        if not out.exists() or any(d.stat().st_mtime > out.stat().st_mtime for d in deps):
            tmp = out.with_suffix(".tmp")
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", f"-I{ROOT / 'include'}", "-o", str(tmp), *map(str, SRCS)], check=True)
            os.replace(tmp, out)
    return out


def case_file(path: Path, records, mode="sam", trim=(0, 0), expect_bad=-1, names=K.NAMES) -> None:
    blob = "".join(names).encode()
    offs = [0]
    for nm in names:
        offs.append(offs[-1] + len(nm.encode()))
    recs, roff = K.pack(records)
    if expect_bad < 0:
        lines = M.lines(records, names, mode, trim)
        marks = bytes(mode == "sam" and M.needs_host(r) for r in records)
    else:
        lines, marks = [b""] * len(records), bytes(len(records))
    with open(path, "wb") as f:
        f.write(struct.pack("<5I", 0 if mode == "sam" else 1, trim[0], trim[1], len(names), len(blob)))
        f.write(struct.pack(f"<{len(offs)}I", *offs) + blob)
        f.write(struct.pack("<QQ", len(records), len(recs) - 16) + roff.tobytes() + recs[:len(recs) - 16].tobytes())
        f.write(struct.pack("<q", expect_bad) + marks + struct.pack(f"<{len(lines)}Q", *map(len, lines)) + b"".join(lines))


def run(path: Path):
    env = {"PATH": "/usr/bin:/bin", "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    r = subprocess.run([str(program()), str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("name", list(CASES))
def test_sam_kernel_code_and_host_formatter_equal_the_model(name, tmp_path):
    """Record counts around the wave and workgroup sizes, every decimal width, the contig and mate rules, CIGARs up
    to 300 ops, SEQ / QUAL from 0 to 10,000 bases at every output alignment, names of 0 to 254 characters, every
    tag type at its extremes, the NUL that ends a tag list, f and B tags (host lines), and the mix of 3,000."""
    case_file(tmp_path / "c.bin", CASES[name])
    out = run(tmp_path / "c.bin")
    hosts = sum(M.needs_host(r) for r in CASES[name])
    assert out.startswith(f"ok: {len(CASES[name])} records") and out.rstrip().endswith(f"{hosts} host lines"), out


@pytest.mark.parametrize("trim", K.TRIMS)
def test_fastq_kernel_code_equals_the_model(trim, tmp_path):
    """Read lengths on both sides of begin + end + 1."""
    case_file(tmp_path / "c.bin", K.fastq_records(), "fastq", trim)
    run(tmp_path / "c.bin")
    case_file(tmp_path / "d.bin", K.seq_records() + K.name_records(), "fastq", trim)
    run(tmp_path / "d.bin")


def test_no_contigs(tmp_path):
    case_file(tmp_path / "c.bin", K.ref_records() + [K.basic(i) for i in range(5)], names=[])
    run(tmp_path / "c.bin")


@pytest.mark.parametrize("name,bad", [("unknown", 2)] + [(k, len(v) - 1) for k, v in K.malformed_records().items()])
def test_unknown_and_cut_tags_are_refused_by_both(name, bad, tmp_path):
    records = K.unknown_records() if name == "unknown" else K.malformed_records()[name]
    with pytest.raises(M.BadRecord):
        M.sam_line(records[bad], K.NAMES)
    case_file(tmp_path / "c.bin", records, expect_bad=bad)
    assert f"record {bad} refused" in run(tmp_path / "c.bin")
