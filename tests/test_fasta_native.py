"""CPU: the FASTA loader lifted out of the realigner and the reference table `openge calmd` uploads
(openge_amd/csrc/fasta.h, host_pool.h), exercised by a stand-alone program (tests/native/fasta_selftest.cpp) built
with AddressSanitizer and UndefinedBehaviorSanitizer: line geometry, CRLF, a last line without a newline, an empty
contig, names with descriptions, contigs the FASTA lacks.  Nothing sanitized is loaded into Python."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "fasta_selftest.cpp"
CSRC = ROOT / "openge_amd" / "csrc"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("fasta_native") / "fasta_selftest"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("threads", [1, 4])
def test_loader_and_reference_table_under_asan_and_ubsan(exe, tmp_path, threads):
    r = subprocess.run([str(exe), str(tmp_path), str(threads)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "fasta_selftest ok" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
