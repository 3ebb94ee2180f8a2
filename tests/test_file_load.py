"""CPU: the module layer's loader (csrc/file_load.cpp: range_to_device, file_to_device, the prefetch; bamio's
pread_all under them) as a stand-alone program over a malloc-backed stand-in for the device (tests/native/
file_load_main.cpp), built with AddressSanitizer and, separately, ThreadSanitizer.  4096-byte chunks read as
1024-byte slices, every boundary length at file offsets 0, 1 and 4097: the bytes arrive, nothing is written
past them, a short file fails, and every allocation or copy that fails fails the call without a leak."""
import fcntl
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NATIVE = ROOT / "tests" / "native"
CSRC = ROOT / "openge_amd" / "csrc"
SRCS = [NATIVE / "file_load_main.cpp", CSRC / "file_load.cpp", CSRC / "bamio.cpp"]
FLAGS = {"asan": ["-fsanitize=address", "-fno-omit-frame-pointer"], "tsan": ["-fsanitize=thread"]}


def _build(kind: str) -> Path:
    out = NATIVE / "_build" / f"file_load_{kind}"
    out.parent.mkdir(exist_ok=True)
    # pytest-xdist workers may ask for the same binary at once: build under a lock, publish atomically
    with open(out.parent / f".file_load_{kind}.lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        deps = SRCS + list(CSRC.glob("*.h")) + [ROOT / "include" / "openge_hip.h"]
        if out.exists() and all(d.stat().st_mtime <= out.stat().st_mtime for d in deps):
            return out
        tmp = out.with_suffix(".tmp")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", *FLAGS[kind], f"-I{ROOT / 'include'}", "-o", str(tmp),
                        *map(str, SRCS), "-lz", "-lpthread", "-ldl"], check=True)
        os.replace(tmp, out)
        return out


@pytest.mark.parametrize("kind", ["asan", "tsan"])
def test_loader_clean_under_sanitizer(kind, tmp_path):
    exe = _build(kind)
    data = tmp_path / "bytes.bin"
    data.write_bytes(np.random.default_rng(20).integers(0, 256, 24 * 1024 + 7, dtype=np.uint8).tobytes())
    env = {"PATH": "/usr/bin:/bin", "ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "TSAN_OPTIONS": "halt_on_error=1"}
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "AddressSanitizer" not in r.stderr and "ThreadSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
    assert r.stdout.startswith("ok ")
