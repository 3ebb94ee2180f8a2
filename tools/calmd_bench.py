#!/usr/bin/env python3
"""Stage times of oge_calmd_dev on the realigned C5 set (the Measured table).

The C5 set of tests/test_gpu_large.py (oge_synth_realign at the goldens' spec: 50,000 indel sites, 4,000,000 reads)
is realigned with oge_localrealign, the realigned records go up to HBM once, and oge_calmd_dev runs CALLS times in
one process.  Printed as one JSON object: per stage the HIP-event time of the first call and the median, minimum
and maximum of the others, the host wall time of a call, the counters, the bytes that move at the least and the
time they take at the HBM rate of MI355X_MICROARCH (8 TB/s).

    python tools/calmd_bench.py [--calls 6] [--out FILE]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from openge_amd import lib as L  # noqa: E402

STAGES = ("calmd", "calmd_ref", "calmd_size", "calmd_emit")
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    spec = json.loads((ROOT / "tests" / "golden" / "large.json").read_text())["c5_50k"]["spec"]
    ctx = L.Context(0)
    with tempfile.TemporaryDirectory() as d:
        fa, iv, bam = L.synth_realign(L.realign_synth_params(**spec), d, level=1, threads=16)
        b = L.Bam(bam, threads=16)
        sq = [dict(f.split(":", 1) for f in ln.split("\t")[1:]) for ln in b.header_text.splitlines() if ln.startswith("@SQ")]
        refs = [(f["SN"], int(f["LN"])) for f in sq]
        offs = np.append(b.offs, np.uint64(b.recs.size))
        out, oo, st = ctx.localrealign(b.header_text, b.recs, offs, b.n, fa, iv, L.realign_opts(threads=16))
        n = len(oo) - 1
        base, end = int(oo[0]), int(oo[n])
        d_recs = torch.from_numpy(np.concatenate([out[base:end], np.zeros(16, np.uint8)])).cuda()
        d_offs = torch.from_numpy((oo - np.uint64(base)).view(np.int64).copy()).cuda()
        _, names = L._ref_table(refs)
        o, res, dr, do = ctx._calmd_opts(16), L.CalmdResult(), C.c_void_p(), C.c_void_p()
        times, wall = {s: [] for s in STAGES}, []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            L.check(L.lib().oge_calmd_dev(ctx.h, d_recs.data_ptr(), d_offs.data_ptr(), n, len(refs), names, len(names), fa.encode(),
                                          C.byref(o), C.byref(res), C.byref(dr), C.byref(do)), ctx.h)
            wall.append((time.perf_counter() - t0) * 1e3)
            for s in STAGES:
                times[s].append(ctx.timing(s))
        uploads = ctx.counter("calmd_ref_uploads")
        fasta_bytes = Path(fa).stat().st_size
    counters = {k: getattr(res, k) for k in L.CalmdResult.FIELDS}
    bytes_in = end - base
    # the least that moves: every record read once and written once, its two 8-byte offsets, and of the reference
    # the bases the reads cover (not counted: they are shared between overlapping reads and stay in the caches)
    floor_bytes = bytes_in + counters["bytes_out"] + 16 * n
    rep = {
        "reads": n, "bytes_in": bytes_in, "fasta_bytes": fasta_bytes, "counters": counters, "ref_uploads": uploads,
        "first_call_ms": {s: round(times[s][0], 3) for s in STAGES}, "first_call_wall_ms": round(wall[0], 3),
        "later_calls_ms": {s: {"median": round(statistics.median(times[s][1:]), 3), "min": round(min(times[s][1:]), 3),
                               "max": round(max(times[s][1:]), 3)} for s in STAGES},
        "later_calls_wall_ms": {"median": round(statistics.median(wall[1:]), 3), "min": round(min(wall[1:]), 3), "max": round(max(wall[1:]), 3)},
        "floor_bytes": floor_bytes, "floor_ms": round(floor_bytes / HBM_BYTES_PER_S * 1e3, 4),
    }
    rep["ratio_to_floor"] = round(rep["later_calls_ms"]["calmd"]["median"] / rep["floor_ms"], 2)
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
