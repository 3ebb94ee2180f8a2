#!/usr/bin/env python3
"""Times the SAM input passes (csrc/sam_parse.hip) and a whole command that reads SAM.

Kernels: generates bench.py's kind of synthetic records (preset c2, default 10M pairs = 20M reads) straight into HBM,
formats them to SAM text in HBM (oge_text_size_dev / oge_text_emit_dev), then times the line index
(oge_sam_lines_dev with a table to fill: count kernel, scan, fill kernel), the size pass (oge_sam_size_dev: size
kernel + the 64-bit scan) and the emit pass (oge_sam_emit_dev over all lines) from the library's own stage events
(oge_ctx_timing).  Every shape is warmed up first; each figure is the median of --steps rounds over the three calls with
the minimum and maximum beside it.  Bytes are counted from the shapes: the line index reads the text twice and writes
8 B per line; the size pass reads the text and 16 B of offsets per line and writes 11 B per line; the emit pass reads
the text and 24 B of offsets per line and writes the records.  Rates are (bytes read + bytes written) / time, also as a
fraction of the 6.3 TB/s the other rooflines of DESIGN.md use.  The parsed records are compared with the generated
ones byte for byte.

Command (--cli-pairs > 0): writes a BAM of that many synthetic pairs and its SAM text (`openge view`), then times
`openge view --nopg -F bam -o FILE` on the SAM file and on the BAM file and, where oracle/_ref/view/view_ref_driver
exists (tests/golden/make_view_goldens.py builds it), the reference's own chain on the SAM file with --threads host
threads.  The reference's time counts only if its output holds as many records as the SAM file has lines (its reader
can drop lines); the count is reported either way.  Wall times, median of --cli-steps runs after one warm-up each.

    python tools/samin_bench.py [--pairs 10000000] [--steps 7] [--warmup 2] [--cli-pairs 1000000] [--out FILE]
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HBM_ACHIEVABLE = 6.3e12


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cli-pairs", type=int, default=1_000_000)
    ap.add_argument("--cli-steps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from openge_amd import lib as L

    dev = torch.device("cuda:0")
    ctx = L.Context(0)
    p = L.synth_params(args.pairs, preset="c2", seed=args.seed)
    n = 2 * args.pairs
    d_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ctx.synth_range_dev(p, 0, n, d_offs.data_ptr(), None)
    ctx.sync()
    B = int(d_offs[-1].item())
    d_recs = torch.empty(B + 64, dtype=torch.uint8, device=dev)
    d_recs[B:] = 0  # the arena's slack
    torch.cuda.synchronize()  # torch's stream is not the context's: nothing of torch's may still be writing
    ctx.synth_range_dev(p, 0, n, d_offs.data_ptr(), d_recs.data_ptr())
    ctx.sync()
    buf = C.create_string_buffer(1 << 16)
    L.check(L.lib().oge_synth_header_text(C.byref(p), buf, 1 << 16, None))
    names = [f.split(":", 1)[1] for line in buf.value.decode().splitlines() if line.startswith("@SQ") for f in line.split("\t") if f.startswith("SN:")]
    opts, _keep = L.text_opts(names)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_mark = torch.empty(n, dtype=torch.uint8, device=dev)
    T, host_lines_out = ctx.text_size_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_toff.data_ptr(), d_mark.data_ptr())
    d_text = torch.empty(T + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.text_emit_dev(d_recs.data_ptr(), d_offs.data_ptr(), d_toff.data_ptr(), 0, n, opts, d_text.data_ptr(), T)
    ctx.sync()
    assert host_lines_out == 0

    # the text back into records
    assert ctx.sam_lines_dev(d_text.data_ptr(), T, 0) == n
    d_lo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_ro = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_warn = torch.empty(n, dtype=torch.uint8, device=dev)
    d_back = torch.empty(B + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def lines():
        ctx.sam_lines_dev(d_text.data_ptr(), T, 0, d_lo.data_ptr(), n + 1)
        return ctx.timing("sam_lines")

    def size():
        total, n_host = ctx.sam_size_dev(d_text.data_ptr(), d_lo.data_ptr(), n, opts, d_ro.data_ptr(), d_mark.data_ptr(), d_warn.data_ptr())
        assert (total, n_host) == (B, 0), (total, n_host, B)
        return ctx.timing("sam_size")

    def emit():
        ctx.sam_emit_dev(d_text.data_ptr(), d_lo.data_ptr(), d_ro.data_ptr(), 0, n, opts, d_back.data_ptr(), B)
        ctx.sync()
        return ctx.timing("sam_emit")

    for _ in range(args.warmup):
        lines(), size(), emit()
    ms = {"sam_lines": [], "sam_size": [], "sam_emit": []}
    for _ in range(args.steps):
        ms["sam_lines"].append(lines())
        ms["sam_size"].append(size())
        ms["sam_emit"].append(emit())
    same = bool(torch.equal(d_back[:B], d_recs[:B])) and bool(torch.equal(d_ro, d_offs))
    traffic = {"sam_lines": 2 * T + 8 * n, "sam_size": (T + 16 * n) + 11 * n, "sam_emit": (T + 24 * n) + B}
    res = {"reads": n, "text_bytes": T, "record_bytes": B, "records_equal_the_generated_ones": same, "steps": args.steps, "warmup": args.warmup,
           "wave_lines": ctx.counter("sam_wave_lines"), "ms": {k: spread(v) for k, v in ms.items()}, "traffic_bytes": traffic}
    for k in ms:
        rate = traffic[k] / (statistics.median(ms[k]) * 1e-3)
        res[f"{k}_TBps"] = round(rate / 1e12, 3)
        res[f"{k}_fraction_of_6.3TBps"] = round(rate / HBM_ACHIEVABLE, 3)
    del d_back, d_recs, d_text, d_toff, d_mark, d_lo, d_ro, d_warn
    ctx.close()

    if args.cli_pairs > 0:
        tmp = Path(args.tmp)
        bam, sam, o1, o2, o3 = (tmp / f"samin_bench_{k}" for k in ("in.bam", "in.sam", "from_sam.bam", "from_bam.bam", "ref.bam"))
        q = L.synth_params(args.cli_pairs, preset="c2", seed=args.seed)
        recs, offs, hdr = L.synth_host(q)
        L.write_bam(bam, hdr, recs, offs, 2 * args.cli_pairs, level=1, threads=args.threads)
        openge = str(L.PKG / "openge")
        subprocess.run([openge, "view", "--nopg", "-o", str(sam), str(bam)], check=True, capture_output=True, timeout=900)
        cmds = {"view_bam_from_sam": [openge, "view", "--nopg", "-t", str(args.threads), "-F", "bam", "-o", str(o1), str(sam)],
                "view_bam_from_bam": [openge, "view", "--nopg", "-t", str(args.threads), "-F", "bam", "-o", str(o2), str(bam)]}
        ref = ROOT / "oracle" / "_ref" / "view" / "view_ref_driver"
        if ref.exists():
            cmds["reference_chain_from_sam"] = [str(ref), str(sam), "bam", "-o", str(o3), "-t", str(args.threads)]
        wall = {k: [] for k in cmds}
        ref_failed = 0
        for step in range(args.cli_steps + 1):  # the first run of each is the warm-up
            for k, cmd in cmds.items():
                t0 = time.perf_counter()
                r = subprocess.run(cmd, check=not k.startswith("reference"), capture_output=True, timeout=900)
                if r.returncode != 0:  # the reference's chain may abort on a text this large: said below, not fatal here
                    ref_failed = r.returncode
                if step:
                    wall[k].append(time.perf_counter() - t0)

        def count(path) -> int:
            r = subprocess.run([openge, "count", str(path)], capture_output=True, timeout=900)
            return int(r.stdout) if r.returncode == 0 else -1
        res["cli"] = {"reads": 2 * args.cli_pairs, "bam_bytes": bam.stat().st_size, "sam_bytes": sam.stat().st_size, "host_threads": args.threads,
                      "wall_s": {k: spread(v) for k, v in wall.items()}, "records_from_sam": count(o1), "records_from_bam": count(o2),
                      "same_output_bytes": o1.read_bytes() == o2.read_bytes()}
        if ref.exists():
            got = count(o3)
            res["cli"]["reference_records"] = got
            res["cli"]["reference_exit_status"] = ref_failed
            if got == 2 * args.cli_pairs and not ref_failed:
                res["cli"]["reference_over_openge"] = round(statistics.median(wall["reference_chain_from_sam"]) / statistics.median(wall["view_bam_from_sam"]), 2)
        for f in (bam, sam, o1, o2, o3):
            f.unlink(missing_ok=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
