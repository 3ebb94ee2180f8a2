#!/usr/bin/env python3
"""Times the SAM text passes (csrc/sam.hip) and the whole `openge view` command.

Kernels: generates bench.py's kind of synthetic records (preset c2, default 10M pairs = 20M reads) straight into
HBM, then times the size pass (oge_text_size_dev: size kernel + the 64-bit scan) and the emit pass
(oge_text_emit_dev over all records) from the library's own stage events (oge_ctx_timing).  Every shape is warmed
up first; each figure is the median of --steps alternating calls with the minimum and maximum beside it.  Bytes are
counted from the shapes: the size pass reads every record but its SEQ and QUAL bytes plus 8 B of offset and writes
9 B per record; the emit pass reads the records and 24 B of offsets per record and writes the text.  Rates are
(bytes read + bytes written) / time, also as a fraction of the 6.3 TB/s the other rooflines of DESIGN.md use.

Command (--cli-pairs > 0): writes a BAM of that many synthetic pairs, then times `openge view --nopg -o FILE` and,
where oracle/_ref/view/view_ref_driver exists (tests/golden/make_view_goldens.py builds it), the reference's own
FileReader -> Filter -> FileWriter chain on the same file with --threads host threads; both write SAM into --tmp
and the two files must be the same bytes.  Wall times, median of --cli-steps runs after one warm-up each.

    python tools/text_bench.py [--pairs 10000000] [--steps 7] [--warmup 2] [--cli-pairs 1000000] [--out FILE]
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
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


def sha(path) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        while chunk := f.read(1 << 24):
            h.update(chunk)
    return h.hexdigest()


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
    st = ctx.stats_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, lengths=True)
    bases = int((st["lengths"][0].astype("uint64") * st["lengths"][1]).sum())
    seq_qual = bases + (bases + n) // 2  # QUAL + packed SEQ (an odd read's last nibble rounds up)
    d_toff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_mark = torch.empty(n, dtype=torch.uint8, device=dev)
    total, n_host = ctx.text_size_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_toff.data_ptr(), d_mark.data_ptr())
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def size():
        ctx.text_size_dev(d_recs.data_ptr(), d_offs.data_ptr(), n, opts, d_toff.data_ptr(), d_mark.data_ptr())
        return ctx.timing("text_size")

    def emit():
        ctx.text_emit_dev(d_recs.data_ptr(), d_offs.data_ptr(), d_toff.data_ptr(), 0, n, opts, d_out.data_ptr(), total)
        ctx.sync()
        return ctx.timing("text_emit")

    for _ in range(args.warmup):
        size(), emit()
    ms = {"text_size": [], "text_emit": []}
    for _ in range(args.steps):
        ms["text_size"].append(size())
        ms["text_emit"].append(emit())
    traffic = {"text_size": (B - seq_qual + 8 * n) + 9 * n, "text_emit": (B + 24 * n) + total}
    res = {"reads": n, "record_bytes": B, "text_bytes": total, "host_lines": n_host, "text_over_record_bytes": round(total / B, 4),
           "steps": args.steps, "warmup": args.warmup, "ms": {k: spread(v) for k, v in ms.items()}, "traffic_bytes": traffic}
    for k in ms:
        rate = traffic[k] / (statistics.median(ms[k]) * 1e-3)
        res[f"{k}_TBps"] = round(rate / 1e12, 3)
        res[f"{k}_fraction_of_6.3TBps"] = round(rate / HBM_ACHIEVABLE, 3)
    res["emit_written_over_read"] = round(total / (B + 24 * n), 4)
    del d_out, d_recs, d_toff, d_mark
    ctx.close()

    if args.cli_pairs > 0:
        tmp = Path(args.tmp)
        src, ours, theirs = tmp / "text_bench_in.bam", tmp / "text_bench_ours.sam", tmp / "text_bench_ref.sam"
        q = L.synth_params(args.cli_pairs, preset="c2", seed=args.seed)
        recs, offs, hdr = L.synth_host(q)
        L.write_bam(src, hdr, recs, offs, 2 * args.cli_pairs, level=1, threads=args.threads)
        cmds = {"openge_view": [str(L.PKG / "openge"), "view", "--nopg", "-t", str(args.threads), "-o", str(ours), str(src)]}
        ref = ROOT / "oracle" / "_ref" / "view" / "view_ref_driver"
        if ref.exists():
            cmds["reference_chain"] = [str(ref), str(src), "sam", "-o", str(theirs), "-t", str(args.threads)]
        wall = {k: [] for k in cmds}
        for step in range(args.cli_steps + 1):  # the first run of each is the warm-up
            for k, cmd in cmds.items():
                t0 = time.perf_counter()
                subprocess.run(cmd, check=True, capture_output=True, timeout=900)
                if step:
                    wall[k].append(time.perf_counter() - t0)
        res["cli"] = {"reads": 2 * args.cli_pairs, "input_bytes": src.stat().st_size, "sam_bytes": ours.stat().st_size, "host_threads": args.threads,
                      "wall_s": {k: spread(v) for k, v in wall.items()}}
        if ref.exists():
            res["cli"]["same_bytes_as_reference"] = sha(ours) == sha(theirs)
            res["cli"]["reference_over_openge"] = round(statistics.median(wall["reference_chain"]) / statistics.median(wall["openge_view"]), 2)
        for f in (src, ours, theirs):
            f.unlink(missing_ok=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
