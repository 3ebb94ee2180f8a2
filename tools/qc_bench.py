#!/usr/bin/env python3
"""Times the stats / coverage reductions (csrc/qc.hip) on the flagship benchmark's records.

Generates bench.py's synthetic set (preset c2, default 150M pairs = 300M reads) straight into HBM with the synth
entry points, then reports, from the library's own stage events (oge_ctx_timing):
  qc_stats      plain, with lengths (-L), with inserts (-I)
  qc_coverage   bin size 100 and 1
  input_pass    the record input pass of oge_sort_markdup_dev on the same records (it reads a superset of the
                core fields plain qc_stats reads), and the ratio qc_stats / input_pass
Every shape is warmed up first; each figure is the median of --steps calls, alternating the measured calls, with
the minimum and maximum beside it.  Prints one JSON line; --out also writes a text table.

    python tools/qc_bench.py [--pairs 150000000] [--steps 7] [--warmup 2] [--out profiles/qc_300m.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=150_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
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
    X, Y, cap = ctx.mergesort_reserve(B)
    ctx.synth_range_dev(p, 0, n, d_offs.data_ptr(), Y)
    ctx.sync()
    buf = C.create_string_buffer(1 << 16)
    L.check(L.lib().oge_synth_header_text(C.byref(p), buf, 1 << 16, None))
    hdr = buf.value.decode()
    lens = [int(f.split(":", 1)[1]) for line in hdr.splitlines() if line.startswith("@SQ") for f in line.split("\t") if f.startswith("LN:")]
    opts, keep = L.markdup_opts_from_header(hdr, p.n_ref)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_perm = torch.empty(n, dtype=torch.int32, device=dev)
    recs, offs = Y, d_offs.data_ptr()

    legs = {
        "qc_stats plain": (lambda: ctx.stats_dev(recs, offs, n), "qc_stats"),
        "qc_stats -L": (lambda: ctx.stats_dev(recs, offs, n, lengths=True), "qc_stats"),
        "qc_stats -I": (lambda: ctx.stats_dev(recs, offs, n, inserts=True), "qc_stats"),
        "qc_coverage b100": (lambda: ctx.coverage_dev(recs, offs, n, lens, 100, fetch=False), "qc_coverage"),
        "qc_coverage b1": (lambda: ctx.coverage_dev(recs, offs, n, lens, 1, fetch=False), "qc_coverage"),
        "input_pass": (lambda: ctx.sort_markdup_dev(recs, offs, n, opts, d_perm.data_ptr(), X, d_out_off.data_ptr()), "input_pass"),
    }
    for _ in range(args.warmup):
        for fn, _stage in legs.values():
            fn()
    ms = {k: [] for k in legs}
    for _ in range(args.steps):  # alternate the legs: drift of the shared host and clocks hits all alike
        for k, (fn, stage) in legs.items():
            fn()
            ms[k].append(ctx.timing(stage))
    st = ctx.stats_dev(recs, offs, n, inserts=True, lengths=True)
    res = {"reads": n, "record_bytes": B, "steps": args.steps, "warmup": args.warmup,
           "ms": {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
           "sorted": st["sorted"], "mapped": st["mapped"], "n_insert": st["n_insert"], "n_lengths": len(st["lengths"][0])}
    ip = res["ms"]["input_pass"]["median"]
    res["plain_over_input_pass"] = round(res["ms"]["qc_stats plain"]["median"] / ip, 3) if ip else None
    res["plain_GBps_of_64B_lines"] = round(n * 64 / res["ms"]["qc_stats plain"]["median"] / 1e6, 1)
    print(json.dumps(res))
    if args.out:
        lines = [f"qc_bench: {n} reads, {B} record bytes, median of {args.steps} alternating calls after {args.warmup} warm-ups (min..max)"]
        lines += [f"  {k:<18} {v['median']:>10.3f} ms  ({v['min']:.3f} .. {v['max']:.3f})" for k, v in res["ms"].items()]
        lines.append(f"  qc_stats plain / input_pass = {res['plain_over_input_pass']}")
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
