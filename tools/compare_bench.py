#!/usr/bin/env python3
"""Times `openge compare` (csrc/compare.hip) on the flagship benchmark's records.

GPU leg (default): generates bench.py's synthetic set (preset c2, default 150M pairs = 300M reads) straight into HBM,
and in every round
  sorts it by coordinate with oge_sort_markdup_dev             -> the stage times input_pass, sort_radix, sort_ties
  copies the sorted records, moves --edits reads by one base and changes one CIGAR op length in --edits others
  compares the sorted set with the edited copy (oge_compare_dev) -> the stage time compare
so both legs alternate inside one run.  The first --warmup rounds are dropped; each figure is the median of --steps
rounds with the minimum and maximum beside it, from the library's own stage events (oge_ctx_timing).  The expectation
checked by eye: compare = one key pass per set plus one radix sort of 2n items, of the order of the sort stages;
the nested stages compare_keys, compare_sort and compare_runs give the split.

Reference leg (--reference-pairs N, host only): writes the same kind of pair of files for N pairs with the host
generator and times the reference's own compare command on them (the driver built by
tests/golden/make_compare_goldens.py).

Prints one JSON line; --out also writes a text table.

    python tools/compare_bench.py [--pairs 150000000] [--edits 1000] [--steps 5] [--warmup 1] [--out profiles/compare_300m.txt]
    python tools/compare_bench.py --reference-pairs 4000000
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COMPARE_STAGES = ("compare", "compare_keys", "compare_sort", "compare_runs")
SORT_STAGES = ("input_pass", "sort_radix", "sort_ties", "meta_gather", "gather_records")


def edit_host(recs: np.ndarray, offs: np.ndarray, picks: np.ndarray) -> int:
    """the first half of picks: pos ^= 1; the second half: the first op's length ^= 1 (reads without ops: pos ^= 2)"""
    half = len(picks) // 2
    for k, i in enumerate(picks):
        o = int(offs[i])
        ncig = int(recs[o + 16]) | (int(recs[o + 17]) << 8)
        if k < half or not ncig:
            recs[o + 8] ^= 1 if k < half else 2
        else:
            recs[o + 36 + int(recs[o + 12])] ^= 0x10
    return len(picks)


def reference_leg(pairs: int, edits: int, seed: int) -> dict:
    from openge_amd import lib as L

    driver = ROOT / "oracle" / "_ref" / "compare" / "compare_ref_driver"
    if not driver.exists():
        raise SystemExit(f"{driver} is missing: run tests/golden/make_compare_goldens.py first")
    p = L.synth_params(pairs, preset="c2", seed=seed)
    recs, offs, hdr = L.synth_host(p)
    n = 2 * pairs
    order = np.arange(n, dtype=np.uint32)
    with tempfile.TemporaryDirectory() as d:
        a, b = Path(d) / "a.bam", Path(d) / "b.bam"
        L.write_bam(a, hdr, recs, offs, n, order=order, level=1)
        picks = np.random.default_rng(seed).choice(n, size=2 * edits, replace=False)
        edit_host(recs, offs, picks)
        L.write_bam(b, hdr, recs, offs, n, order=order, level=1)
        t0 = time.perf_counter()
        r = subprocess.run([str(driver), str(a), str(b)], capture_output=True, text=True)
        dt = time.perf_counter() - t0
    return {"reference_reads": n, "reference_seconds": round(dt, 3), "reference_stdout": r.stdout.strip(), "reference_status": r.returncode,
            "edited_reads": 2 * edits}


def gpu_leg(args) -> dict:
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
    X, Y, _cap = ctx.mergesort_reserve(B)
    buf = C.create_string_buffer(1 << 16)
    L.check(L.lib().oge_synth_header_text(C.byref(p), buf, 1 << 16, None))
    opts, _keep = L.markdup_opts_from_header(buf.value.decode(), p.n_ref)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_perm = torch.empty(n, dtype=torch.int32, device=dev)
    picks = np.sort(np.random.default_rng(args.seed).choice(n, size=2 * args.edits, replace=False))
    word = np.zeros(1, np.uint32)

    def poke(addr: int, xor: int) -> None:
        L.check(L.lib().oge_memcpy(ctx.h, word.ctypes.data, addr, 4, 2), ctx.h)
        word[0] ^= xor
        L.check(L.lib().oge_memcpy(ctx.h, addr, word.ctypes.data, 4, 1), ctx.h)

    ms = {k: [] for k in SORT_STAGES + COMPARE_STAGES}
    res = None
    for rnd in range(args.warmup + args.steps):
        ctx.synth_range_dev(p, 0, n, d_offs.data_ptr(), Y)
        ctx.sync()
        ctx.sort_markdup_dev(Y, d_offs.data_ptr(), n, opts, d_perm.data_ptr(), X, d_out_off.data_ptr())
        sort_ms = {k: ctx.timing(k) for k in SORT_STAGES}
        # the edited copy takes the place of the unsorted input
        L.check(L.lib().oge_memcpy(ctx.h, Y, X, B, 3), ctx.h)
        ctx.sync()
        torch.cuda.synchronize()
        offs = d_out_off[torch.from_numpy(picks.astype(np.int64)).to(dev)].cpu().numpy()
        for k, o in enumerate(offs):
            o = int(o)
            if k < args.edits:
                poke(Y + o + 8, 1)  # pos
            else:
                L.check(L.lib().oge_memcpy(ctx.h, word.ctypes.data, Y + o + 12, 4, 2), ctx.h)
                lname = int(word[0]) & 0xFF
                L.check(L.lib().oge_memcpy(ctx.h, word.ctypes.data, Y + o + 16, 4, 2), ctx.h)
                if int(word[0]) & 0xFFFF:
                    poke(Y + o + 36 + lname, 0x10)  # the first op's length
                else:
                    poke(Y + o + 8, 2)
        ctx.sync()
        res = ctx.compare_dev(X, d_out_off.data_ptr(), n, Y, d_out_off.data_ptr(), n, p.n_ref)
        if rnd >= args.warmup:
            for k, v in sort_ms.items():
                ms[k].append(v)
            for k in COMPARE_STAGES:
                ms[k].append(ctx.timing(k))
    out = {"reads": n, "record_bytes": B, "steps": args.steps, "warmup": args.warmup, "edited_reads": 2 * args.edits,
           "result": {k: res[k] for k in ("n_ref", "n_other", "common", "additions", "deletions", "hard_runs")},
           "items": ctx.counter("compare_items"), "runs": ctx.counter("compare_runs"),
           "key_bits": ctx.counter("compare_key_bits"), "hash_bits": ctx.counter("compare_hash_bits"),
           "ms": {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()}}
    sort_total = sum(out["ms"][k]["median"] for k in ("input_pass", "sort_radix", "sort_ties"))
    out["compare_over_input_pass_plus_sort"] = round(out["ms"]["compare"]["median"] / sort_total, 3) if sort_total else None
    ctx.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=150_000_000)
    ap.add_argument("--edits", type=int, default=1000, help="reads moved, and as many reads with a changed CIGAR")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reference-pairs", type=int, default=0, help="time the reference's command on this many pairs instead (host only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = reference_leg(args.reference_pairs, args.edits, args.seed) if args.reference_pairs else gpu_leg(args)
    print(json.dumps(res))
    if args.out:
        if args.reference_pairs:
            lines = [f"compare_bench: the reference's compare on {res['reference_reads']} reads a file ({res['edited_reads']} edited): "
                     f"{res['reference_seconds']} s, printed {res['reference_stdout']!r}"]
        else:
            lines = [f"compare_bench: {res['reads']} reads a set, {res['record_bytes']} record bytes, {res['edited_reads']} edited reads, "
                     f"median of {args.steps} rounds after {args.warmup} warm-up (min..max)"]
            lines += [f"  {k:<16} {v['median']:>10.3f} ms  ({v['min']:.3f} .. {v['max']:.3f})" for k, v in res["ms"].items()]
            lines.append(f"  compare / (input_pass + sort_radix + sort_ties) = {res['compare_over_input_pass_plus_sort']}")
            lines.append(f"  result {res['result']}, {res['items']} items in {res['runs']} runs, sort key {res['key_bits']} bits of which hash {res['hash_bits']}")
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
