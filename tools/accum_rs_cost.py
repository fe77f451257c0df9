#!/usr/bin/env python3
"""What the accumulating mode of the reduce-scatter half costs: P logical ranks on ONE MI355X, n
gradient elements in one bucket (default 8 ranks x 134 M bf16, the size of profiles/clip_step.md).

Three launch times, alternating in one call:
  plain        reduce_scatter_sq of this tree
  accumulate   reduce_scatter_sq(accumulate=True) of this tree
  parent       reduce_scatter_sq of another checkout (--parent PATH, built there), in child
               processes started between this tree's rounds

Every round times `iters` launches of each variant in turn with device events; the figure of a
variant is the median over rounds of the round's median. Byte model per owned element of a
16-bit gradient: 2 B read per rank's contribution + 4 B written; accumulating reads 4 B more.

    python tools/accum_rs_cost.py --parent ab_old --out profiles/accum_rs.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timed(fn, iters):
    import torch

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def measure(args, variants):
    """Round medians (ms) of the variants, alternating, in this process with the package that is
    first on sys.path."""
    import torch

    from akka_allreduce_1_amd.ops import dtype_code, fill_uniform
    from akka_allreduce_1_amd.parallel import LocalCluster

    dev = torch.device("cuda", 0)
    P, n = args.ranks, args.n
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    es = 2 if dtype == torch.bfloat16 else 4
    per_rank = -(-n * es // P)
    slot = (per_rank + (1 << 20) - 1) // (1 << 20) * (1 << 20)  # one block per slot, whole MiB
    cl = LocalCluster(P, slot_bytes=slot, grid=args.grid, timeout_s=20)
    b = cl.comms[0].block_elems(n, dtype_code(dtype))
    grads = [fill_uniform(torch.empty(n, dtype=dtype, device=dev), seed=10 + k) for k in range(P)]
    gshards = [torch.zeros(b, device=dev) for _ in range(P)]
    fns = {"plain": lambda: cl.reduce_scatter_sq(grads, gshards),
           "accumulate": lambda: cl.reduce_scatter_sq(grads, gshards, accumulate=True)}
    for v in variants:
        for _ in range(args.warmup):
            fns[v]()
    cl.check()
    out = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            if v == "accumulate":  # keep the sums finite whatever the number of launches
                for g in gshards:
                    g.zero_()
            out[v].append(_timed(fns[v], args.iters))
    cl.check()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--n", type=int, default=134_217_728)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="another built checkout whose plain launch is timed too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:  # the plain launch of the checkout on PYTHONPATH, one round set
        print(json.dumps(measure(args, ["plain"])), flush=True)
        return 0
    res = {"plain": [], "accumulate": [], "parent": []}
    for _ in range(3 if args.parent else 1):  # this tree and the parent take turns
        here = measure(args, ["plain", "accumulate"])
        res["plain"] += here["plain"]
        res["accumulate"] += here["accumulate"]
        if args.parent:
            tree = os.path.abspath(args.parent)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--ranks", str(args.ranks), "--n", str(args.n),
                   "--dtype", args.dtype, "--grid", str(args.grid), "--iters", str(args.iters), "--warmup",
                   str(args.warmup), "--rounds", str(args.rounds)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree,
                               env=dict(os.environ, PYTHONPATH=tree, MXAR_ACCUM_COST_TREE=tree))
            if r.returncode != 0:
                print(r.stderr[-2000:], file=sys.stderr)
                return 1
            res["parent"] += json.loads(r.stdout.strip().splitlines()[-1])["plain"]
    med = {k: round(statistics.median(v), 4) for k, v in res.items() if v}
    es = 2 if args.dtype == "bf16" else 4
    summary = {"ranks": args.ranks, "n": args.n, "dtype": args.dtype, "grid": args.grid, "median_ms": med,
               "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items() if v},
               "accumulate_over_plain": round(med["accumulate"] / med["plain"], 4),
               "extra_bytes_read": 4 * args.n, "elem_size": es}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    # a child imports the package of the checkout it was pointed at
    sys.path.insert(0, os.environ.get("MXAR_ACCUM_COST_TREE") or ROOT)
    sys.exit(main())
