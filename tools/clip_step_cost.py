#!/usr/bin/env python3
"""What gradient clipping costs the fused sharded-DP step: P logical ranks on ONE MI355X, n
parameters in one bucket (default 8 ranks x 134 M bf16, the size of profiles/round4).

Step times, alternating in one call:
  clipped   reduce_scatter_sq + clip_coef + step_adamw_shard of this tree
  fused     step_adamw of this tree
  parent, parent_clipped
            the same two of another checkout (--parent PATH, built there), in child processes
            started between this tree's rounds. The child is THIS file run on that checkout's
            package, so the checkout needs this tree's Python API (reduce_scatter_sq with
            `accumulate`, clip_coef, step_adamw_shard); an older one fails in the child.

--loss-scale adds two variants of this tree to the alternation:
  scaled    the clean loss-scaled + clipped step: reduce_scatter_sq + loss_scale_step (the
            records' all-gather and the one-wave control kernel, csrc/hip/xgmi_scale.hip) +
            step_adamw_record; a static scale of 1024, so nothing drifts over the rounds
  skipped   the same launches with an inf among the sums of squares: the update half walks its
            flag protocol and moves no data
With --parent the summary then also holds `scaled_vs_parent_clipped`: this tree's clean
loss-scaled step over the parent's clipped step, and whether it is inside the parent's margin.

Every round times `iters` steps of each variant in turn with device events; the figure of a
variant is the median over rounds of the round's median. Byte model per owned parameter: fused
14 B read + 14 B written, clipped 8 B more (the fp32 shard written and read once). With
--parent the summary also holds `margin`: the relative spread (max - min over median) of the
parent's own round medians, and `within_margin`: this tree's median <= parent's * (1 + margin).

    python tools/clip_step_cost.py --parent ab_old --out profiles/clip_step.json

--digest (with --parent): no timing. The fused step, the clipped step and the accumulating
clipped step (two micro-batches, then the update) run three chained steps each on small seeded
cases - P in {1, 2, 3, 8}, fp32 / bf16 / fp16, n in {4099, 65 539, 300 003}, 2 MiB slots,
grid 64 - here and in a child on the parent's package; one SHA-256 per case over every rank's
parameters, master, moments, gradient shard and sum of squares. Exit status 1 if a digest
differs from the parent's (2: the child failed).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


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
    params = [fill_uniform(torch.empty(n, dtype=dtype, device=dev), seed=1) for _ in range(P)]
    states = [{k: torch.zeros(b, device=dev) for k in ("master", "exp_avg", "exp_avg_sq")} for _ in range(P)]
    gshards = [torch.zeros(b, device=dev) for _ in range(P)] if set(variants) - {"fused"} else None
    step = [0]

    def fused():
        step[0] += 1
        cl.step_adamw(grads, params, states, step=step[0], **HP)

    def clipped():
        step[0] += 1
        sqs = cl.reduce_scatter_sq(grads, gshards)
        _, coef = cl.clip_coef(sqs, 1.0)
        cl.step_adamw_shard(gshards, params, states, coef=coef, step=step[0], **HP)

    fns = {"fused": fused, "clipped": clipped}
    if "scaled" in variants or "skipped" in variants:
        from akka_allreduce_1_amd.parallel import loss_scale as LS

        cfg = LS.LossScaleConfig(1024.0)
        table = LS.CorrectionTable(dev, HP["betas"])
        ls_states = [LS.new_state(cfg, dev) for _ in range(P)]
        records = [torch.zeros(LS.REC_WORDS, device=dev) for _ in range(P)]
        inf = [torch.full((1,), float("inf"), device=dev) for _ in range(P)]
        bound = [0]

        def scaled(sq_override=None):
            bound[0] += 1
            table.ensure(bound[0])
            sqs = cl.reduce_scatter_sq(grads, gshards)
            cl.loss_scale_step(sq_override or sqs, ls_states, records, [table] * P, cfg, 1.0)
            cl.step_adamw_record(gshards, params, states, records=records, **HP)

        fns["scaled"] = scaled
        fns["skipped"] = lambda: scaled(inf)
    for v in variants:
        for _ in range(args.warmup):
            fns[v]()
    cl.check()
    out = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            out[v].append(_timed(fns[v], args.iters))
    cl.check()
    return out


def digests():
    """{case: SHA-256} of the three step forms with the package that is first on sys.path."""
    import torch

    from akka_allreduce_1_amd.ops import dtype_code, fill_uniform
    from akka_allreduce_1_amd.parallel import LocalCluster

    dev = torch.device("cuda", 0)
    out = {}
    for P in (1, 2, 3, 8):  # 3: the runtime-P loops
        cl = LocalCluster(P, slot_bytes=2 << 20, grid=64, timeout_s=20)
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)):
            for n in (4099, 65_539, 300_003):
                b = cl.comms[0].block_elems(n, dtype_code(dtype))
                full = fill_uniform(torch.empty(n, device=dev), seed=1)
                for form in ("fused", "clipped", "accum"):
                    params = [full.to(dtype, copy=True) for _ in range(P)]
                    states = []
                    for k in range(P):
                        own = full[k * b:(k + 1) * b]
                        st = {key: torch.zeros(b, device=dev) for key in ("master", "exp_avg", "exp_avg_sq")}
                        st["master"][:own.numel()] = own
                        states.append(st)
                    gshards = [torch.zeros(b, device=dev) for _ in range(P)]
                    sha = hashlib.sha256()
                    for step in (1, 2, 3):
                        micro = [[fill_uniform(torch.empty(n, dtype=dtype, device=dev), seed=1000 * step + 100 * m + k)
                                  for k in range(P)] for m in range(2)]
                        sqs = []
                        if form == "fused":
                            cl.step_adamw(micro[0], params, states, step=step, **HP)
                        else:
                            sqs = cl.reduce_scatter_sq(micro[0], gshards)
                            if form == "accum":
                                sqs = cl.reduce_scatter_sq(micro[1], gshards, accumulate=True)
                            _, coef = cl.clip_coef(sqs, 1.0)
                            cl.step_adamw_shard(gshards, params, states, coef=coef, step=step, **HP)
                        cl.check()
                        for k in range(P):
                            for t in [params[k], *states[k].values(), gshards[k], *sqs[k:k + 1]]:
                                sha.update(t.reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
                    out[f"P{P} {name} n{n} {form}"] = sha.hexdigest()
    return out


def _child(tree, extra):
    """This file run on the package of the checkout `tree`; the last line of its output."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + extra, capture_output=True, text=True,
                       timeout=600, cwd=tree, env=dict(os.environ, PYTHONPATH=tree, MXAR_CLIP_COST_TREE=tree))
    if r.returncode != 0:
        print(r.stderr[-2000:], file=sys.stderr)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--n", type=int, default=134_217_728)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="another built checkout (with this tree's Python API) whose steps are timed or digested too")
    ap.add_argument("--digest", action="store_true", help="compare result digests with --parent instead of timing")
    ap.add_argument("--loss-scale", action="store_true", help="time the clean loss-scaled step and a skipped step too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:  # the checkout on PYTHONPATH: its digests, or one round set of its two steps
        print(json.dumps(digests() if args.digest else measure(args, ["clipped", "fused"])), flush=True)
        return 0
    if args.digest:
        if not args.parent:
            ap.error("--digest needs --parent")
        here = digests()
        there = _child(os.path.abspath(args.parent), ["--digest"])
        if there is None:
            return 2
        differ = sorted(c for c in here if here[c] != there.get(c))
        for c in sorted(here):
            print(("DIFFERS " if c in differ else "same    ") + c + " " + here[c], flush=True)
        summary = {"cases": len(here), "differ": differ,
                   "all": hashlib.sha256("".join(here[c] for c in sorted(here)).encode()).hexdigest()}
        print(json.dumps(summary), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(dict(summary, here=here, parent=there), f, indent=1)
        return 1 if differ or len(there) != len(here) else 0
    res = {"clipped": [], "fused": [], "parent": [], "parent_clipped": []}
    mine = ["clipped", "fused"] + (["scaled", "skipped"] if args.loss_scale else [])
    passes = 3 if args.parent else 1
    for _ in range(passes):  # this tree and the parent take turns
        here = measure(args, mine)
        for v in mine:
            res.setdefault(v, []).extend(here[v])
        if args.parent:
            there = _child(os.path.abspath(args.parent),
                           ["--ranks", str(args.ranks), "--n", str(args.n), "--dtype", args.dtype, "--grid",
                            str(args.grid), "--iters", str(args.iters), "--warmup", str(args.warmup), "--rounds",
                            str(args.rounds)])
            if there is None:
                return 2
            res["parent"] += there["fused"]
            res["parent_clipped"] += there["clipped"]
    med = {k: round(statistics.median(v), 4) for k, v in res.items() if v}
    es = 2 if args.dtype == "bf16" else 4
    owned = args.n  # all ranks live on this device: every parameter is owned here once
    summary = {"ranks": args.ranks, "n": args.n, "dtype": args.dtype, "grid": args.grid, "median_ms": med,
               "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items() if v},
               "clipped_over_fused": round(med["clipped"] / med["fused"], 4),
               "byte_model": {"fused_B_per_param": 28, "clipped_B_per_param": 36, "ratio": round(36 / 28, 4),
                              "elem_size": es, "owned_params_on_device": owned}}
    if args.parent:
        pairs = {"fused": "parent", "clipped": "parent_clipped"}
        margin = {v: (max(res[p]) - min(res[p])) / statistics.median(res[p]) for v, p in pairs.items()}
        summary["margin"] = {v: round(m, 4) for v, m in margin.items()}
        summary["within_margin"] = {v: med[v] <= med[p] * (1 + margin[v]) for v, p in pairs.items()}
        if args.loss_scale:
            summary["scaled_vs_parent_clipped"] = {
                "ratio": round(med["scaled"] / med["parent_clipped"], 4),
                "within_margin": med["scaled"] <= med["parent_clipped"] * (1 + margin["clipped"])}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    if os.environ.get("MXAR_CLIP_COST_TREE"):  # a child: import the package of that checkout
        sys.path.insert(0, os.environ["MXAR_CLIP_COST_TREE"])
    else:
        sys.path.insert(0, ROOT)
    sys.exit(main())
