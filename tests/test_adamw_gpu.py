"""Fused sharded-DP step (csrc/hip/xgmi_adam.hip): reduce-scatter of the gradients + AdamW on
the owned shard + all-gather of the parameters in one launch.

What is pinned, all in one process on one GPU through LocalCluster (one cached cluster per
rank count, 2 MiB slots, grid 64):

  1. the gradient reduce is exact: on inputs whose sum is exact in fp32 in every order
     (akka_allreduce_1_amd/utils/exact_data.py) and with lr = wd = beta1 = beta2 = 0 the step
     must leave exp_avg = g, exp_avg_sq = fl32(g * g) and master untouched, bit for bit;
  2. the parameters every rank ends with are the owner's fp32 master rounded ONCE to the
     parameter dtype (`params == master.to(dtype)`, torch.equal), and nothing else is written:
     not past n, not the padding of the shard states, not the gradients (the fp16 scalar tail
     once missed this at ties of the fp32 value: its conversion was fused with the last
     multiply-subtract into one mixed-precision FMA, see `adamw()`);
  3. one step from states the test sets against the same formula in float64, inside error
     bounds derived from the operation count of `adamw()` (see `_reference`);
  4. all of it over P = 1, 2, 3, 4, 5, 8 (3 and 5 take the runtime-P loop), three dtypes and
     sizes the launch planner is asked to confirm reach every body of the kernel, plus the flat
     geometry of blocks >= 2 MiB;
  5. an inf / NaN in one rank's gradient reaches every rank at that element and no other;
  6. the state-access modes of MXAR_ADAM_STREAM (fresh child processes: the knob is read once);
  7. `XgmiCommunicator.step_adamw` with its `grid=` override and `op="sum"`;
  8. three chained steps against a PyTorch fp32 evaluation on the full vector (the first test
     this file had).

Items 1, 2 and 5 hold no tolerance at all.
"""
import inspect
import os
import subprocess
import sys

import pytest
import torch

from akka_allreduce_1_amd._native import C
from akka_allreduce_1_amd.ops import dtype_code, fill_uniform
from akka_allreduce_1_amd.parallel import LocalCluster
from akka_allreduce_1_amd.utils.exact_data import exact_inputs, exact_sum

gpu = pytest.mark.gpu
H = C.hip
DEV = torch.device("cuda", 0)
SLOT = 2 << 20
GRID = 64
NMAX = 300_003
GUARD = 64       # sentinel elements behind every parameter tensor
SENTINEL = -7.0  # finite: a stray read is harmless, a stray write visible
UNSET = 3.0      # what the parameters hold before a step: neither the sentinel nor a result
WORLDS = [1, 2, 3, 4, 5, 8]  # 3 and 5: the runtime-P instantiation (PT = 0)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HP = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
U = 2.0 ** -24   # unit roundoff of fp32

_CLUSTERS: dict = {}
_DATA: dict = {}


def _cluster(P, slot=SLOT):
    if (P, slot) not in _CLUSTERS:
        _CLUSTERS[P, slot] = LocalCluster(P, slot_bytes=slot, grid=GRID, timeout_s=10)
    return _CLUSTERS[P, slot]


def _data(P, dtype, n=NMAX, mode="wide"):
    """Rank gradients whose sum is exact in fp32 in every order: made once on the CPU, copied to
    the GPU, never written. Returns (cpu tensors, gpu tensors)."""
    key = (P, dtype, n, mode)
    if key not in _DATA:
        cpu = exact_inputs(P, n, dtype, mode, seed=7000 + 100 * P + _es(dtype))
        _DATA[key] = (cpu, [x.to(DEV) for x in cpu])
    return _DATA[key]


def _sizes(P, dtype, slot=SLOT):
    """Less than one pack (every block but rank 0's empty); one pack +- 1; a ragged tail and a
    short last block; more than one chunk; several runs of 256 packs per reduce unit."""
    es = _es(dtype)
    pack = 16 // es
    return sorted({n for n in (1, 7, pack - 1, pack, pack + 1, 4099, 65_539, NMAX) if n * es <= P * slot})


# ------------------------------------------------------------------------------------------
# The checks of items 1 and 2. Plain functions of torch and the package only: the child
# processes of the state-access-mode test run their source as it stands here.
# ------------------------------------------------------------------------------------------
def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _same(got, want):
    """Bit-equal, NaN where and only where the expectation is NaN."""
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(got[~nan], want[~nan])


def _first_diff(got, want):
    bad = ((got != want) & ~(got.isnan() & want.isnan())).nonzero().flatten()
    if bad.numel() == 0:
        return "no differing element"
    i = int(bad[0])
    return (f"{bad.numel()} of {got.numel()} elements differ, first {i} last {int(bad[-1])}: "
            f"got {float(got[i])!r} want {float(want[i])!r}")


def _make_case(cl, n, dtype, master, exp_avg, exp_avg_sq):
    """Parameters (UNSET, GUARD sentinel elements behind them) and shard states of every rank:
    block r of the three full fp32 vectors, the rest of each shard tensor a sentinel."""
    P = cl.world
    b = cl.comms[0].block_elems(n, dtype_code(dtype))
    bufs = []
    for _ in range(P):
        buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        buf[:n] = UNSET
        bufs.append(buf)
    states = []
    for r in range(P):
        lo, hi = r * b, min(n, (r + 1) * b)
        st = {}
        for key, full in (("master", master), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            st[key] = torch.full((b,), SENTINEL, dtype=torch.float32, device=DEV)
            if hi > lo:
                st[key][:hi - lo] = full[lo:hi]
        states.append(st)
    return {"n": n, "b": b, "P": P, "dtype": dtype, "bufs": bufs, "params": [x[:n] for x in bufs], "states": states}


def _gather(case, key):
    """The full n-element vector of a state, from the ranks' shards."""
    n, b = case["n"], case["b"]
    parts = [st[key][:min(n, (r + 1) * b) - r * b] for r, st in enumerate(case["states"]) if min(n, (r + 1) * b) > r * b]
    return torch.cat(parts)


def _bits(x):
    return x.view(torch.int32 if x.element_size() == 4 else torch.int16)


def _check_written(case, grads, grads_before, what):
    """Item 2: every rank's parameters are the master rounded once; nothing else was written."""
    n, b, dtype = case["n"], case["b"], case["dtype"]
    want = _gather(case, "master").to(dtype)
    assert want.numel() == n
    for r in range(case["P"]):
        assert _same(case["params"][r], want), \
            f"{what} rank {r}: params != master.to(dtype): {_first_diff(case['params'][r], want)}"
        assert bool((case["bufs"][r][n:] == SENTINEL).all()), f"{what} rank {r}: wrote past the end of params"
        valid = max(0, min(n, (r + 1) * b) - r * b)
        for key, t in case["states"][r].items():
            assert bool((t[valid:] == SENTINEL).all()), f"{what} rank {r}: wrote {key} past its {valid} valid elements"
        assert torch.equal(_bits(grads[r]), _bits(grads_before[r])), f"{what} rank {r}: the gradient was written"


def _exact_case(cl, xs, g, n, op, step, seed, what):
    """Item 1. xs: rank gradients whose sum is exact in fp32; g: fp32, their sum times the fp32
    scale of `op`. With lr = wd = beta1 = beta2 = 0 (so c1 = c2_sqrt = 1) the kernel computes, in
    fp32 with or without FMA contraction, m' = 0 * m + 1 * g = g, v' = 0 * v + (1 * g) * g =
    fl(g * g) and p' = p * 1 - (0 / 1) * m' / (sqrt(v') + eps) = p: bit for bit, from non-zero
    states so that a body that skips a load is seen."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p0 = torch.randn(n, device=DEV, generator=gen)
    m0 = torch.randn(n, device=DEV, generator=gen)
    v0 = torch.rand(n, device=DEV, generator=gen) + 0.01
    case = _make_case(cl, n, xs[0].dtype, p0, m0, v0)
    grads = [x[:n].clone() for x in xs]
    cl.step_adamw(grads, case["params"], case["states"], lr=0.0, betas=(0.0, 0.0), eps=1e-8, weight_decay=0.0,
                  step=step, op=op)
    cl.check()
    g = g[:n]
    m1, v1, p1 = _gather(case, "exp_avg"), _gather(case, "exp_avg_sq"), _gather(case, "master")
    assert torch.equal(m1, g), f"{what}: exp_avg is not the exact gradient sum: {_first_diff(m1, g)}"
    assert torch.equal(v1, g * g), f"{what}: exp_avg_sq is not fl(g * g): {_first_diff(v1, g * g)}"
    assert torch.equal(p1, p0), f"{what}: master changed at lr = 0: {_first_diff(p1, p0)}"
    _check_written(case, grads, [x[:n] for x in xs], what)


def _chain_case(cl, n, dtype, op, seed, what, steps=3):
    """Item 2 after each of `steps` chained steps with ordinary hyper-parameters on random data."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p0 = torch.randn(n, device=DEV, generator=gen).to(dtype).float()
    m0 = 0.1 * torch.randn(n, device=DEV, generator=gen)
    v0 = 0.01 * torch.rand(n, device=DEV, generator=gen)
    case = _make_case(cl, n, dtype, p0, m0, v0)
    last = p0
    for t in range(1, steps + 1):
        grads = [torch.randn(n, device=DEV, generator=gen).to(dtype) for _ in range(case["P"])]
        before = [x.clone() for x in grads]
        cl.step_adamw(grads, case["params"], case["states"], step=t, op=op, **HP)
        cl.check()
        _check_written(case, grads, before, f"{what} step {t}")
        now = _gather(case, "master")
        assert bool(now.isfinite().all()) and not torch.equal(now, last), f"{what} step {t}: the master did not move"
        last = now


def _exact_gradient(cpu_xs, scale):
    """fp32: the exact sum times the fp32 scale, as the kernel forms it (exact_sum checks that
    the sum is exact and multiplies the fp32 sum by float32(scale))."""
    return exact_sum(cpu_xs, torch.float32, scale).to(DEV)


def _mode_child(mode):
    """One child process of the state-access-mode test: items 1 and 2 at P = 2 and 3 (the
    templated and the runtime rank count), bf16 and fp32, one size with a single short run and a
    scalar tail and one with several chunks and sub-units."""
    for P in (2, 3):
        cl = LocalCluster(P, slot_bytes=2 << 20, grid=64, timeout_s=10)
        for dtype in (torch.bfloat16, torch.float32):
            cpu = exact_inputs(P, 65_539, dtype, "wide", seed=31 * P + mode)
            xs = [x.to(DEV) for x in cpu]
            for op in ("sum", "avg"):
                g = _exact_gradient(cpu, 1.0 / P if op == "avg" else 1.0)
                for n in (4099, 65_539):
                    what = f"mode {mode} P={P} {dtype} n={n} {op}"
                    _exact_case(cl, xs, g, n, op, 1, n + P, what)
                    _chain_case(cl, n, dtype, op, n + P + 1, what)
        assert cl.comms[0].stats.adamw == 2 * 2 * 2 * 4
    print("mode-ok", mode)


_CHILD_FUNCS = (_es, _same, _first_diff, _make_case, _gather, _bits, _check_written, _exact_case, _chain_case,
                _exact_gradient, _mode_child)
_CHILD_HEAD = f"""import torch
from akka_allreduce_1_amd.ops import dtype_code
from akka_allreduce_1_amd.parallel import LocalCluster
from akka_allreduce_1_amd.utils.exact_data import exact_inputs, exact_sum
DEV = torch.device("cuda", 0)
GUARD, SENTINEL, UNSET, HP = {GUARD}, {SENTINEL}, {UNSET}, {HP!r}
"""


# ------------------------------------------------------------------------------------------
# Item 3: the float64 reference and its error bounds
# ------------------------------------------------------------------------------------------
def _f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


def _host_constants(b1, b2, t):
    """c1 = 1 - beta1^t and c2_sqrt = sqrt(1 - beta2^t) formed in float32 from the float32
    betas, as set_adamw_hyper forms them; the powers are the correctly rounded ones (float64 pow,
    rounded once). Returns (c1, c2_sqrt, beta1^t, beta2^t) as Python floats holding fp32 values."""
    one = torch.tensor(1.0, dtype=torch.float32)
    pw1 = torch.tensor(b1 ** t, dtype=torch.float64).float()
    pw2 = torch.tensor(b2 ** t, dtype=torch.float64).float()
    return (one - pw1).item(), (one - pw2).sqrt().item(), pw1.item(), pw2.item()


def _reference(p, m, v, g, hp, t):
    """One AdamW step in float64 from the fp32 inputs p, m, v (states) and g (the summed, scaled
    gradient), with the hyper-parameters as the kernel receives them (rounded to float32; c1 and
    c2_sqrt from `_host_constants`), and per-element bounds on what fp32 may differ by.

    Derivation, from `adamw()` in csrc/hip/xgmi_adam_device.h with u = 2^-24. Every fp32 operation
    returns its exact result times (1 + d); |d| <= u for +, -, * (an FMA contraction only
    removes roundings), and |d| <= 2u (one ulp, the documented maximum of the device's sqrtf
    and fp32 division) for sqrt and /. Terms of order u^2 are covered by the factor 1.01.

      m' = fl(fl(b1 * m) + fl(fl(1 - b1) * g)): the first product carries 1 rounding, the
           second 2 (1 - b1, then the product), the sum 1 on both:
             |err m'| <= u * (2 |b1 m| + 3 |(1 - b1) g|) =: u * Em
      v' = fl(fl(b2 * v) + fl(fl(fl(1 - b2) * g) * g)): 1 and 3 roundings, the sum 1:
             |err v'| <= u * (2 b2 v + 4 (1 - b2) g^2)           (all terms >= 0: <= 4u relative)
      denom = fl(fl(sqrt(v') / c2_sqrt) + eps): sqrt halves the 4u of v' and adds 2u, the
           division 2u, the sum 1u on the whole: |err denom| <= 7u * denom
      p1 = fl(p * fl(1 - fl(lr * wd))): with lr * wd < 1/2 the factor carries at most 2u, the
           product 1u: |err p1| <= 3u |p1| (nothing at wd = 0: p * 1)
      D  = fl(fl(fl(lr / c1) * m') / denom): 2u + 1u + 2u and the 7u of denom on |D|, and the
           error of m' scaled: |err D| <= 12u |D| + u * (lr / c1) * Em / denom
      p' = fl(p1 - D): 1u on the result
             |err p'| <= u * (3 |p1| + |p'| + 12 |D| + Dm),  Dm = (lr / c1) * Em / denom
    Without cancellation between b1 m and (1 - b1) g, Dm <= 3 |D| and the bound is within
    u * (4 |p| + 16 |D|); where the two terms of m' cancel, Dm exceeds that multiple of |D| and
    the derivation stands as it is. Host pow: the runtime's powf may differ by one ulp (2u
    relative) from the correctly rounded power used here; beta^1 = beta is exact. That moves c1
    by 2u beta1^t and 1 - beta2^t likewise, so D by |D| * (2u beta1^t / c1 + u beta2^t /
    c2_sqrt^2) (the square root halves the second), added for t > 1.
    """
    lr, wd, eps = _f32(hp["lr"]), _f32(hp["weight_decay"]), _f32(hp["eps"])
    b1, b2 = _f32(hp["betas"][0]), _f32(hp["betas"][1])
    c1, c2, pw1, pw2 = _host_constants(b1, b2, t)
    assert lr * wd < 0.5
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    t1, t2 = b1 * m, (1 - b1) * g
    m_new = t1 + t2
    v_new = b2 * v + (1 - b2) * g * g
    denom = v_new.sqrt() / c2 + eps
    a = lr / c1
    p1 = p * (1 - lr * wd)
    D = a * m_new / denom
    p_new = p1 - D
    Em = 2 * t1.abs() + 3 * t2.abs()
    Dm = a * Em / denom
    pow_slack = (2 * U * pw1 / c1 + U * pw2 / (c2 * c2)) if t > 1 else 0.0
    return {
        "exp_avg": m_new, "exp_avg_sq": v_new, "master": p_new,
        "bound_exp_avg": 1.01 * U * Em,
        "bound_exp_avg_sq": 1.01 * U * (2 * b2 * v + 4 * (1 - b2) * g * g),
        "bound_master": 1.01 * U * (3 * p1.abs() + p_new.abs() + 12 * D.abs() + Dm) + pow_slack * D.abs(),
        # the ceilings the bounds are held to (test_bounds_...): the last one wherever b1 m and
        # (1 - b1) g do not cancel by more than 6x (1.01 (4 |p| + 13 |D| + Dm) <= 8 |p| + 32 |D|
        # from Dm <= 18 |D|)
        "cap_exp_avg": 8 * U * (t1.abs() + t2.abs()),
        "cap_exp_avg_sq": 8 * U * (b2 * v + (1 - b2) * g * g),
        "cap_master": U * (8 * p.abs() + 32 * D.abs()) + pow_slack * D.abs(),
        "no_cancellation": Dm <= 18 * D.abs(),
    }


REF_CASES = [dict(lr=1e-2, betas=(0.9, 0.99), eps=eps, weight_decay=wd, t=t)
             for t in (1, 2, 10, 1000) for eps in (1e-8, 1e-3) for wd in (0.0, 0.1)]


def _reference_inputs(cpu_xs, n, P, seed, device):
    """Random fp32 states and rank gradients spanning several orders of magnitude whose fp32 sum
    is exact (grid values times a power of two per element), so that g is the same number in the
    kernel's rank-order sum and here; every 97th element has g = 0 and exp_avg_sq = 0: the
    denominator is eps alone. Returns (p, m, v, rank gradients, g = fl(sum * float32(1 / P)))."""
    gen = torch.Generator().manual_seed(seed)
    dtype = cpu_xs[0].dtype
    k = torch.randint(-6, 3, (n,), generator=gen)
    factor = torch.ldexp(torch.ones(n), k).to(dtype)
    zero = torch.arange(n) % 97 == 5
    xs = []
    for x in cpu_xs:
        y = x[:n] * factor  # a power of two: exact in every dtype here
        y[zero] = 0
        xs.append(y)
    g = exact_sum(xs, torch.float32, 1.0 / P)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * torch.ldexp(torch.ones(n), torch.randint(-8, 2, (n,), generator=gen))
    v = (torch.randn(n, generator=gen) * factor.float()) ** 2
    v[zero] = 0
    assert bool((g[zero] == 0).all()) and bool((v[zero] == 0).all())
    return [t.to(device) for t in (p, m, v)] + [[x.to(device) for x in xs], g.to(device)]


def _torch_fp32_step(p, m, v, g, hp, t):
    """`adamw()` operation by operation in torch fp32 (no FMA), with the host's constants."""
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)  # noqa: E731
    lr, wd, eps, b1, b2 = f(hp["lr"]), f(hp["weight_decay"]), f(hp["eps"]), f(hp["betas"][0]), f(hp["betas"][1])
    c1, c2, _, _ = _host_constants(b1.item(), b2.item(), t)
    one = f(1.0)
    pv = p * (one - lr * wd)
    mv = b1 * m + (one - b1) * g
    vv = b2 * v + (one - b2) * g * g
    denom = vv.sqrt() / f(c2) + eps
    pv = pv - (lr / f(c1)) * mv / denom
    return {"master": pv, "exp_avg": mv, "exp_avg_sq": vv}


def _within(got, ref, what):
    for key in ("exp_avg", "exp_avg_sq", "master"):
        err = (got[key].double() - ref[key]).abs()
        over = (~(err <= ref["bound_" + key])).nonzero().flatten()  # a NaN is over
        if over.numel():
            i = int(over[0])
            pytest.fail(f"{what}: {key} beyond its bound in {over.numel()} of {err.numel()} elements, first {i}: got "
                        f"{float(got[key][i])!r} reference {float(ref[key][i])!r} error {float(err[i]):.3e} bound "
                        f"{float(ref['bound_' + key][i]):.3e}; largest error / bound "
                        f"{float((err / ref['bound_' + key].clamp_min(1e-300)).max()):.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bounds_are_under_their_ceilings_and_hold_plain_fp32_on_the_cpu(dtype):
    """No GPU: the derived bounds stay under the ceilings set for them (exp_avg and exp_avg_sq
    everywhere, master wherever the two terms of exp_avg do not cancel - most elements), and a
    plain torch fp32 evaluation of the formula on the data the GPU test uses stays inside them."""
    for P in (3, 4):
        n = 65_539
        cpu = exact_inputs(P, n, dtype, "wide", seed=7000 + 100 * P + _es(dtype))
        p, m, v, _, g = _reference_inputs(cpu, n, P, 17 * P + n, "cpu")
        mag = g[g != 0].abs()
        assert float(mag.max() / mag.min()) > 1e3  # a few orders of magnitude
        for hp in REF_CASES:
            ref = _reference(p, m, v, g, hp, hp["t"])
            assert bool((ref["bound_exp_avg"] <= ref["cap_exp_avg"]).all())
            assert bool((ref["bound_exp_avg_sq"] <= ref["cap_exp_avg_sq"]).all())
            free = ref["no_cancellation"]
            assert float(free.double().mean()) > 0.5
            assert bool((ref["bound_master"][free] <= ref["cap_master"][free]).all())
            _within(_torch_fp32_step(p, m, v, g, hp, hp["t"]), ref, f"torch fp32 P={P} {dtype} {hp}")


# ------------------------------------------------------------------------------------------
# Item 4: the sizes reach every body of the kernel (asked of the launch planner)
# ------------------------------------------------------------------------------------------
def _reduce_units(plan, n, P):
    """Element counts of the non-empty reduce units (rank, chunk, sub-unit) of a launch."""
    out = []
    for r in range(P):
        blen = max(0, min(n - r * plan["block"], plan["block"]))
        for c in range(plan["nch"]):
            clen = max(0, min(blen - c * plan["chunk"], plan["chunk"]))
            for q in range(plan["sub"]):
                ulen = max(0, min(clen - q * plan["subchunk"], plan["subchunk"]))
                if ulen:
                    out.append(ulen)
    return out


def _coverage(knobs, sizes, P, dtype):
    es = _es(dtype)
    pack = 16 // es
    seen = set()
    for n in sizes:
        plan = H.plan_allreduce("adamw", knobs, n, es, P)
        units = _reduce_units(plan, n, P)
        if plan["nch"] >= 2:
            for r in range(P):
                blen = max(0, min(n - r * plan["block"], plan["block"]))
                if blen > plan["chunk"] and blen % plan["chunk"]:
                    seen.add("several chunks, the last one short")
        if plan["sub"] >= 2:
            seen.add("sub-units")
        if any(u // pack > 2 * 256 for u in units):
            seen.add("the unrolled loop runs twice")
        if any((u // pack) % 256 for u in units):
            seen.add("a short last run")
        if any(u % pack for u in units):
            seen.add("a scalar tail")
        if any(n <= r * plan["block"] for r in range(P)):
            seen.add("ranks with an empty block")
    return seen


class _grid:
    """The cluster at another workgroup budget, for the duration of a `with`."""

    def __init__(self, cl, grid):
        self.cl, self.grid = cl, grid

    def __enter__(self):
        self.saved = [c.grid for c in self.cl.comms]
        for c in self.cl.comms:
            c.grid = self.grid

    def __exit__(self, *exc):
        for c, g in zip(self.cl.comms, self.saved):
            c.grid = g


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_sizes_reach_every_body_of_the_kernel(P, dtype):
    cl = _cluster(P)
    seen = _coverage(cl.comms[0].knobs, _sizes(P, dtype), P, dtype)
    want = {"the unrolled loop runs twice", "a short last run", "a scalar tail"}
    if P >= 2:
        want.add("ranks with an empty block")
    if P >= 3:
        want.add("sub-units")
    if P != 8:  # 8 ranks share 64 workgroups: one chunk per block; the exact test adds a pass at 128
        want.add("several chunks, the last one short")
    assert want <= seen, want - seen
    if P == 8:
        with _grid(cl, 128):
            assert "several chunks, the last one short" in _coverage(cl.comms[0].knobs, [4099, 65_539], P, dtype)


# ------------------------------------------------------------------------------------------
# Items 1 - 3 over every rank count, dtype and size
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_gradient_reduce_is_exact(P, dtype):
    """`avg` runs at every rank count: exact_sum defines the scaled sum as the kernel forms it
    (the fp32 sum times float32(1 / P)), so 1 / 3 and 1 / 5 need no exactness."""
    cl = _cluster(P)
    cpu, xs = _data(P, dtype)
    launches = cl.comms[0].stats.adamw
    for op in ("avg", "sum"):
        g = _exact_gradient(cpu, 1.0 / P if op == "avg" else 1.0)
        for n in _sizes(P, dtype):
            for step in (1, 7):
                _exact_case(cl, xs, g, n, op, step, n + step, f"exact P={P} {dtype} n={n} {op} step {step}")
        if P == 8:  # two chunks per block (at 64 workgroups the planner gives 8 ranks one)
            with _grid(cl, 128):
                for n in (4099, 65_539):
                    _exact_case(cl, xs, g, n, op, 1, n, f"exact P=8 grid 128 {dtype} n={n} {op}")
    assert cl.comms[0].stats.adamw - launches == 2 * (2 * len(_sizes(P, dtype)) + (2 if P == 8 else 0))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_params_are_the_master_rounded_once_and_nothing_else_is_written(P, dtype):
    cl = _cluster(P)
    for n in _sizes(P, dtype):
        for op in ("avg", "sum"):
            _chain_case(cl, n, dtype, op, 13 * n + P, f"chain P={P} {dtype} n={n} {op}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_one_step_matches_the_float64_reference(P, dtype):
    """ONE launch at step t from states the test sets, every state against `_reference` inside
    its derived bounds (about two orders tighter than rtol = 1e-5)."""
    cl = _cluster(P)
    cpu, _ = _data(P, dtype)
    for n in _sizes(P, dtype):
        p, m, v, xs, g = _reference_inputs(cpu, n, P, 17 * P + n, DEV)
        for hp in REF_CASES:
            case = _make_case(cl, n, dtype, p, m, v)
            grads = [x.clone() for x in xs]
            cl.step_adamw(grads, case["params"], case["states"], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                          weight_decay=hp["weight_decay"], step=hp["t"], op="avg")
            cl.check()
            what = f"P={P} {dtype} n={n} {hp}"
            _within({k: _gather(case, k) for k in ("exp_avg", "exp_avg_sq", "master")},
                    _reference(p, m, v, g, hp, hp["t"]), what)
            _check_written(case, grads, xs, what)


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_flat_geometry(dtype):
    """Blocks of at least 2 MiB take the flat geometry (one chunk per workgroup, no sub-units):
    what the bench and ZeRO buckets run. Items 1 and 2. bf16 on 4 MiB slots; 2 * 2^20 + 5 fp32
    elements are 20 bytes more than two 4 MiB slots hold, so fp32 runs on 8 MiB slots."""
    P, n = 2, 2 * 2 ** 20 + 5
    es = _es(dtype)
    cl = _cluster(P, (4 << 20) if es == 2 else (8 << 20))
    knobs = cl.comms[0].knobs
    plan = H.plan_allreduce("adamw", knobs, n, es, P)
    assert plan["sub"] == 1 and plan["nch"] > 1 and plan["block"] * es >= knobs.flat_min, plan
    assert knobs.geom < 0 and knobs.units_per_wg == 0  # the planner's own choice, nothing forced
    cpu, xs = _data(P, dtype, n)
    for op in ("avg", "sum"):
        _exact_case(cl, xs, _exact_gradient(cpu, 0.5 if op == "avg" else 1.0), n, op, 1, 5, f"flat {dtype} {op}")
    _chain_case(cl, n, dtype, "avg", 6, f"flat {dtype} chain")


# ------------------------------------------------------------------------------------------
# Item 5: non-finite gradients
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["+inf", "-inf", "nan", "+inf and -inf"])
def test_non_finite_gradients_arrive_everywhere_and_spread_nowhere(kind, dtype):
    """An inf or NaN in ONE rank's gradient (fp16 loss scaling relies on it) makes that element
    NaN in the owner's master and in every rank's parameters, and touches no other element: all
    states elsewhere are bit-equal to the same step run without it."""
    P, n = 4, 4099
    cl = _cluster(P)
    cpu, _ = _data(P, dtype, mode="narrow")
    pack = 16 // _es(dtype)
    b = cl.comms[0].block_elems(n, dtype_code(dtype))
    pos = [0, n - 1, 5 * pack - 1, 2 * b]  # first; last (ragged tail); a pack's last; block 2's first
    assert len(set(pos)) == 4 and max(pos) < n
    clean = [x[:n].clone() for x in cpu]
    dirty = [x.clone() for x in clean]
    inf = float("inf")
    for j, i in enumerate(pos):  # a different rank at each position
        dirty[j % P][i] = {"+inf": inf, "-inf": -inf, "nan": float("nan"), "+inf and -inf": inf}[kind]
        if kind == "+inf and -inf":
            dirty[(j + 1) % P][i] = -inf
    gen = torch.Generator(device=DEV).manual_seed(99)
    p0 = torch.randn(n, device=DEV, generator=gen)
    m0 = 0.1 * torch.randn(n, device=DEV, generator=gen)
    v0 = 0.01 * torch.rand(n, device=DEV, generator=gen)
    cases = []
    for xs in (clean, dirty):
        case = _make_case(cl, n, dtype, p0, m0, v0)
        grads = [x.to(DEV) for x in xs]
        before = [x.clone() for x in grads]
        cl.step_adamw(grads, case["params"], case["states"], step=1, op="avg", **HP)
        cl.check()
        _check_written(case, grads, before, f"{kind} {dtype}")  # all ranks hold master.to(dtype): NaN included
        cases.append(case)
    ref, got = cases
    at = torch.zeros(n, dtype=torch.bool, device=DEV)
    at[pos] = True
    master = _gather(got, "master")
    assert torch.equal(master.isnan(), at), "the owner's master is NaN at the four positions and only there"
    assert bool(_gather(ref, "master").isfinite().all())
    for r in range(P):
        y = got["params"][r]
        assert torch.equal(y.isnan(), at) and bool(y[~at].isfinite().all()), f"rank {r}"
        assert torch.equal(_bits(y)[~at], _bits(ref["params"][r])[~at]), f"rank {r}: a neighbour's parameter changed"
    for key in ("master", "exp_avg", "exp_avg_sq"):
        a, w = _gather(got, key), _gather(ref, key)
        assert torch.equal(_bits(a)[~at], _bits(w)[~at]), f"{key}: a neighbour of a non-finite gradient changed"


# ------------------------------------------------------------------------------------------
# Item 6: state-access modes
# ------------------------------------------------------------------------------------------
@gpu
def test_state_access_modes_in_child_processes():
    """MXAR_ADAM_STREAM (a study knob: needs MXAR_STUDY=1) is read once per process, so each mode
    runs items 1 and 2 in a fresh child, one after the other; a failing child ends the sequence.
    Modes 0, 1, 2: the generic body for every dtype with plain / nt + write-through / nt + plain
    state access. Mode 3: the run-contiguous halves for bf16 (the default there) and, for fp32,
    the generic body with nt loads and plain stores."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = _CHILD_HEAD + "\n\n".join(inspect.getsource(f) for f in _CHILD_FUNCS)
    for mode in (0, 1, 2, 3):
        env = dict(os.environ, PYTHONPATH=root, MXAR_STUDY="1", MXAR_ADAM_STREAM=str(mode))
        r = subprocess.run([sys.executable, "-c", body + f"\n_mode_child({mode})\n"], capture_output=True, text=True,
                           timeout=120, cwd=root, env=env)
        assert r.returncode == 0 and f"mode-ok {mode}" in r.stdout, (mode, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert "MXAR_ADAM_STREAM ignored" not in r.stderr, r.stderr[-500:]  # the knob was honoured


# ------------------------------------------------------------------------------------------
# Which product of a moment update is rounded (moment() / grad_fused() in xgmi_adam_device.h)
# ------------------------------------------------------------------------------------------
def _grad_fused(plan, n, pack):
    """Per element of a world-1 launch: True where adamw_unit forms fma(1 - beta, g, fl(beta s)),
    False where it forms fma(beta, s, fl((1 - beta) g)): elements x, y of the float4s of a lane's
    second pack (pack index i of the unit with (i // 256) odd) under plain state loads, and the
    scalar tail. pack 8: the run-contiguous halves, where a run of `rows` packs holds the x..w of
    lane l's half h at h * rows * 4 + l * 4."""
    gf = torch.zeros(n, dtype=torch.bool)
    for c in range(plan["nch"]):
        clen = max(0, min(n - c * plan["chunk"], plan["chunk"]))
        for q in range(plan["sub"]):
            ulen = max(0, min(clen - q * plan["subchunk"], plan["subchunk"]))
            start = c * plan["chunk"] + q * plan["subchunk"]
            npk = ulen // pack
            j = torch.arange(npk * pack)
            if pack == 4:
                w, k = (j // 4 // 256) % 2, j % 4
            else:
                run = j // 2048
                rows = torch.clamp(npk - run * 256, max=256)
                w, k = run % 2, ((j - run * 2048) % (rows * 4)) % 4
            gf[start:start + npk * pack] = ~((w == 1) & (k < 2))
    return gf


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_moment_roundings_are_the_pinned_ones(dtype):
    """beta1 = beta2 = 0.75, so (1 - beta) g = g / 4 is exact and the two candidates of each moment
    are computable exactly in float64 (every value is a multiple of 2^-30 at least, below 2; g^2 / 4
    a multiple of 2^-16): fl(0.75 s + g / 4) with one rounding where the gradient's product is the
    rounded one, fl(fl(0.75 s) + g / 4) where the state's is; for the second moment t = fl(g^2 / 4)
    and fl(0.75 v + t) against fl(g^2 / 4 + fl(0.75 v)). The moments must have the bits of the
    candidate that grad_fused() names for the element's place, and the candidates must differ
    often enough for that to say something."""
    cl = _cluster(1)
    n, es = NMAX, _es(dtype)
    gen = torch.Generator().manual_seed(4242)
    m = torch.randint(-(2 ** 24) + 1, 2 ** 24, (n,), generator=gen).double() * 2.0 ** -24
    v = torch.randint(0, 2 ** 24, (n,), generator=gen).double() * 2.0 ** -28  # below g^2 / 4 often: two roundings show
    g = torch.randint(2, 128, (n,), generator=gen).double() * 2.0 ** -7 * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    assert torch.equal(g.to(dtype).double(), g) and torch.equal(m.float().double(), m)
    case = _make_case(cl, n, dtype, torch.zeros(n), m.float(), v.float())
    cl.step_adamw([g.to(dtype).to(DEV)], case["params"], case["states"], step=1, lr=1e-2, betas=(0.75, 0.75), eps=1e-8,
                  weight_decay=0.0)
    cl.check()
    f32 = lambda x: x.float().double()
    gf = _grad_fused(H.plan_allreduce("adamw", cl.comms[0].knobs, n, es, 1), n, 16 // es)
    assert 0.7 < gf.float().mean() < 0.9  # all but x, y of every other run of 256 packs, and the tails
    for key, grad_rounded, state_rounded in (
            ("exp_avg", (0.75 * m + g / 4).float(), (f32(0.75 * m) + g / 4).float()),
            ("exp_avg_sq", (0.75 * v + f32(g * g / 4)).float(), (g * g / 4 + f32(0.75 * v)).float())):
        assert (grad_rounded != state_rounded).float().mean() > 0.01, key
        want = torch.where(gf, state_rounded, grad_rounded)
        got = _gather(case, key).cpu()
        print(f"{key} {dtype}: {int((got != want).sum())} of {n} differ from the pinned candidate; "
              f"{int((got != grad_rounded).sum())} from 'gradient product rounded' everywhere, "
              f"{int((got != state_rounded).sum())} from 'state product rounded' everywhere")
        assert torch.equal(got, want), f"{key}: {_first_diff(got, want)}"


# ------------------------------------------------------------------------------------------
# Item 7: the communicator's wrapper
# ------------------------------------------------------------------------------------------
class _OneRank:
    """A world-1 XgmiCommunicator behind LocalCluster's step_adamw / check interface."""

    world = 1

    def __init__(self, comm, grid):
        self.comm, self.grid, self.comms = comm, grid, [comm.native]

    def step_adamw(self, grads, params, states, **kw):
        self.comm.step_adamw(grads[0], params[0], states[0], grid=self.grid, **kw)

    def check(self):
        self.comm.check()


@gpu
def test_communicator_step_with_grid_override_and_sum():
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import XgmiCommunicator, free_port

    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{free_port()}", rank=0, world_size=1)
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=SLOT, timeout_s=10.0)
        default = comm.native.grid
        assert default > 8
        for grid in (8, 0):  # the override, then back to the default
            one = _OneRank(comm, grid)
            for dtype in DTYPES:
                cpu, xs = _data(1, dtype)
                for n in (7, 4099, 65_539):
                    for op in ("sum", "avg"):
                        what = f"communicator grid={grid} {dtype} n={n} {op}"
                        _exact_case(one, xs, _exact_gradient(cpu, 1.0), n, op, 1, n, what)
                        _chain_case(one, n, dtype, op, n + 1, what)
                    assert comm.native.grid == (grid or default)
        assert comm.stats.adamw == 2 * 3 * 3 * 2 * 4
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------
# Item 8: three chained steps against PyTorch fp32 on the full vector
# ------------------------------------------------------------------------------------------
def _ref_adamw(p, m, v, g, lr, b1, b2, eps, wd, t):
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / (1 - b2 ** t) ** 0.5 + eps
    p = p - (lr / (1 - b1 ** t)) * m / denom
    return p, m, v


@gpu
@pytest.mark.parametrize("P", [1, 2, 4, 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1000, 300_003])
def test_fused_adamw_step_matches_reference(P, dtype, n):
    """Mean gradient and the AdamW formula of torch.optim.AdamW in PyTorch fp32."""
    cl = _cluster(P)
    launches = cl.comms[0].stats.adamw
    b = cl.comms[0].block_elems(n, dtype_code(dtype))
    p0 = fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=1)
    params = [p0.clone() for _ in range(P)]
    states = []
    for r in range(P):
        master = torch.zeros(b, device=DEV)
        lo, hi = r * b, min(n, (r + 1) * b)
        if hi > lo:
            master[:hi - lo] = p0[lo:hi].float()
        states.append({"master": master, "exp_avg": torch.zeros(b, device=DEV), "exp_avg_sq": torch.zeros(b, device=DEV)})
    ref_p, ref_m, ref_v = p0.float(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    hp = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    for t in range(1, 4):
        grads = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=100 * t + r) for r in range(P)]
        cl.step_adamw(grads, params, states, step=t, **hp)
        cl.check()
        g = sum(x.float() for x in grads) / P
        ref_p, ref_m, ref_v = _ref_adamw(ref_p, ref_m, ref_v, g, hp["lr"], *hp["betas"], hp["eps"],
                                         hp["weight_decay"], t)
        master_full = torch.cat([states[r]["master"][:max(0, min(n, (r + 1) * b) - r * b)] for r in range(P)])
        for r in range(P):
            lo, hi = r * b, min(n, (r + 1) * b)
            if hi > lo:
                torch.testing.assert_close(states[r]["master"][:hi - lo], ref_p[lo:hi], rtol=1e-5, atol=1e-6)
                torch.testing.assert_close(states[r]["exp_avg"][:hi - lo], ref_m[lo:hi], rtol=1e-5, atol=1e-6)
                torch.testing.assert_close(states[r]["exp_avg_sq"][:hi - lo], ref_v[lo:hi], rtol=1e-5, atol=1e-9)
            assert torch.equal(params[r], master_full.to(dtype)), (t, r)  # the master, rounded once
            if dtype == torch.float32:
                assert (params[r] - ref_p).abs().max().item() <= 1e-6, (t, r)
            assert torch.equal(params[r], params[0])  # identical on every rank
    assert cl.comms[0].stats.adamw - launches == 3
