"""The clipped sharded-DP step (csrc/hip/xgmi_clip.hip): the fused step split into a
reduce-scatter half (fp32 shard + sum of squares) and an update half (AdamW from the shard times
the clip coefficient + all-gather), with the coefficient computed between them.

All in one process on one GPU through LocalCluster, on the cached clusters, data and checks of
tests/test_adamw_gpu.py (2 MiB slots, grid 64, sentinels behind every buffer):

  1. `gshard` is the exact fp32 gradient sum of the rank's block, bit for bit, on inputs whose
     sum is exact; nothing past the valid length is written, the gradients are not written;
  2. the sum of squares is exact where every order gives the same fp32 value (each element
     non-zero on one rank at most, values +-0.5, +-1, +-2: every square and every partial sum
     is a small multiple of one power of two);
  3. the update half is bit-equal to the pinned fused step run on gradients pre-multiplied by
     the same power-of-two coefficient; three chained steps leave params = master.to(dtype) and
     write nothing else;
  4. a bound above the norm gives coef = 1.0f exactly and, at ShardedDataParallel level, the
     clipped step is bit-equal to the unclipped fused step;
  5. on random data the norm and the coefficient stay inside the bound the kernel file derives
     from the depth of its summation tree (the float64 value is the reference);
  6. an inf / NaN in one rank's gradient gives an inf / NaN norm and coef 0 / NaN, and no buffer
     is written outside its valid range;
  7. the XgmiCommunicator wrappers, with the `grid=` override and the default grid.

Items 1 - 4 hold no tolerance at all."""
import math

import pytest
import torch

import test_adamw_gpu as A
from akka_allreduce_1_amd.ops import dtype_code
from akka_allreduce_1_amd.utils.exact_data import exact_inputs, exact_sum

gpu = pytest.mark.gpu
H, DEV, U = A.H, A.DEV, A.U
GUARD, SENTINEL, HP, NMAX = A.GUARD, A.SENTINEL, A.HP, A.NMAX
WORLDS, DTYPES = A.WORLDS, A.DTYPES
_POW2: dict = {}


# ------------------------------------------------------------------------------------------
# The bound of the sum of squares, from the tree documented in csrc/hip/xgmi_clip.hip
# ------------------------------------------------------------------------------------------
def _depth(L, dtype):
    """Longest chain of additions for a reduce unit of L elements: iters(L) + log2(U * EL) + 12,
    EL = elements per 16-B pack, U = 2 packs per lane per iteration, 256 lanes."""
    el = 16 // A._es(dtype)
    iters = -(-(L // el) // (2 * 256))
    return iters + int(math.log2(2 * el)) + 12


def _sq_bound(L, dtype):
    """Relative error of a rank's sum of squares at most (all terms are non-negative): depth
    roundings of relative size u each; 1.01 covers the terms of order u^2."""
    return 1.01 * _depth(L, dtype) * U


def _max_unit(knobs, n, P, dtype):
    plan = H.plan_allreduce("adamw", knobs, n, A._es(dtype), P)
    return max(A._reduce_units(plan, n, P))


def _block(P, n, dtype):
    pack = 16 // A._es(dtype)
    return -(-(-(-n // P)) // pack) * pack


@pytest.mark.parametrize("dtype", DTYPES)
def test_derived_bound_is_small_and_holds_plain_fp32_on_the_cpu(dtype):
    """No GPU. A unit is never longer than the rank's block, and the depth grows with the
    length: the bound at L = block covers every geometry the planner can choose for the sizes of
    this file, and stays far under 1e-3; so does the documented figure at 2^28 elements per
    rank (256 workgroups: L = 2^20) and an explicit grid of 8 (L = 2^25). A plain torch fp32
    evaluation of the sum of squares of the data item 5 uses sits inside the bound."""
    for P in WORLDS:
        for n in A._sizes(P, dtype):
            assert _sq_bound(_block(P, n, dtype), dtype) < 1e-3
    assert _sq_bound(_block(1, NMAX, dtype), dtype) < 2e-5
    assert _sq_bound(2 ** 20, dtype) < 4e-5 and _sq_bound(2 ** 25, dtype) < 1e-3
    for P in (3, 4):
        cpu = exact_inputs(P, NMAX, dtype, "wide", seed=7000 + 100 * P + A._es(dtype))
        g = exact_sum(cpu, torch.float32, 1.0 / P)
        b = _block(P, NMAX, dtype)
        for r in range(P):
            blk = g[r * b:min(NMAX, (r + 1) * b)]
            ref = float(blk.double().pow(2).sum())
            got = float((blk * blk).sum())
            assert abs(got - ref) <= _sq_bound(blk.numel(), dtype) * ref, (P, r, got, ref)


# ------------------------------------------------------------------------------------------
# Buffers and checks
# ------------------------------------------------------------------------------------------
def _valid(n, b, r):
    return max(0, min(n, (r + 1) * b) - r * b)


def _gshards(cl, n, dtype):
    """One fp32 shard buffer per rank, SENTINEL everywhere, GUARD more elements behind it."""
    b = cl.comms[0].block_elems(n, dtype_code(dtype))
    bufs = [torch.full((b + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(cl.world)]
    return b, bufs, [x[:b] for x in bufs]


def _check_gshards(bufs, n, b, what):
    for r, buf in enumerate(bufs):
        assert bool((buf[_valid(n, b, r):] == SENTINEL).all()), f"{what} rank {r}: gshard written past its valid length"


def _full(gs, n, b):
    return torch.cat([g[:_valid(n, b, r)] for r, g in enumerate(gs)])


def _rs_sq(cl, xs, n, op, what):
    """reduce_scatter_sq on clones of xs[:n]; checks what must not be written. Returns
    (b, gshards, sqs)."""
    grads = [x[:n].clone() for x in xs]
    b, bufs, gs = _gshards(cl, n, xs[0].dtype)
    sqs = cl.reduce_scatter_sq(grads, gs, op=op)
    cl.check()
    _check_gshards(bufs, n, b, what)
    for r in range(cl.world):
        assert torch.equal(A._bits(grads[r]), A._bits(xs[r][:n])), f"{what} rank {r}: the gradient was written"
        assert sqs[r].dtype == torch.float32 and sqs[r].numel() == 1
    return b, gs, sqs


# ------------------------------------------------------------------------------------------
# The sizes reach every body of both kernels (asked of the launch planner)
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_sizes_reach_every_body_of_both_kernels(P, dtype):
    """Both halves run on the `adamw` plan: the pack loop twice and with a short last run (the
    16-bit update body splits it into halves), the scalar tail, empty blocks, sub-units, several
    chunks; and, for the last workgroup's sum over the partials, more than one batch of 64."""
    cl = A._cluster(P)
    seen = A._coverage(cl.comms[0].knobs, A._sizes(P, dtype), P, dtype)
    want = {"the unrolled loop runs twice", "a short last run", "a scalar tail"}
    if P >= 2:
        want.add("ranks with an empty block")
    if P >= 3:
        want.add("sub-units")
    if P != 8:
        want.add("several chunks, the last one short")
    assert want <= seen, want - seen
    if P == 8:
        with A._grid(cl, 128):
            assert "several chunks, the last one short" in A._coverage(cl.comms[0].knobs, [4099, 65_539], P, dtype)
    if P == 1:
        with A._grid(cl, 128):
            plan = H.plan_allreduce("adamw", cl.comms[0].knobs, NMAX, A._es(dtype), 1)
            assert plan["nch"] * plan["sub"] > 64, plan


# ------------------------------------------------------------------------------------------
# Item 1
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_gshard_is_the_exact_gradient_sum(P, dtype):
    cl = A._cluster(P)
    cpu, xs = A._data(P, dtype)
    before = (cl.comms[0].stats.rs_sq, cl.comms[0].stats.adamw, cl.comms[0].stats.coll)
    runs = 0
    for op in ("avg", "sum"):
        g = A._exact_gradient(cpu, 1.0 / P if op == "avg" else 1.0)
        grids = [None] + ([128] if P in (1, 8) else [])
        for grid in grids:
            for n in (A._sizes(P, dtype) if grid is None else [65_539, NMAX]):
                what = f"gshard P={P} {dtype} n={n} {op} grid {grid}"
                if grid is None:
                    b, gs, sqs = _rs_sq(cl, xs, n, op, what)
                else:
                    with A._grid(cl, grid):
                        b, gs, sqs = _rs_sq(cl, xs, n, op, what)
                runs += 1
                got = _full(gs, n, b)
                assert torch.equal(got, g[:n]), f"{what}: {A._first_diff(got, g[:n])}"
                for r in range(P):  # and the sum of squares inside its bound
                    blk = g[r * b:min(n, (r + 1) * b)].double()
                    ref = float(blk.pow(2).sum())
                    assert abs(float(sqs[r]) - ref) <= _sq_bound(max(1, blk.numel()), dtype) * ref, (what, r)
    st = cl.comms[0].stats
    assert (st.rs_sq - before[0], st.adamw - before[1], st.coll - before[2]) == (runs, 0, 0)


# ------------------------------------------------------------------------------------------
# Item 2
# ------------------------------------------------------------------------------------------
def _pow2_data(P, dtype, n=NMAX):
    """Each element non-zero on one rank at most (about one in P + 1 is zero on every rank),
    values +-0.5, +-1, +-2. Returns (owner, value, gpu rank tensors)."""
    if (P, dtype) not in _POW2:
        gen = torch.Generator().manual_seed(4100 + 10 * P + A._es(dtype))
        owner = torch.randint(-1, P, (n,), generator=gen)
        vals = torch.tensor([0.5, 1.0, 2.0, -0.5, -1.0, -2.0])[torch.randint(0, 6, (n,), generator=gen)]
        xs = [torch.where(owner == k, vals, torch.zeros(())).to(dtype).to(DEV) for k in range(P)]
        _POW2[P, dtype] = (owner, vals, xs)
    return _POW2[P, dtype]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_sum_of_squares_is_exact(P, dtype):
    """Every square is (1/4, 1 or 4) * scale^2 with scale a power of two, so every partial sum of
    at most 300 003 of them is a multiple of scale^2 / 4 below 2^24 of that unit: exact in fp32
    in every order. Per-rank sq and the norm of the total equal the float64 values."""
    cl = A._cluster(P)
    owner, vals, xs = _pow2_data(P, dtype)
    for op in ("sum", "avg") if P in (2, 4, 8) else ("sum",):
        scale = 1.0 / P if op == "avg" else 1.0
        grids = [None] + ([128] if P == 1 else [])  # P = 1 at 128 workgroups: 128 partials, two batches
        for grid in grids:
            for n in (A._sizes(P, dtype) if grid is None else [NMAX]):
                what = f"sq P={P} {dtype} n={n} {op} grid {grid}"
                if grid is None:
                    b, gs, sqs = _rs_sq(cl, xs, n, op, what)
                else:
                    with A._grid(cl, grid):
                        b, gs, sqs = _rs_sq(cl, xs, n, op, what)
                sq64 = torch.where(owner[:n] >= 0, (vals[:n].double() * scale) ** 2, torch.zeros((), dtype=torch.float64))
                total = 0.0
                for r in range(P):
                    ref = sq64[r * b:min(n, (r + 1) * b)].sum()
                    total += float(ref)
                    assert torch.equal(sqs[r].cpu(), ref.float().reshape(1)), (what, r, float(sqs[r]), float(ref))
                norms, coefs = cl.clip_coef(sqs, 1e30)
                for r in range(P):
                    assert norms[r].dim() == 0 and norms[r].dtype == torch.float32
                    assert float(norms[r]) == float(torch.tensor(total, dtype=torch.float64).sqrt().float()), (what, r)
                    assert float(coefs[r]) == 1.0  # item 4: nothing to clip, exactly 1.0f


# ------------------------------------------------------------------------------------------
# Item 3
# ------------------------------------------------------------------------------------------
def _states(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(n, device=DEV, generator=gen), 0.1 * torch.randn(n, device=DEV, generator=gen),
            0.01 * torch.rand(n, device=DEV, generator=gen))


def _check_written(case, gbufs, what):
    """A._check_written without its gradient check (the update half takes no gradient), plus the
    shard buffers' sentinels."""
    n, b, dtype = case["n"], case["b"], case["dtype"]
    want = A._gather(case, "master").to(dtype)
    for r in range(case["P"]):
        assert A._same(case["params"][r], want), f"{what} rank {r}: params != master.to(dtype): " \
                                                 f"{A._first_diff(case['params'][r], want)}"
        assert bool((case["bufs"][r][n:] == SENTINEL).all()), f"{what} rank {r}: wrote past the end of params"
        for key, t in case["states"][r].items():
            assert bool((t[_valid(n, b, r):] == SENTINEL).all()), f"{what} rank {r}: wrote {key} past its valid elements"
    _check_gshards(gbufs, n, b, what)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_update_half_equals_the_fused_step_bit_for_bit(P, dtype):
    """coef = 2^-j: the fused step on gradients pre-multiplied by 2^-j forms (sum x 2^-j) * scale,
    the split step ((sum x) * scale) * 2^-j - the same fp32 number while nothing underflows (the
    narrow grid: multiples of 2^-10 below 2^-2 in bf16, 2 in fp16; 2^-13 at least after the
    coefficient, far above the smallest fp16 subnormal 2^-24). Everything after it is adamw().

    The two kernels are compiled separately; both run the one adamw_unit of
    csrc/hip/xgmi_adam_device.h, whose moment() fixes which product of a moment update is rounded
    (fma(beta1, m, fl((1 - beta1) g)) or fma(1 - beta1, g, fl(beta1 m)), by the element's place),
    and differ only in the gradient source (the P-way sum or the fp32 shard), which this test
    holds against each other; the figures are printed for the day it stops holding."""
    cl = A._cluster(P)
    cpu, xs = A._data(P, dtype, mode="narrow")
    before = (cl.comms[0].stats.rs_sq, cl.comms[0].stats.adamw_shard)
    runs = 0
    unequal = []
    for n in A._sizes(P, dtype):
        p0, m0, v0 = _states(n, 31 * n + P)
        for op in ("avg", "sum"):
            for j in (0, 1, 3):
                what = f"update P={P} {dtype} n={n} {op} coef 2^-{j}"
                fused = A._make_case(cl, n, dtype, p0, m0, v0)
                scaled = [(x[:n] * 2.0 ** -j).contiguous() for x in xs]
                assert all(torch.equal(s.double() * 2.0 ** j, x[:n].double()) for s, x in zip(scaled, xs))
                cl.step_adamw(scaled, fused["params"], fused["states"], step=2, op=op, **HP)
                split = A._make_case(cl, n, dtype, p0, m0, v0)
                b, gbufs, gs = _gshards(cl, n, dtype)
                cl.reduce_scatter_sq([x[:n].clone() for x in xs], gs, op=op)
                coef = [torch.tensor(2.0 ** -j, dtype=torch.float32, device=DEV) for _ in range(P)]
                cl.step_adamw_shard(gs, split["params"], split["states"], coef=coef, step=2, **HP)
                cl.check()
                runs += 1
                for key in ("master", "exp_avg", "exp_avg_sq"):  # the figures; asserted after every case ran
                    got, want = A._gather(split, key), A._gather(fused, key)
                    ulps = (A._bits(got).long() - A._bits(want).long()).abs()
                    print(f"{what}: {key}: {int((ulps != 0).sum())} of {n} differ, at most {int(ulps.max())} ulp")
                    if not torch.equal(A._bits(got), A._bits(want)):
                        unequal.append(f"{what}: {key}: {A._first_diff(got, want)}")
                for r in range(P):
                    if not torch.equal(A._bits(split["params"][r]), A._bits(fused["params"][r])):
                        unequal.append(f"{what}: params of rank {r}")
                _check_written(split, gbufs, what)
    st = cl.comms[0].stats
    assert (st.rs_sq - before[0], st.adamw_shard - before[1]) == (runs, runs)
    assert not unequal, f"{len(unequal)} differences from the fused step, first: {unequal[0]}"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_update_half_matches_the_float64_reference(P, dtype):
    """The update half against the float64 evaluation and the error bounds tests/test_adamw_gpu.py
    derives from the operation count of adamw() for the fused step (`_reference`): the gradient
    is the same fp32 number (exact data; the coefficient 1/2 is exact), so the same bounds hold."""
    cl = A._cluster(P)
    cpu, _ = A._data(P, dtype)
    for n in A._sizes(P, dtype):
        p, m, v, xs, g = A._reference_inputs(cpu, n, P, 17 * P + n, DEV)
        b, gs, sqs = _rs_sq(cl, xs, n, "avg", f"reference P={P} {dtype} n={n}")
        assert torch.equal(_full(gs, n, b), g)
        coef = [torch.tensor(0.5, device=DEV) for _ in range(P)]
        for hp in A.REF_CASES[::3]:
            what = f"reference P={P} {dtype} n={n} {hp}"
            case = A._make_case(cl, n, dtype, p, m, v)
            cl.step_adamw_shard(gs, case["params"], case["states"], coef=coef, lr=hp["lr"], betas=hp["betas"],
                                eps=hp["eps"], weight_decay=hp["weight_decay"], step=hp["t"])
            cl.check()
            A._within({k: A._gather(case, k) for k in ("exp_avg", "exp_avg_sq", "master")},
                      A._reference(p, m, v, g * 0.5, hp, hp["t"]), what)
            _check_written(case, [x._base for x in gs], what)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_three_chained_clipped_steps_write_params_and_nothing_else(P, dtype):
    """Random gradients, the coefficient from clip_coef with a bound that clips: after every step
    params = master.to(dtype) on every rank; nothing past n, past the valid shard length, in the
    gradients or in the shard buffers' padding is written; the master moves."""
    cl = A._cluster(P)
    for n in A._sizes(P, dtype):
        gen = torch.Generator(device=DEV).manual_seed(17 * n + P)
        p0 = torch.randn(n, device=DEV, generator=gen).to(dtype).float()
        m0 = 0.1 * torch.randn(n, device=DEV, generator=gen)
        v0 = 0.01 * torch.rand(n, device=DEV, generator=gen)
        case = A._make_case(cl, n, dtype, p0, m0, v0)
        last = p0
        for t in range(1, 4):
            what = f"chain P={P} {dtype} n={n} step {t}"
            xs = [torch.randn(n, device=DEV, generator=gen).to(dtype) for _ in range(P)]
            b, gs, sqs = _rs_sq(cl, xs, n, "avg", what)
            gbufs = [g._base if g._base is not None else g for g in gs]
            norms, coefs = cl.clip_coef(sqs, 0.25 * math.sqrt(n) / math.sqrt(P))
            assert all(torch.equal(c, coefs[0]) for c in coefs) and 0 < float(coefs[0]) <= 1, what
            cl.step_adamw_shard(gs, case["params"], case["states"], coef=coefs, step=t, **HP)
            cl.check()
            _check_written(case, gbufs, what)
            now = A._gather(case, "master")
            assert bool(now.isfinite().all()) and not torch.equal(now, last), f"{what}: the master did not move"
            last = now


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_flat_geometry(dtype):
    """Blocks of at least 2 MiB (what ZeRO buckets run): item 1, and the update half against the
    float64 reference and bit for bit against the fused step, on the flat geometry."""
    P, n = 2, 2 * 2 ** 20 + 5
    es = A._es(dtype)
    cl = A._cluster(P, (4 << 20) if es == 2 else (8 << 20))
    plan = H.plan_allreduce("adamw", cl.comms[0].knobs, n, es, P)
    assert plan["sub"] == 1 and plan["nch"] > 1 and plan["block"] * es >= cl.comms[0].knobs.flat_min, plan
    cpu, xs = A._data(P, dtype, n)
    g = A._exact_gradient(cpu, 0.5)
    b, gs, sqs = _rs_sq(cl, xs, n, "avg", f"flat {dtype}")
    assert torch.equal(_full(gs, n, b), g[:n])
    L = max(A._reduce_units(plan, n, P))
    for r in range(P):
        ref = float(g[r * b:min(n, (r + 1) * b)].double().pow(2).sum())
        assert abs(float(sqs[r]) - ref) <= _sq_bound(L, dtype) * ref
    p0, m0, v0 = _states(n, 5)
    case = A._make_case(cl, n, dtype, p0, m0, v0)
    coef = [torch.tensor(0.5, device=DEV) for _ in range(P)]
    hp = A.REF_CASES[3]
    cl.step_adamw_shard(gs, case["params"], case["states"], coef=coef, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                        weight_decay=hp["weight_decay"], step=hp["t"])
    cl.check()
    A._within({k: A._gather(case, k) for k in ("exp_avg", "exp_avg_sq", "master")},
              A._reference(p0, m0, v0, g[:n] * 0.5, hp, hp["t"]), f"flat {dtype}")
    _check_written(case, [x._base for x in gs], f"flat {dtype}")
    fused, split = A._make_case(cl, n, dtype, p0, m0, v0), A._make_case(cl, n, dtype, p0, m0, v0)
    cl.step_adamw([(x * 0.5).contiguous() for x in xs], fused["params"], fused["states"], step=1, op="avg", **HP)
    cl.step_adamw_shard(gs, split["params"], split["states"], coef=coef, step=1, **HP)
    cl.check()
    for key in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(A._bits(A._gather(split, key)), A._bits(A._gather(fused, key))), key
    for r in range(P):
        assert torch.equal(A._bits(split["params"][r]), A._bits(fused["params"][r])), r


# ------------------------------------------------------------------------------------------
# Item 5
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_norm_and_coefficient_on_random_data_stay_inside_the_derived_bound(P, dtype):
    """Random grid data (wide: the fp32 gradient is the same number here and in the kernel), mean.
    Each rank's sum of squares carries at most depth(L) roundings for the launch's longest unit
    L; the total is formed in float64; the square root and its rounding to fp32 add 2u; the
    coefficient's add and divide 3u more. Every rank holds the same bits."""
    cl = A._cluster(P)
    cpu, xs = A._data(P, dtype)
    g = A._exact_gradient(cpu, 1.0 / P).double()
    for n in A._sizes(P, dtype):
        what = f"random P={P} {dtype} n={n}"
        b, gs, sqs = _rs_sq(cl, xs, n, "avg", what)
        bound = _sq_bound(_max_unit(cl.comms[0].knobs, n, P, dtype), dtype)
        assert bound < 1e-3
        total = 0.0
        for r in range(P):
            ref = float(g[r * b:min(n, (r + 1) * b)].pow(2).sum())
            total += ref
            print(f"{what} rank {r}: sq {float(sqs[r])!r} ref {ref!r} bound {bound:.3e}")
            assert abs(float(sqs[r]) - ref) <= bound * ref, (what, r, float(sqs[r]), ref)
        ref_norm = math.sqrt(total)
        max_norm = 0.5 * ref_norm
        ref_coef = min(1.0, max_norm / (ref_norm + 1e-6))
        norms, coefs = cl.clip_coef(sqs, max_norm)
        print(f"{what}: norm {float(norms[0])!r} ref {ref_norm!r} coef {float(coefs[0])!r} ref {ref_coef!r}")
        assert abs(float(norms[0]) - ref_norm) <= (bound + 2 * U) * ref_norm, what
        assert abs(float(coefs[0]) - ref_coef) <= (bound + 5 * U) * ref_coef, what
        for r in range(1, P):
            assert torch.equal(norms[r], norms[0]) and torch.equal(coefs[r], coefs[0]), (what, r)


# ------------------------------------------------------------------------------------------
# Item 6
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["+inf", "nan"])
def test_non_finite_gradient_gives_a_non_finite_norm_and_writes_nothing_stray(kind, dtype):
    """torch's clip_grad_norm_ with error_if_nonfinite=False: an inf norm gives coef 0 (and 0 *
    inf = NaN at that element), a NaN norm NaN everywhere."""
    P, n = 4, 4099
    cl = A._cluster(P)
    cpu, _ = A._data(P, dtype, mode="narrow")
    xs = [x[:n].clone() for x in cpu]
    xs[1][n - 1] = float("inf") if kind == "+inf" else float("nan")  # the ragged tail of the last block
    xs = [x.to(DEV) for x in xs]
    b, gs, sqs = _rs_sq(cl, xs, n, "avg", f"{kind} {dtype}")
    norms, coefs = cl.clip_coef(sqs, 1.0)
    for r in range(P):
        if kind == "+inf":
            assert float(norms[r]) == float("inf") and float(coefs[r]) == 0.0, r
        else:
            assert bool(norms[r].isnan()) and bool(coefs[r].isnan()), r
    owner = (n - 1) // b
    assert all(bool(sqs[r].isfinite()) == (r != owner) for r in range(P))
    p0, m0, v0 = _states(n, 99)
    case = A._make_case(cl, n, dtype, p0, m0, v0)
    cl.step_adamw_shard(gs, case["params"], case["states"], coef=coefs, step=1, **HP)
    cl.check()
    _check_written(case, [x._base for x in gs], f"{kind} {dtype}")  # NaN included: params = master.to(dtype)
    master = A._gather(case, "master")
    if kind == "+inf":
        at = torch.zeros(n, dtype=torch.bool, device=DEV)
        at[n - 1] = True
        assert torch.equal(master.isnan(), at)
    else:
        assert bool(master.isnan().all())


# ------------------------------------------------------------------------------------------
# Items 4 and 7: the communicator's wrappers and ShardedDataParallel, world 1
# ------------------------------------------------------------------------------------------
class _OneRank:
    """A world-1 XgmiCommunicator behind LocalCluster's interface for the clipped step."""

    world = 1

    def __init__(self, comm, grid):
        self.comm, self.grid, self.comms = comm, grid, [comm.native]

    def step_adamw(self, grads, params, states, **kw):
        self.comm.step_adamw(grads[0], params[0], states[0], grid=self.grid, **kw)

    def reduce_scatter_sq(self, grads, gshards, *, op="avg"):
        return [self.comm.reduce_scatter_sq(grads[0], gshards[0], op=op, grid=self.grid)]

    def clip_coef(self, sqs, max_norm):
        norm, coef = self.comm.clip_coef(sqs[0], max_norm)
        return [norm], [coef]

    def step_adamw_shard(self, gshards, params, states, *, coef, **kw):
        self.comm.step_adamw_shard(gshards[0], params[0], states[0], coef=coef[0], grid=self.grid, **kw)

    def check(self):
        self.comm.check()


def _one_process_group():
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import free_port

    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{free_port()}", rank=0, world_size=1)
    return dist


@gpu
def test_communicator_wrappers_with_grid_override():
    from akka_allreduce_1_amd.parallel import XgmiCommunicator

    dist = _one_process_group()
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=A.SLOT, timeout_s=10.0)
        default = comm.native.grid
        assert default > 8
        runs = 0
        for grid in (8, 0):  # the override, then back to the default
            one = _OneRank(comm, grid)
            for dtype in DTYPES:
                cpu, xs = A._data(1, dtype, mode="narrow")
                g = A._exact_gradient(cpu, 1.0)
                for n in (7, 4099, 65_539):
                    what = f"communicator grid={grid} {dtype} n={n}"
                    b, gs, sqs = _rs_sq(one, xs, n, "avg", what)
                    assert comm.native.grid == (grid or default)
                    assert torch.equal(_full(gs, n, b), g[:n]), what
                    ref = float(g[:n].double().pow(2).sum())
                    ref_norm = math.sqrt(ref)
                    norms, coefs = one.clip_coef(sqs, 0.5 * ref_norm)
                    ref_coef = 0.5 * ref_norm / (ref_norm + 1e-6)
                    bound = _sq_bound(n, dtype)
                    assert abs(float(norms[0]) - ref_norm) <= (bound + 2 * U) * ref_norm, what
                    assert abs(float(coefs[0]) - ref_coef) <= (bound + 5 * U) * ref_coef, what
                    # the update half against the float64 reference
                    p0, m0, v0 = _states(n, n + 1)
                    split = A._make_case(one, n, dtype, p0, m0, v0)
                    half = [torch.tensor([0.5], device=DEV)]
                    one.step_adamw_shard(gs, split["params"], split["states"], coef=half, step=1, **HP)
                    one.check()
                    assert comm.native.grid == (grid or default)
                    A._within({k: A._gather(split, k) for k in ("exp_avg", "exp_avg_sq", "master")},
                              A._reference(p0, m0, v0, g[:n] * 0.5, HP, 1), what)
                    _check_written(split, [x._base for x in gs], what)
                    runs += 1
        assert (comm.stats.rs_sq, comm.stats.adamw_shard, comm.stats.adamw) == (runs, runs, 0)
        with pytest.raises(ValueError):
            comm.step_adamw_shard(gs[0], split["params"][0], split["states"][0], coef=torch.ones(2, device=DEV), step=1,
                                  **HP)
        with pytest.raises(ValueError):
            comm.reduce_scatter_sq(xs[0][:n], gs[0][:-4])
    finally:
        dist.destroy_process_group()


def _net(dtype):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.Tanh(), torch.nn.Linear(96, 64), torch.nn.Tanh(),
                               torch.nn.Linear(64, 10)).to(DEV).to(dtype)


@gpu
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sharded_step_without_clipping_is_the_unclipped_fused_step(dtype, overlap):
    """max_grad_norm above the norm: coef is exactly 1.0f and three clipped steps leave the same
    bits as three unclipped fused steps. Then a low bound clips (the runs part), and an inf and a
    NaN gradient show in last_grad_norm. Checkpoints carry no gshard.

    The bit-for-bit comparison is asserted last, after every other check of this test."""
    from akka_allreduce_1_amd.parallel import ShardedDataParallel, XgmiCommunicator

    dist = _one_process_group()
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=A.SLOT, timeout_s=10.0)
        fused = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
        ma, mb, mc = _net(dtype), _net(dtype), _net(dtype)
        za = ShardedDataParallel(ma, comm, None, bucket_bytes=16 << 10, fused_adamw=fused, max_grad_norm=1e9,
                                 overlap=overlap)
        zb = ShardedDataParallel(mb, comm, None, bucket_bytes=16 << 10, fused_adamw=fused, overlap=overlap)
        zc = ShardedDataParallel(mc, comm, None, bucket_bytes=16 << 10, fused_adamw=fused, max_grad_norm=1e-3,
                                 overlap=overlap)
        assert len(za.buckets) > 1
        with pytest.raises(ValueError, match="max_grad_norm"):
            ShardedDataParallel(_net(dtype), comm, None, fused_adamw=fused, step_in_backward=True, max_grad_norm=1.0)
        x = torch.randn(32, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(dtype)
        launches = (comm.stats.rs_sq, comm.stats.adamw_shard, comm.stats.adamw)
        unequal = []
        for step in range(3):
            for mm, zz in ((ma, za), (mb, zb), (mc, zc)):
                zz.zero_grad()
                mm(x * (step + 1)).float().pow(2).mean().backward()
                zz.step()
            comm.check()
            assert za.last_clip_coef.dim() == 0 and za.last_clip_coef.dtype == torch.float32
            assert float(za.last_clip_coef) == 1.0 and float(za.last_grad_norm) > 0
            assert 0 < float(zc.last_clip_coef) < 1.0
            for i, (p, p2) in enumerate(zip(ma.parameters(), mb.parameters())):
                if not torch.equal(A._bits(p.data), A._bits(p2.data)):  # asserted last: the rest runs first
                    ulps = (A._bits(p.data).long() - A._bits(p2.data).long()).abs()
                    unequal.append(f"step {step} parameter {i}: {int((ulps != 0).sum())} of {p.numel()} differ, "
                                   f"at most {int(ulps.max())} ulp")
        assert any(not torch.equal(p.data, p2.data) for p, p2 in zip(mc.parameters(), mb.parameters()))
        nb = len(za.buckets)
        assert (comm.stats.rs_sq - launches[0], comm.stats.adamw_shard - launches[1],
                comm.stats.adamw - launches[2]) == (6 * nb, 6 * nb, 3 * nb)
        assert za.stats["clip_bytes"] == 3 * 8 * sum(b.numel for b in za.buckets) and zb.stats["clip_bytes"] == 0
        assert all(d["gshard_bytes"] == 4 * d["shard"] for d in za.describe())
        assert all(d["gshard_bytes"] == 0 for d in zb.describe())
        assert set(za.state_dict()) == set(zb.state_dict()) and set(za.state_dict()["adamw"][0]) == {
            "master", "exp_avg", "exp_avg_sq"}
        for bad in (float("inf"), float("nan")):  # one element of one parameter's gradient
            def poison(g, bad=bad):
                g = g.clone()
                g.view(-1)[3] = bad
                return g

            hook = next(mc.parameters()).register_hook(poison)
            zc.zero_grad()
            mc(x).float().pow(2).mean().backward()
            hook.remove()
            zc.step()
            comm.check()
            if bad == float("inf"):
                assert float(zc.last_grad_norm) == float("inf") and float(zc.last_clip_coef) == 0.0
            else:
                assert bool(zc.last_grad_norm.isnan()) and bool(zc.last_clip_coef.isnan())
        print("\n".join(unequal))
        assert not unequal, f"clipped (coef = 1) and unclipped fused steps differ: {unequal[:3]}"
    finally:
        dist.destroy_process_group()
