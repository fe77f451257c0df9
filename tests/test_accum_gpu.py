"""Gradient accumulation on the fused sharded-DP path: the accumulating mode of the reduce-scatter
half (csrc/hip/xgmi_clip.hip, `reduce_scatter_sq(..., accumulate=True)`) and
`ShardedDataParallel(grad_accumulation=True)`.

All in one process on one GPU through LocalCluster, on the cached clusters, sizes and checks of
tests/test_adamw_gpu.py and tests/test_clip_gpu.py (2 MiB slots, grid 64, sentinels behind every
buffer):

  1. the value rule gshard = fl32(gshard + fl32(scale * S)), bit for bit, on two micro-batches of
     exact inputs: the expectation is g1 + g2 in CPU fp32. At P = 3 and 5 (scale 1/3, 1/5) a
     contracted multiply-add gives other bits; a CPU test shows the inputs tell the two apart;
  2. on random data the accumulating launch equals `old + plain launch` in torch fp32 on the GPU,
     and accumulating into zeros equals the plain launch;
  3. the sum of squares is that of the NEW shard values: inside the bound the kernel file derives
     (tests/test_clip_gpu.py `_sq_bound`), exact on the power-of-two data;
  4. nothing stray is read for effect or written: sentinels, elements past a block's valid length
     (empty blocks included), the gradients; three launches chained without a host sync;
  5. the XgmiCommunicator wrapper with the `grid=` override, the counters, the argument checks;
  6. ShardedDataParallel at world 1: bit-equal to autograd's own fp32 accumulation, the fp32
     accumulator of bf16 gradients, launch counts, a step without accumulate(), the refusals.

Items 1, 2, 4 and 6 hold no tolerance at all."""
import pytest
import torch

import test_adamw_gpu as A
import test_clip_gpu as C
from akka_allreduce_1_amd.utils.exact_data import exact_inputs, exact_sum

gpu = pytest.mark.gpu
DEV, SENTINEL, NMAX = A.DEV, A.SENTINEL, A.NMAX
WORLDS, DTYPES = A.WORLDS, A.DTYPES
_BATCHES: dict = {}


def _batches_cpu(P, dtype):
    """Two micro-batches of exact inputs, each with its own seed (CPU rank tensors), and
    want = g1 + g2 in CPU fp32 (g = the exact sum times float32(1 / P)). Made once."""
    if (P, dtype) not in _BATCHES:
        cpus = [exact_inputs(P, NMAX, dtype, "wide", seed=9100 + 1000 * k + 100 * P + A._es(dtype)) for k in range(2)]
        g1, g2 = (exact_sum(cpu, torch.float32, 1.0 / P) for cpu in cpus)
        _BATCHES[P, dtype] = (cpus, g1 + g2)
    return _BATCHES[P, dtype]


def _batches(P, dtype):
    """(cpu micro-batches, the same on the GPU, want), the GPU copies made once and never written."""
    if (P, dtype, "gpu") not in _BATCHES:
        cpus, want = _batches_cpu(P, dtype)
        _BATCHES[P, dtype, "gpu"] = (cpus, [[x.to(DEV) for x in cpu] for cpu in cpus], want)
    return _BATCHES[P, dtype, "gpu"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_exact_inputs_tell_a_contracted_multiply_add_from_the_value_rule(dtype):
    """No GPU. The fma mutant fl32(scale * S2 + g1), one rounding (formed in float64: the product
    of two fp32 numbers is exact there), differs from the rule's fl32(g1 + fl32(scale * S2)) on a
    good part of the elements at P = 3; at a power-of-two P the two agree everywhere."""
    for P in (3, 4):
        cpus, want = _batches_cpu(P, dtype)
        g1 = exact_sum(cpus[0], torch.float32, 1.0 / P)
        S2 = exact_sum(cpus[1], torch.float32)
        s = torch.tensor(1.0 / P, dtype=torch.float32)
        mutant = (S2.double() * s.double() + g1.double()).float()
        differ = float((mutant != want).double().mean())
        print(f"P={P} {dtype}: the fma mutant differs in {differ:.3f} of the elements")
        assert (differ > 0.05) if P == 3 else (differ == 0.0), (P, differ)


# ------------------------------------------------------------------------------------------
# One launch with everything item 4 asks checked around it
# ------------------------------------------------------------------------------------------
def _launch(cl, xs, n, bufs, gs, b, what, *, op="avg", accumulate=True, sync=True):
    """reduce_scatter_sq on clones of xs[:n] into gs. With sync: cl.check(), then the sentinels
    behind and the elements past the valid length of every gshard and the gradients' bits."""
    grads = [x[:n].clone() for x in xs]
    sqs = cl.reduce_scatter_sq(grads, gs, op=op, accumulate=accumulate)
    if sync:
        cl.check()
        C._check_gshards(bufs, n, b, what)
        for r in range(cl.world):
            assert torch.equal(A._bits(grads[r]), A._bits(xs[r][:n])), f"{what} rank {r}: the gradient was written"
    return sqs, grads


# ------------------------------------------------------------------------------------------
# Item 1
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_exact_chain_of_two_micro_batches(P, dtype):
    cl = A._cluster(P)
    _, (xs1, xs2), want = _batches(P, dtype)
    want = want.to(DEV)
    st = cl.comms[0].stats
    before = (st.rs_sq, st.rs_sq_acc)
    sizes = A._sizes(P, dtype)
    for n in sizes:
        what = f"chain P={P} {dtype} n={n}"
        b, bufs, gs = C._gshards(cl, n, dtype)
        _launch(cl, xs1, n, bufs, gs, b, what + " plain", accumulate=False)
        _launch(cl, xs2, n, bufs, gs, b, what + " accumulating")
        got = C._full(gs, n, b)
        assert torch.equal(got, want[:n]), f"{what}: {A._first_diff(got, want[:n])}"
    assert (st.rs_sq - before[0], st.rs_sq_acc - before[1]) == (2 * len(sizes), len(sizes))


# ------------------------------------------------------------------------------------------
# Items 2, 3 (the bound) and 4
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_random_data_accumulates_as_torch_fp32_adds(P, dtype):
    cl = A._cluster(P)
    for n in A._sizes(P, dtype):
        what = f"random P={P} {dtype} n={n}"
        gen = torch.Generator(device=DEV).manual_seed(23 * n + P)
        xs = [torch.randn(n, device=DEV, generator=gen).to(dtype) for _ in range(P)]
        b, pbufs, plain = C._gshards(cl, n, dtype)
        _launch(cl, xs, n, pbufs, plain, b, what + " plain", accumulate=False)
        _, bufs, gs = C._gshards(cl, n, dtype)
        olds = []
        for r in range(P):  # random old values in the valid part; the sentinel stays past it
            v = C._valid(n, b, r)
            olds.append(torch.randn(v, device=DEV, generator=gen))
            gs[r][:v] = olds[r]
        sqs, _ = _launch(cl, xs, n, bufs, gs, b, what + " accumulating")
        bound = C._sq_bound(C._max_unit(cl.comms[0].knobs, n, P, dtype), dtype)
        for r in range(P):
            v = C._valid(n, b, r)
            want = olds[r] + plain[r][:v]
            assert torch.equal(gs[r][:v], want), f"{what} rank {r}: {A._first_diff(gs[r][:v], want)}"
            ref = float(gs[r][:v].double().pow(2).sum())  # of the resulting values, read back
            print(f"{what} rank {r}: sq {float(sqs[r])!r} ref {ref!r} bound {bound:.3e}")
            assert abs(float(sqs[r]) - ref) <= bound * ref, (what, r, float(sqs[r]), ref)
        # into zeros: the plain launch by value
        _, zbufs, zs = C._gshards(cl, n, dtype)
        for r in range(P):
            zs[r][:C._valid(n, b, r)] = 0
        zsq, _ = _launch(cl, xs, n, zbufs, zs, b, what + " into zeros")
        psq, _ = _launch(cl, xs, n, pbufs, plain, b, what + " plain again", accumulate=False)
        for r in range(P):
            v = C._valid(n, b, r)
            assert torch.equal(zs[r][:v], plain[r][:v]), f"{what} rank {r}: accumulating into zeros != plain"
            assert torch.equal(zsq[r], psq[r]), f"{what} rank {r}: sq of equal shards differs"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_three_accumulating_launches_chained_without_a_host_sync(P, dtype):
    cl = A._cluster(P)
    for n in (A._sizes(P, dtype)[0], 4099, NMAX):
        what = f"chained P={P} {dtype} n={n}"
        gen = torch.Generator(device=DEV).manual_seed(29 * n + P)
        xs = [torch.randn(n, device=DEV, generator=gen).to(dtype) for _ in range(P)]
        b, pbufs, plain = C._gshards(cl, n, dtype)
        _launch(cl, xs, n, pbufs, plain, b, what + " plain", accumulate=False)
        _, bufs, gs = C._gshards(cl, n, dtype)
        for r in range(P):
            gs[r][:C._valid(n, b, r)] = 0.25
        grads = [x.clone() for x in xs]
        for _ in range(3):
            cl.reduce_scatter_sq(grads, gs, op="avg", accumulate=True)
        cl.check()
        C._check_gshards(bufs, n, b, what)
        for r in range(P):
            v = C._valid(n, b, r)
            want = ((0.25 + plain[r][:v]) + plain[r][:v]) + plain[r][:v]
            assert torch.equal(gs[r][:v], want), f"{what} rank {r}: {A._first_diff(gs[r][:v], want)}"
            assert torch.equal(A._bits(grads[r]), A._bits(xs[r])), f"{what} rank {r}: the gradient was written"


# ------------------------------------------------------------------------------------------
# Item 3, exact
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_sum_of_squares_of_the_accumulated_shard_is_exact(P, dtype):
    """The power-of-two data of tests/test_clip_gpu.py split over two micro-batches by element
    parity: every element is non-zero on one rank and one micro-batch at most, so the accumulated
    shard holds value * scale or 0 and every partial sum of squares is exact in fp32."""
    cl = A._cluster(P)
    owner, vals, xs = C._pow2_data(P, dtype)
    even = (torch.arange(NMAX, device=DEV) % 2 == 0)
    halves = [[torch.where(even, x, torch.zeros((), dtype=dtype, device=DEV)) for x in xs],
              [torch.where(~even, x, torch.zeros((), dtype=dtype, device=DEV)) for x in xs]]
    for op in ("sum", "avg") if P in (2, 4, 8) else ("sum",):
        scale = 1.0 / P if op == "avg" else 1.0
        for n in A._sizes(P, dtype):
            what = f"sq P={P} {dtype} n={n} {op}"
            b, bufs, gs = C._gshards(cl, n, dtype)
            _launch(cl, halves[0], n, bufs, gs, b, what + " plain", op=op, accumulate=False)
            sqs, _ = _launch(cl, halves[1], n, bufs, gs, b, what + " accumulating", op=op)
            val64 = torch.where(owner[:n] >= 0, vals[:n].double() * scale, torch.zeros((), dtype=torch.float64))
            assert torch.equal(C._full(gs, n, b).cpu().double(), val64), what
            for r in range(P):
                ref = val64[r * b:min(n, (r + 1) * b)].pow(2).sum()
                assert torch.equal(sqs[r].cpu(), ref.float().reshape(1)), (what, r, float(sqs[r]), float(ref))


# ------------------------------------------------------------------------------------------
# Item 5: the communicator's wrapper
# ------------------------------------------------------------------------------------------
@gpu
def test_communicator_wrapper_with_grid_override():
    from akka_allreduce_1_amd.parallel import XgmiCommunicator

    dist = C._one_process_group()
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=A.SLOT, timeout_s=10.0)
        default = comm.native.grid
        assert default > 8
        runs = 0
        for grid in (8, 0):  # the override, then back to the default
            for dtype in DTYPES:
                _, (xs1, xs2), want = _batches(1, dtype)
                for n in (7, 4099, 65_539):
                    what = f"communicator grid={grid} {dtype} n={n}"
                    b = comm.shard_len(n, dtype)
                    buf = torch.full((b + A.GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
                    gs = buf[:b]
                    g1, g2 = xs1[0][:n].clone(), xs2[0][:n].clone()
                    comm.reduce_scatter_sq(g1, gs, op="avg", grid=grid)
                    sq = comm.reduce_scatter_sq(g2, gs, op="avg", grid=grid, accumulate=True)
                    comm.check()
                    runs += 1
                    assert comm.native.grid == (grid or default)
                    assert torch.equal(gs[:n], want[:n].to(DEV)), what
                    assert bool((buf[n:] == SENTINEL).all()), what
                    assert torch.equal(A._bits(g2), A._bits(xs2[0][:n])), what
                    ref = float(gs[:n].double().pow(2).sum())
                    assert abs(float(sq) - ref) <= C._sq_bound(n, dtype) * ref, what
        assert (comm.stats.rs_sq, comm.stats.rs_sq_acc, comm.stats.adamw_shard, comm.stats.adamw) == (2 * runs, runs, 0, 0)
        with pytest.raises(ValueError):
            comm.reduce_scatter_sq(g2, gs[:-4], accumulate=True)
        with pytest.raises(ValueError):
            comm.reduce_scatter_sq(g2, gs, op="max", accumulate=True)
        with pytest.raises(ValueError):
            comm.reduce_scatter_sq(g2, gs.double(), accumulate=True)
        assert comm.stats.rs_sq == 2 * runs
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------
# Item 6: ShardedDataParallel, world 1
# ------------------------------------------------------------------------------------------
FUSED = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)


def _inputs(dtype, k):
    gen = torch.Generator(device=DEV)
    return [torch.randn(32, 64, device=DEV, generator=gen.manual_seed(40 + i)).to(dtype) for i in range(k)]


def _counters(comm):
    st = comm.stats
    return (st.rs_sq, st.rs_sq_acc, st.adamw_shard, st.adamw)


def _delta(comm, before):
    return tuple(a - b for a, b in zip(_counters(comm), before))


def _unequal(ma, za, mb, zb, what):
    out = []
    for i, (p, p2) in enumerate(zip(ma.parameters(), mb.parameters())):
        if not torch.equal(A._bits(p.data), A._bits(p2.data)):
            out.append(f"{what} parameter {i}")
    for i, (sa, sb) in enumerate(zip(za.adamw_states, zb.adamw_states)):
        for key in ("master", "exp_avg", "exp_avg_sq"):
            if not torch.equal(A._bits(sa[key]), A._bits(sb[key])):
                out.append(f"{what} bucket {i} {key}")
    return out


@gpu
@pytest.mark.parametrize("max_grad_norm", [None, 1e9])
@pytest.mark.parametrize("overlap", [True, False])
def test_sharded_accumulation_equals_autograds_fp32_accumulation(overlap, max_grad_norm):
    """fp32 parameters: backward(x1); accumulate(); backward(x2); step() leaves the bits of the
    flag-less twin (overlap=False, so its hooks launch nothing) run as backward(x1); backward(x2);
    step(), where autograd's fp32 add into the flat gradient is the same add. Then a step of three
    micro-batches for the launch counts, a step without accumulate() against the twin, the
    refusals and the checkpoint keys. The bit comparisons are asserted last."""
    from akka_allreduce_1_amd.parallel import ShardedDataParallel, XgmiCommunicator

    dist = C._one_process_group()
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=A.SLOT, timeout_s=10.0)
        dtype = torch.float32
        ma, mb = C._net(dtype), C._net(dtype)
        za = ShardedDataParallel(ma, comm, None, bucket_bytes=16 << 10, fused_adamw=FUSED, max_grad_norm=max_grad_norm,
                                 overlap=overlap, grad_accumulation=True)
        zb = ShardedDataParallel(mb, comm, None, bucket_bytes=16 << 10, fused_adamw=FUSED, max_grad_norm=max_grad_norm,
                                 overlap=False)
        nb = len(za.buckets)
        assert nb > 1
        clipped = max_grad_norm is not None
        x1, x2, x3 = _inputs(dtype, 3)
        unequal = []

        def loss(m, x):
            return m(x).float().pow(2).mean()

        # two steps of two micro-batches
        for step in range(2):
            before = _counters(comm.native)
            za.zero_grad()
            loss(ma, x1 * (step + 1)).backward()
            za.accumulate()
            assert za.micro_batches == 1
            with pytest.raises(RuntimeError, match="accumulate"):
                za.state_dict()
            loss(ma, x2).backward()
            za.step()
            comm.check()
            assert za.micro_batches == 0
            assert _delta(comm.native, before) == (2 * nb, nb, nb, 0)
            zb.zero_grad()
            loss(mb, x1 * (step + 1)).backward()
            loss(mb, x2).backward()
            zb.step()
            comm.check()
            if clipped:
                assert float(za.last_clip_coef) == 1.0
                assert torch.equal(za.last_grad_norm, zb.last_grad_norm)
            unequal += _unequal(ma, za, mb, zb, f"two micro-batches, step {step}:")
        # k = 3 micro-batches: the launches of one step
        before = _counters(comm.native)
        bytes_before = za.stats["clip_bytes"]
        za.zero_grad()
        for i, x in enumerate((x1, x2, x3)):
            loss(ma, x).backward()
            if i < 2:
                za.accumulate()
        za.step()
        comm.check()
        assert _delta(comm.native, before) == (3 * nb, 2 * nb, nb, 0)
        owned = sum(g.numel() for g in za.gshards)
        assert za.stats["clip_bytes"] - bytes_before == (8 + 2 * 4) * owned
        assert za.stats["accumulates"] == 4 and za.stats["steps"] == 3
        zb.zero_grad()
        for x in (x1, x2, x3):
            loss(mb, x).backward()
        zb.step()
        comm.check()
        unequal += _unequal(ma, za, mb, zb, "three micro-batches:")
        # a step without accumulate(): today's launches, today's bits
        before = _counters(comm.native)
        za.zero_grad()
        loss(ma, x3).backward()
        za.step()
        comm.check()
        mine = _delta(comm.native, before)
        before = _counters(comm.native)
        zb.zero_grad()
        loss(mb, x3).backward()
        zb.step()
        comm.check()
        assert mine == _delta(comm.native, before) == ((nb, 0, nb, 0) if clipped else (0, 0, 0, nb))
        unequal += _unequal(ma, za, mb, zb, "no accumulate():")
        # refusals, checkpoints, describe()
        with pytest.raises(RuntimeError, match="grad_accumulation"):
            zb.accumulate()
        with pytest.raises(ValueError, match="grad_accumulation"):
            ShardedDataParallel(C._net(dtype), comm, None, fused_adamw=FUSED, step_in_backward=True,
                                grad_accumulation=True)
        assert set(za.state_dict()) == set(zb.state_dict())
        assert set(za.state_dict()["adamw"][0]) == {"master", "exp_avg", "exp_avg_sq"}
        assert all(d["accum_bytes"] == d["gshard_bytes"] == 4 * d["shard"] for d in za.describe())
        assert all("accum_bytes" not in d for d in zb.describe())
        assert not unequal, f"{len(unequal)} differences from autograd's accumulation, first: {unequal[:3]}"
    finally:
        dist.destroy_process_group()


@gpu
@pytest.mark.parametrize("max_grad_norm", [None, 1e9])
@pytest.mark.parametrize("overlap", [True, False])
def test_sharded_accumulation_sums_bf16_gradients_in_fp32(overlap, max_grad_norm):
    """bf16 parameters: the flat gradient of each micro-batch is cloned after its backward; after
    step() every bucket's gshard holds g1.float() + g2.float(), bit for bit (world 1: scale 1)."""
    from akka_allreduce_1_amd.parallel import ShardedDataParallel, XgmiCommunicator

    dist = C._one_process_group()
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=A.SLOT, timeout_s=10.0)
        dtype = torch.bfloat16
        m = C._net(dtype)
        zdp = ShardedDataParallel(m, comm, None, bucket_bytes=16 << 10, fused_adamw=FUSED, max_grad_norm=max_grad_norm,
                                  overlap=overlap, grad_accumulation=True)
        assert len(zdp.buckets) > 1
        x1, x2 = _inputs(dtype, 2)
        p0 = [p.detach().clone() for p in m.parameters()]
        zdp.zero_grad()
        m(x1).float().pow(2).mean().backward()
        g1 = [b.flat_grad.clone() for b in zdp.buckets]
        zdp.accumulate()
        assert all(not bool(b.flat_grad.any()) for b in zdp.buckets)  # accumulate() zeroed them
        m(x2).float().pow(2).mean().backward()
        g2 = [b.flat_grad.clone() for b in zdp.buckets]
        zdp.step()
        comm.check()
        for i, b in enumerate(zdp.buckets):
            want = g1[i].float() + g2[i].float()
            assert bool(want.any()) and not torch.equal(want, want.to(dtype).float())  # a real fp32 sum
            got = zdp.gshards[i][:b.numel]
            assert torch.equal(got, want), f"bucket {i}: {A._first_diff(got, want)}"
        assert any(not torch.equal(p, q) for p, q in zip(m.parameters(), p0))
    finally:
        dist.destroy_process_group()
