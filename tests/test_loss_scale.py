"""Loss scaling in ShardedDataParallel on the CPU: the rule (parallel/loss_scale.py) against a
plain-Python model, and the unfused path - worlds 1 and 2, fp32 and bf16 parameters, static and
dynamic scales, with clipping and with accumulation, checkpoints, refusals.

The ranks of a world are threads of this process over `_World`, a CPU communicator of a dozen
lines (reduce-scatter: fp32 sum in rank order, times 1 / world, rounded once; all-gather: a copy):
gloo promises no bf16 reduce-scatter, a thread costs nothing to start, and every collective here
is deterministic. The gradients are written straight into the flat gradient buffers (`p.grad` is
a view of them), so that a scaled run gets exactly `scale * g` and the plain run it is compared
with exactly `g`: with a power-of-two scale everything after the reduce-scatter is then the same
fp32 arithmetic, and the comparisons hold no tolerance.

The fused path's tests are tests/test_loss_scale_gpu.py and tests/test_loss_scale_ddp_gpu.py."""
import copy
import struct
import threading

import pytest
import torch

from akka_allreduce_1_amd.parallel import ShardedDataParallel
from akka_allreduce_1_amd.parallel import loss_scale as LS

INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------
# 1. The rule against a plain-Python model
# ------------------------------------------------------------------------------------------
def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


class _Model:
    """GradScaler's rule, in Python floats rounded to fp32 after every product (the double
    product of an fp32 value and a short factor is exact, so one rounding gives the fp32 one)."""

    def __init__(self, cfg):
        self.cfg, self.scale, self.tracker, self.applied, self.skipped = cfg, _f32(cfg.init_scale), 0, 0, 0

    def step(self, found):
        c = self.cfg
        if found:
            self.skipped += 1
            if c.dynamic:
                self.scale, self.tracker = _f32(self.scale * _f32(c.backoff_factor)), 0
        else:
            self.applied += 1
            if c.dynamic:
                self.tracker += 1
                if self.tracker == c.growth_interval:
                    self.scale, self.tracker = _f32(self.scale * _f32(c.growth_factor)), 0

    def words(self):
        return [self.scale, self.tracker, self.applied, self.skipped]


def _words(state):
    return [float(LS.scale_of(state))] + state[1:].tolist()


def _recs(*sqs):
    recs = torch.zeros(len(sqs), 2, dtype=torch.float64)
    recs[:, 0] = torch.tensor(sqs, dtype=torch.float64)
    return recs


SCRIPT = [0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]


@pytest.mark.parametrize("spec", [
    {"init_scale": 1024.0, "growth_interval": 3},
    {"init_scale": 1024.0, "growth_interval": 3, "growth_factor": 1.5},
    {"init_scale": 3.0, "growth_interval": 2, "growth_factor": 1.5, "backoff_factor": 0.75},
    {"growth_interval": 1},
    True,
    1.0,
    4096.0,
])
def test_rule_follows_the_plain_python_model(spec):
    """Growth after exactly growth_interval clean steps, backoff and tracker reset on a found
    step, a static scale that never moves, a growth factor that is no power of two, the counters."""
    cfg = LS.LossScaleConfig(spec)
    state, model = LS.new_state(cfg, "cpu"), _Model(cfg)
    assert _words(state) == model.words()
    for i, found in enumerate(SCRIPT):
        bad = (INF, NAN)[i % 2]
        before = model.scale
        norm, clip, coef, f = LS.scale_step_rule(_recs(9.0, bad if found else 16.0), state, cfg, None)
        model.step(found)
        assert _words(state) == model.words(), (i, _words(state), model.words())
        assert bool(f) == bool(found) and f.dtype == torch.bool
        assert norm.dtype == clip.dtype == coef.dtype == torch.float32 and norm.dim() == coef.dim() == 0
        assert float(clip) == 1.0 and float(coef) == _f32(1.0 / before)  # the scale BEFORE the step unscales it
        if not found:
            assert float(norm) == _f32(5.0 * _f32(1.0 / before))
        else:
            assert float(norm) == INF if bad == INF else bool(norm.isnan())
    if not cfg.dynamic:
        assert model.scale == cfg.init_scale and model.tracker == 0
    assert model.applied + model.skipped == len(SCRIPT) and model.skipped == sum(SCRIPT)


def test_rule_with_a_power_of_two_scale_gives_the_unscaled_bits():
    """norm, clip and coef * S at S = 2^k are clip_coef_from_records' bits at S = 1: the ground
    every bit-for-bit comparison of a loss-scaled run with a plain one stands on."""
    from akka_allreduce_1_amd.parallel.comm import clip_coef_from_records

    gen = torch.Generator().manual_seed(5)
    for _ in range(50):
        sq = torch.rand(3, generator=gen, dtype=torch.float64) * 10.0
        for max_norm in (0.7, 1.0, 3.0, 1e9):
            norm1, coef1 = clip_coef_from_records(_recs(*sq.tolist()), max_norm)
            for S in (1.0, 2.0, 65536.0, 2.0 ** -3):
                cfg = LS.LossScaleConfig(S)
                norm, clip, coef, found = LS.scale_step_rule(_recs(*(sq * S * S).tolist()), LS.new_state(cfg, "cpu"),
                                                             cfg, max_norm)
                assert not bool(found)
                assert torch.equal(norm, norm1) and torch.equal(clip, coef1) and float(coef) * S == float(coef1)


def test_spec_parsing():
    d = LS.LossScaleConfig(True)
    assert d.dynamic and (d.init_scale, d.growth_factor, d.backoff_factor, d.growth_interval) == (65536.0, 2.0, 0.5, 2000)
    assert LS.LossScaleConfig({}).dynamic and not LS.LossScaleConfig(1.0).dynamic and not LS.LossScaleConfig(128).dynamic
    assert LS.LossScaleConfig({"init_scale": 8.0}).init_scale == 8.0
    for bad in (False, 0.0, -2.0, INF, {"scale": 2.0}, {"growth_factor": 1.0}, {"backoff_factor": 1.0},
                {"growth_interval": 0}, 0.1):
        with pytest.raises(ValueError):
            LS.LossScaleConfig(bad)
    with pytest.raises(TypeError):
        LS.LossScaleConfig("dynamic")


# ------------------------------------------------------------------------------------------
# The CPU communicator and the scripted runs
# ------------------------------------------------------------------------------------------
class _World:
    def __init__(self, world):
        self.world, self.slots, self.barrier = world, [None] * world, threading.Barrier(world)

    def exchange(self, rank, t):
        self.slots[rank] = t
        self.barrier.wait()
        got = list(self.slots)
        self.barrier.wait()
        return got


class _Comm:
    def __init__(self, shared, rank):
        self.shared, self.world, self.rank = shared, shared.world, rank

    def reduce_scatter(self, inp, out, *, op="sum"):
        n = out.numel()
        acc = torch.zeros(n, dtype=torch.float32)
        for t in self.shared.exchange(self.rank, inp.clone()):  # a fast rank refills its buffer at once
            acc += t[self.rank * n:(self.rank + 1) * n].float()
        out.copy_(acc * (1.0 / self.world) if op == "avg" else acc)
        return out

    def all_gather(self, inp, out):
        out.copy_(torch.cat(self.shared.exchange(self.rank, inp.clone())))
        return out


def _on_ranks(world, fn):
    """fn(comm) on every rank of a fresh world, in threads; returns the ranks' results."""
    shared, res = _World(world), [None] * world

    def run(r):
        try:
            res[r] = (True, fn(_Comm(shared, r)))
        except BaseException as e:  # noqa: BLE001
            shared.barrier.abort()
            res[r] = (False, e)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    real = [r[1] for r in res if not r[0] and not isinstance(r[1], threading.BrokenBarrierError)]
    if real:
        raise real[0]
    assert all(r is not None and r[0] for r in res), res
    return [r[1] for r in res]


_SEED_LOCK = threading.Lock()


def _net(dtype):
    with _SEED_LOCK:  # the global generator is shared by the rank threads
        torch.manual_seed(0)
        return torch.nn.Sequential(torch.nn.Linear(7, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5)).to(dtype)


def _make(ps):
    return torch.optim.AdamW(ps, lr=0.01, betas=(0.9, 0.99), weight_decay=0.01)


CALLS, BAD_CALLS, MICRO = 6, (2, 5), 2


def _base_grads(zdp, rank, call, micro):
    """The unscaled gradient of (rank, call, micro-batch): one tensor per bucket, values on a
    coarse grid (multiples of 2^-6 below 4: exact in bf16, and so is any power-of-two multiple)."""
    out = []
    for b in zdp.buckets:
        gen = torch.Generator().manual_seed(1000 * call + 100 * micro + 10 * rank + b.index)
        out.append((torch.randint(-255, 256, (b.numel,), generator=gen).float() / 64.0).to(b.dtype))
    return out


def _run(comm, dtype, *, loss_scale, bad=None, max_norm=None, accumulate=False, calls=range(1, CALLS + 1),
         resume=None, check_skips=True):
    """A scripted run on one rank. Call c (counted from 1) of BAD_CALLS carries `bad` in one
    element of the last rank's gradient (the first micro-batch when accumulating); with
    loss_scale=None those calls are left out altogether: the plain run of the finite steps.
    Returns what the comparisons need."""
    m = _net(dtype)
    zdp = ShardedDataParallel(m, comm, _make, bucket_bytes=300, max_grad_norm=max_norm, grad_accumulation=accumulate,
                              loss_scale=loss_scale)
    assert len(zdp.buckets) > 1
    if resume is not None:
        for p, saved in zip(m.parameters(), resume["params"]):
            p.data.copy_(saved)
        zdp.load_state_dict(resume["sd"])
    norms, scales, snap = [], [], None
    for c in calls:
        poisoned = bad is not None and c in BAD_CALLS
        if poisoned and loss_scale is None:
            continue
        S = float(zdp.loss_scale) if loss_scale is not None else 1.0
        scales.append(S)
        before = _snapshot(m, zdp) if poisoned and check_skips else None
        micros = range(MICRO) if accumulate else range(1)
        for k in micros:
            for b, g in zip(zdp.buckets, _base_grads(zdp, comm.rank, c, k)):
                b.flat_grad.copy_(g * S)
                assert torch.equal(b.flat_grad.double(), g.double() * S)  # scaling the gradient was exact
                if poisoned and k == 0 and comm.rank == comm.world - 1 and b.index == 1:
                    b.flat_grad[3] = bad
            if k != micros[-1]:
                zdp.accumulate()
        zdp.step()
        if loss_scale is not None:
            assert int(zdp.last_step_skipped) == int(poisoned), c
            assert zdp.last_step_skipped.dim() == 0 and not zdp.last_step_skipped.dtype.is_floating_point
            if poisoned:
                n = zdp.last_grad_norm
                assert float(n) == INF if bad == INF else bool(n.isnan()), (c, float(n))
                if check_skips:  # parameters and optimizer state bit-equal to before the skipped call
                    _assert_same(before, _snapshot(m, zdp), f"skipped call {c}")
        if not poisoned:
            norms.append(zdp.last_grad_norm.clone())
        if c == 3:
            snap = {"sd": copy.deepcopy(zdp.state_dict()), "params": [p.data.clone() for p in m.parameters()]}
    out = {"final": _snapshot(m, zdp), "norms": norms, "scales": scales, "snap": snap, "steps": zdp.stats["steps"]}
    if loss_scale is not None:
        out.update(scale=float(zdp.loss_scale), applied=int(zdp.applied_steps), skipped=int(zdp.skipped_steps),
                   sd=zdp.state_dict())
        assert zdp.loss_scale.dim() == 0 and zdp.loss_scale.dtype == torch.float32
    return out


def _snapshot(m, zdp):
    st = zdp.optimizer.state_dict()["state"]
    tensors = [p.data.clone() for p in m.parameters()]
    for k in sorted(st):
        tensors += [st[k][name].clone() for name in sorted(st[k])]
    return tensors


def _assert_same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x, y), f"{what}: tensor {i} differs"


def _modelled_scale(spec):
    model = _Model(LS.LossScaleConfig(spec))
    for c in range(1, CALLS + 1):
        model.step(c in BAD_CALLS)
    return model


# ------------------------------------------------------------------------------------------
# 2. and 3. Skipped steps change nothing; the run equals the plain run of the finite steps
# ------------------------------------------------------------------------------------------
VARIANTS = [  # (loss_scale, bad, max_norm, accumulate)
    ({"init_scale": 65536.0, "growth_interval": 100}, INF, None, False),
    ({"init_scale": 65536.0, "growth_interval": 2}, INF, None, False),
    ({"init_scale": 1024.0, "growth_interval": 100}, NAN, None, False),
    (256.0, INF, None, False),
    (1.0, NAN, None, False),
    ({"init_scale": 4096.0, "growth_interval": 2}, INF, 2.0, False),
    ({"init_scale": 4096.0, "growth_interval": 100}, INF, None, True),
    ({"init_scale": 4096.0, "growth_interval": 2}, NAN, 2.0, True),
    (64.0, INF, 2.0, True),
]


@pytest.mark.parametrize("spec,bad,max_norm,accumulate", VARIANTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("world", [1, 2])
def test_scaled_run_equals_the_plain_run_of_the_finite_steps(world, dtype, spec, bad, max_norm, accumulate):
    kw = dict(max_norm=max_norm, accumulate=accumulate)
    scaled = _on_ranks(world, lambda comm: _run(comm, dtype, loss_scale=spec, bad=bad, **kw))
    plain = _on_ranks(world, lambda comm: _run(comm, dtype, loss_scale=None, bad=bad, **kw))
    model = _modelled_scale(spec)
    want_scale = model.scale
    if isinstance(spec, dict) and spec["growth_interval"] > CALLS:
        assert want_scale == spec["init_scale"] * 0.5 * 0.5
    for r in range(world):
        s, p = scaled[r], plain[r]
        _assert_same(s["final"], p["final"], f"rank {r}: after {CALLS} calls against the plain run of 4")
        assert (s["scale"], s["applied"], s["skipped"], s["steps"]) == (want_scale, 4, 2, CALLS), r
        assert p["steps"] == 4
        # last_grad_norm is the norm of the UNSCALED gradient: the plain run's, bit for bit
        assert len(s["norms"]) == len(p["norms"]) == 4
        if max_norm is not None:
            for a, b in zip(s["norms"], p["norms"]):
                assert torch.equal(a, b) and float(a) > max_norm, (r, float(a), float(b))  # and it clipped
        assert s["sd"]["step"] == 4 and s["sd"]["steps"] == CALLS
        assert s["sd"]["loss_scale"] == {"scale": want_scale, "growth_tracker": model.tracker, "skipped": 2}
        assert "loss_scale" not in p["snap"]["sd"]
    assert all(torch.equal(a, b) for a, b in zip(scaled[0]["final"][:4], scaled[-1]["final"][:4]))  # ranks agree


# ------------------------------------------------------------------------------------------
# 4. Checkpoints
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2])
def test_checkpoint_round_trip_mid_sequence(world):
    spec = {"init_scale": 4096.0, "growth_interval": 2}
    kw = dict(loss_scale=spec, bad=INF, max_norm=2.0)
    whole = _on_ranks(world, lambda comm: _run(comm, torch.bfloat16, **kw))
    resumed = _on_ranks(world, lambda comm: _run(comm, torch.bfloat16, calls=range(4, CALLS + 1),
                                                 resume=whole[comm.rank]["snap"], **kw))
    for r in range(world):
        sd = whole[r]["snap"]["sd"]
        assert sd["step"] == 2 and sd["steps"] == 3 and sd["loss_scale"]["skipped"] == 1
        assert all(not isinstance(v, torch.Tensor) for v in sd["loss_scale"].values())
        _assert_same(resumed[r]["final"], whole[r]["final"], f"rank {r}: resumed at call 4")
        for key in ("scale", "applied", "skipped", "steps"):
            assert resumed[r][key] == whole[r][key], (r, key)
        assert resumed[r]["sd"]["loss_scale"] == whole[r]["sd"]["loss_scale"]


def test_checkpoint_without_the_key_loads_and_a_plain_one_still_does():
    def both(comm):
        plain = _run(comm, torch.float32, loss_scale=None, calls=range(1, 4))
        snap = plain["snap"]
        assert "loss_scale" not in snap["sd"]
        m = _net(torch.float32)
        z = ShardedDataParallel(m, comm, _make, bucket_bytes=300, loss_scale={"init_scale": 512.0})
        z.load_state_dict(snap["sd"])
        assert float(z.loss_scale) == 512.0 and int(z.applied_steps) == 3 and int(z.skipped_steps) == 0
        assert z.state_dict()["loss_scale"] == {"scale": 512.0, "growth_tracker": 0, "skipped": 0}
        # and the other way: a loss-scaled checkpoint into a plain instance, exactly as today
        z2 = ShardedDataParallel(_net(torch.float32), comm, _make, bucket_bytes=300)
        z2.load_state_dict(z.state_dict())
        assert "loss_scale" not in z2.state_dict() and z2.stats["steps"] == 3
        again = _run(comm, torch.float32, loss_scale=None, calls=range(4, 5), resume=snap)
        return again["steps"]

    assert _on_ranks(1, both) == [4]


# ------------------------------------------------------------------------------------------
# 5. Errors, and the small interface
# ------------------------------------------------------------------------------------------
class _NoComm:
    world, rank = 1, 0


def test_refusals_and_scale_loss():
    with pytest.raises(ValueError, match="loss_scale"):
        ShardedDataParallel(_net(torch.float32), _NoComm(), None, fused_adamw={"lr": 1e-3}, step_in_backward=True,
                            loss_scale=1.0)
    with pytest.raises(ValueError, match="step_adamw"):  # the fused path needs the record-driven update half
        ShardedDataParallel(_net(torch.float32), _NoComm(), None, fused_adamw={"lr": 1e-3}, loss_scale=True)
    plain = ShardedDataParallel(_net(torch.float32), _NoComm(), _make)
    with pytest.raises(RuntimeError, match="loss_scale"):
        plain.scale_loss(torch.ones(()))
    z = ShardedDataParallel(_net(torch.float32), _NoComm(), _make, loss_scale=True)
    assert float(z.loss_scale) == 65536.0 and int(z.applied_steps) == int(z.skipped_steps) == 0
    loss = torch.tensor(0.25, requires_grad=True)
    scaled = z.scale_loss(loss)
    assert float(scaled.detach()) == 16384.0
    scaled.backward()
    assert float(loss.grad) == 65536.0
