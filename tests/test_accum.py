"""Gradient accumulation in ShardedDataParallel, unfused path, on CPU with gloo (world 2, two
processes): three steps of two micro-batches (`accumulate()` after the first, `step()` after the
second) against a full-model reference that adds the rank-mean gradients of both micro-batches
into `p.grad`, applies torch.nn.utils.clip_grad_norm_ when clipping, then the optimizer; the flag
without an `accumulate()` call against a flag-less twin, bit for bit; the refusals. Model, bucket
size, optimizers and tolerances are those of tests/test_clip.py. The fused path's tests are
tests/test_accum_gpu.py."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from akka_allreduce_1_amd.parallel.ddp import TorchDistComm


def _model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 33), torch.nn.ReLU(), torch.nn.Linear(33, 5), torch.nn.ReLU(),
                               torch.nn.Linear(5, 3))


def _accum_worker(rank, world, port, q):
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import ShardedDataParallel

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # data[k][r]: micro-batch k of rank r
        data = [[torch.randn(4, 7, generator=torch.Generator().manual_seed(200 + 10 * k + r)) for r in range(world)]
                for k in range(2)]

        def accumulated_mean_grads(ref, step):
            """p.grad = sum over micro-batches of the mean over ranks."""
            total = [torch.zeros_like(p) for p in ref.parameters()]
            for k in range(2):
                for r in range(world):
                    ref.zero_grad()
                    ref(data[k][r] * (step + 1)).pow(2).sum().backward()
                    for t, p in zip(total, ref.parameters()):
                        t.add_(p.grad / world)
            for t, p in zip(total, ref.parameters()):
                p.grad = t

        # 1. three steps of two micro-batches against the full-model reference
        for max_norm in (None, 0.5):
            for opt_name in ("sgd", "adam"):
                make = (lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9)) if opt_name == "sgd" else (
                    lambda ps: torch.optim.Adam(ps, lr=0.01))
                m, ref = _model(0), _model(0)
                zdp = ShardedDataParallel(m, TorchDistComm(), make, bucket_bytes=300, max_grad_norm=max_norm,
                                          grad_accumulation=True)
                assert len(zdp.buckets) > 1
                assert all(d["accum_bytes"] == 4 * d["shard"] for d in zdp.describe())
                ref_opt = make(list(ref.parameters()))
                clipped = 0
                for step in range(3):
                    zdp.zero_grad()
                    m(data[0][rank] * (step + 1)).pow(2).sum().backward()
                    zdp.accumulate()
                    assert zdp.micro_batches == 1
                    with pytest.raises(RuntimeError, match="accumulate"):
                        zdp.state_dict()
                    m(data[1][rank] * (step + 1)).pow(2).sum().backward()
                    zdp.step()
                    assert zdp.micro_batches == 0
                    accumulated_mean_grads(ref, step)
                    if max_norm is not None:
                        norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
                        assert abs(float(zdp.last_grad_norm) - float(norm)) <= 1e-5 * float(norm), (opt_name, step)
                        want = min(1.0, max_norm / (float(norm) + 1e-6))
                        assert abs(float(zdp.last_clip_coef) - want) <= 1e-5, (opt_name, step)
                        clipped += float(zdp.last_clip_coef) < 1.0
                    ref_opt.step()
                    for p, rp in zip(m.parameters(), ref.parameters()):
                        assert torch.allclose(p, rp, atol=1e-5), (max_norm, opt_name, step)
                assert clipped == (3 if max_norm is not None else 0)  # the bound was low enough to clip every step
                assert zdp.stats["accumulates"] == 3 and zdp.stats["steps"] == 3
                zdp.state_dict()  # allowed again after step()
                zdp.remove_hooks()

        # 2. the flag without accumulate(): the same bits as without the flag
        make = lambda ps: torch.optim.Adam(ps, lr=0.01)  # noqa: E731
        for max_norm in (None, 0.5):
            ma, mb = _model(0), _model(0)
            za = ShardedDataParallel(ma, TorchDistComm(), make, bucket_bytes=300, max_grad_norm=max_norm,
                                     grad_accumulation=True)
            zb = ShardedDataParallel(mb, TorchDistComm(), make, bucket_bytes=300, max_grad_norm=max_norm)
            for step in range(3):
                for mm, zz in ((ma, za), (mb, zb)):
                    zz.zero_grad()
                    mm(data[0][rank] * (step + 1)).pow(2).sum().backward()
                    zz.step()
                for p, p2 in zip(ma.parameters(), mb.parameters()):
                    assert torch.equal(p, p2), (max_norm, step)
            assert set(za.state_dict()) == set(zb.state_dict())  # checkpoints unchanged
            assert all("accum_bytes" not in d for d in zb.describe()) and "accumulates" not in zb.stats
            with pytest.raises(RuntimeError, match="grad_accumulation"):
                zb.accumulate()
        q.put((rank, True, ""))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, False, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_unfused_accumulation_matches_the_full_model_reference_gloo():
    from akka_allreduce_1_amd.parallel.comm import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_accum_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=30)
    bad = [r for r in res if not r[1]]
    assert not bad, bad[0][2]


class _NoComm:
    world, rank = 1, 0


def test_refusals():
    from akka_allreduce_1_amd.parallel import ShardedDataParallel

    with pytest.raises(ValueError, match="grad_accumulation"):
        ShardedDataParallel(_model(0), _NoComm(), None, fused_adamw={"lr": 1e-3}, step_in_backward=True,
                            grad_accumulation=True)
    zdp = ShardedDataParallel(_model(0), _NoComm(), lambda ps: torch.optim.SGD(ps, lr=0.1))
    with pytest.raises(RuntimeError, match="grad_accumulation"):
        zdp.accumulate()
    assert zdp.micro_batches == 0
