"""The schedule of tests/test_zero_schedule.py with its streams: 2 processes on one MI355X around a
real XgmiCommunicator, one step in each mode, every communicator call recorded together with
whether the current stream was the side stream (`zdp.stream`) when it was made."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from test_clip_ddp_gpu import _model

pytestmark = pytest.mark.gpu

STEP_METHODS = ("step_adamw", "reduce_scatter_sq", "clip_coef", "step_adamw_shard", "reduce_scatter", "all_gather")


class _StreamProxy:
    """Forwards everything to the communicator; calls of the step surface made while `zdp` is set
    are recorded as (method, current stream is zdp.stream)."""

    def __init__(self, comm):
        self._comm, self.zdp, self.log = comm, None, []

    def __getattr__(self, name):
        attr = getattr(self._comm, name)
        if name not in STEP_METHODS:
            return attr

        def call(*args, **kw):
            if self.zdp is not None:
                self.log.append((name, torch.cuda.current_stream() == self.zdp.stream))
            return attr(*args, **kw)
        return call


def _stream_worker(rank, world, port, q):
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import ShardedDataParallel, XgmiCommunicator

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        comm = _StreamProxy(XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=15.0))
        hp = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01}
        x = torch.randn(16, 64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(30 + rank))

        def one_step(fused, **kw):
            m = _model(0, torch.float32)
            make = None if fused else (lambda ps: torch.optim.AdamW(ps, lr=1e-3))
            zdp = ShardedDataParallel(m, comm, make, bucket_bytes=32 << 10, fused_adamw=hp if fused else None, **kw)
            n = len(zdp.buckets)
            assert n > 1
            comm.zdp, comm.log = zdp, []
            m(x).pow(2).mean().backward()
            zdp.step()
            comm.check()
            comm.zdp = None
            zdp.remove_hooks()
            assert all(torch.isfinite(p).all() for p in m.parameters())
            return n, comm.log

        for overlap in (True, False):  # reduce halves on the side stream exactly when overlap; the rest on the current
            n, log = one_step(True, max_grad_norm=1.0, overlap=overlap)
            assert log == ([("reduce_scatter_sq", overlap)] * n + [("clip_coef", False)]
                           + [("step_adamw_shard", False)] * n)
        n, log = one_step(True, step_in_backward=True)
        assert log == [("step_adamw", True)] * n
        n, log = one_step(True)
        assert log == [("step_adamw", False)] * n
        n, log = one_step(False)
        assert log == [("reduce_scatter", True)] * n + [("all_gather", False)] * n
        q.put((rank, True, ""))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, False, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_streams_of_every_step_kind_two_processes():
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_stream_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad[0][2]
