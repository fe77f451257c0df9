"""ShardedDataParallel(fused_adamw=..., max_grad_norm=..., grad_accumulation=True) with
XgmiCommunicator: 2 processes on one MI355X (IPC-mapped slabs), three clipped steps of two
micro-batches each against a full-model reference that adds the rank-mean gradients of both
micro-batches into `p.grad`, applies torch.nn.utils.clip_grad_norm_ and then torch.optim.AdamW.
Model, slots, grid, timeout and tolerances are those of tests/test_clip_ddp_gpu.py."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _model(seed, dtype):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.GELU(), torch.nn.Linear(256, 128), torch.nn.GELU(),
                            torch.nn.Linear(128, 8))
    return m.to(device="cuda:0", dtype=dtype)


def _accum_worker(rank, world, port, q, overlap):
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import ShardedDataParallel, XgmiCommunicator

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=15.0)
        hp = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01}
        m, ref = _model(0, torch.float32), _model(0, torch.float32)
        g = torch.Generator(device="cuda:0")
        # data[k][r]: micro-batch k of rank r
        data = [[torch.randn(16, 64, device="cuda:0", generator=g.manual_seed(30 + 10 * k + r)) for r in range(world)]
                for k in range(2)]

        def accumulated_mean_grads():
            """p.grad = sum over micro-batches of the mean over ranks."""
            total = [torch.zeros_like(p) for p in ref.parameters()]
            for k in range(2):
                for r in range(world):
                    ref.zero_grad()
                    ref(data[k][r]).pow(2).mean().backward()
                    for t, p in zip(total, ref.parameters()):
                        t.add_(p.grad / world)
            for t, p in zip(total, ref.parameters()):
                p.grad = t

        accumulated_mean_grads()
        norm0 = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), float("inf")))
        max_norm = 0.02 * norm0  # low enough to clip every one of the three steps
        zdp = ShardedDataParallel(m, comm, None, bucket_bytes=32 << 10, fused_adamw=hp, max_grad_norm=max_norm,
                                  overlap=overlap, grad_accumulation=True)
        nb = len(zdp.buckets)
        assert nb > 1
        ref_opt = torch.optim.AdamW(list(ref.parameters()), lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                                    weight_decay=hp["weight_decay"])
        for step in range(3):
            zdp.zero_grad()
            m(data[0][rank]).pow(2).mean().backward()
            zdp.accumulate()
            m(data[1][rank]).pow(2).mean().backward()
            zdp.step()
            comm.check()
            accumulated_mean_grads()
            norm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
            ref_opt.step()
            assert abs(float(zdp.last_grad_norm) - norm) <= 1e-5 * norm, (step, float(zdp.last_grad_norm), norm)
            assert 0 < float(zdp.last_clip_coef) < 1, step
            assert abs(float(zdp.last_clip_coef) - max_norm / (norm + 1e-6)) <= 1e-5, step
            for p, rp in zip(m.parameters(), ref.parameters()):
                err = (p - rp).abs().max().item()
                assert err <= 1e-5, (step, err)
            # identical on both ranks: rank 0's parameters and coefficient, bit for bit
            flat = torch.cat([p.data.reshape(-1) for p in m.parameters()] + [zdp.last_clip_coef.reshape(1)])
            both = [torch.empty_like(flat).cpu() for _ in range(world)]
            dist.all_gather(both, flat.cpu())
            assert torch.equal(both[0].view(torch.int32), both[1].view(torch.int32)), step
        st = comm.native.stats
        assert (st.rs_sq, st.rs_sq_acc, st.adamw_shard, st.adamw) == (6 * nb, 3 * nb, 3 * nb, 0)
        q.put((rank, True, ""))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, False, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [True, False])
def test_accumulated_clipped_fused_step_two_processes(overlap):
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_accum_worker, args=(r, 2, port, q, overlap)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad[0][2]
