"""ShardedDataParallel(fused_adamw=..., loss_scale=...) with XgmiCommunicator: 2 processes on one
MI355X (IPC-mapped slabs), the model and rank count of tests/test_clip_ddp_gpu.py.

  1. a static power-of-two scale and no overflow: three loss-scaled fused steps are bit-equal to
     the existing clipped fused steps, and to the existing accumulated ones, on unscaled losses.
     The parameters are fp32 and the scale is 1024: the scaled loss's backward multiplies the one
     upstream gradient by 2^10 and every product and sum after it scales exactly (nothing leaves
     the normal range), so autograd itself hands over exactly 1024 times the plain gradients;
  2. an overflow forced at call 2 (an inf injected into one rank's gradient): the parameters are
     identical on every rank and unchanged by the skipped call, the scale is halved, applied_steps
     is 2 after three calls, last_step_skipped and skipped_steps are right;
  3. a state_dict round trip on every rank: the resumed instance takes the next step to the same bits;
  4. the unfused path on the same communicator ends the same script with the same scale, tracker
     and counters."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _model(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.GELU(), torch.nn.Linear(256, 128), torch.nn.GELU(),
                            torch.nn.Linear(128, 8))
    return m.to(device="cuda:0", dtype=torch.float32)


def _bits(m):
    return torch.cat([p.data.reshape(-1) for p in m.parameters()]).view(torch.int32)


def _worker(rank, world, port, q):
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import ShardedDataParallel, XgmiCommunicator

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=15.0)
        hp = {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01}
        kw = dict(bucket_bytes=32 << 10, fused_adamw=hp)
        g = torch.Generator(device="cuda:0")
        data = [torch.randn(16, 64, device="cuda:0", generator=g.manual_seed(30 + rank + 10 * k)) for k in range(4)]

        def same_on_every_rank(t, what):
            both = [torch.empty_like(t).cpu() for _ in range(world)]
            dist.all_gather(both, t.cpu())
            assert all(torch.equal(b, both[0]) for b in both), what

        def backward(m, z, x, poison=None):
            loss = m(x).pow(2).mean()
            loss = z.scale_loss(loss) if hasattr(z, "loss_scale") else loss
            hook = None
            if poison is not None:
                def put(gr, bad=poison):
                    gr = gr.clone()
                    gr.view(-1)[3] = bad
                    return gr
                hook = next(m.parameters()).register_hook(put)
            loss.backward()
            if hook is not None:
                hook.remove()

        # 1. clipped, both overlap settings, then accumulated (two micro-batches): scaled == plain
        ref = _model(0)  # the same bound on every rank: from one fixed batch
        ref(torch.randn(16, 64, device="cuda:0", generator=g.manual_seed(30))).pow(2).mean().backward()
        max_norm = 0.05 * float(torch.nn.utils.clip_grad_norm_(ref.parameters(), float("inf")))
        for variant in ({"max_grad_norm": max_norm, "overlap": True}, {"max_grad_norm": max_norm, "overlap": False},
                        {"grad_accumulation": True}, {"grad_accumulation": True, "max_grad_norm": max_norm}):
            ms, mp_ = _model(0), _model(0)
            zs = ShardedDataParallel(ms, comm, None, loss_scale=1024.0, **variant, **kw)
            zp = ShardedDataParallel(mp_, comm, None, **variant, **kw)
            assert len(zs.buckets) > 1
            shard, plain = comm.native.stats.adamw_shard, comm.native.stats.adamw
            for step in range(3):
                for m, z in ((ms, zs), (mp_, zp)):
                    z.zero_grad()
                    if variant.get("grad_accumulation"):
                        backward(m, z, data[step])
                        z.accumulate()
                        backward(m, z, data[step + 1])
                    else:
                        backward(m, z, data[step])
                    z.step()
                comm.check()
                assert torch.equal(_bits(ms), _bits(mp_)), (variant, step)
                assert int(zs.last_step_skipped) == 0 and int(zs.applied_steps) == step + 1
                if "max_grad_norm" in variant:  # the norm of the unscaled gradient, and it clipped
                    assert torch.equal(zs.last_grad_norm.reshape(1), zp.last_grad_norm.reshape(1)), (variant, step)
                    assert torch.equal(zs.last_clip_coef.reshape(1), zp.last_clip_coef.reshape(1)), (variant, step)
                    assert 0 < float(zs.last_clip_coef) < 1
            for a, b in zip(zs.adamw_states, zp.adamw_states):
                for key in ("master", "exp_avg", "exp_avg_sq"):
                    assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), (variant, key)
            assert float(zs.loss_scale) == 1024.0 and int(zs.skipped_steps) == 0
            # loss_scale forces the split step: every update half of both runs was a shard launch
            assert comm.native.stats.adamw == plain and comm.native.stats.adamw_shard - shard == 6 * len(zs.buckets)
            zs.remove_hooks()
            zp.remove_hooks()

        # 2. dynamic scale, an inf in rank 1's gradient at call 2
        spec = {"init_scale": 1024.0, "growth_interval": 100}
        m = _model(0)
        z = ShardedDataParallel(m, comm, None, loss_scale=spec, max_grad_norm=max_norm, **kw)
        seen = []
        for call in (1, 2, 3):
            before = _bits(m).clone()
            states = [{k: v.clone() for k, v in st.items()} for st in z.adamw_states]
            z.zero_grad()
            backward(m, z, data[call], poison=float("inf") if call == 2 and rank == 1 else None)
            z.step()
            comm.check()
            same_on_every_rank(_bits(m), f"call {call}: parameters differ between ranks")
            skipped = call == 2
            assert int(z.last_step_skipped) == int(skipped), call
            assert torch.equal(before, _bits(m)) == skipped, call
            if skipped:
                assert float(z.last_grad_norm) == float("inf")
                for st, old in zip(z.adamw_states, states):
                    assert all(torch.equal(st[k].view(torch.int32), old[k].view(torch.int32)) for k in old), call
            seen.append((float(z.loss_scale), int(z.applied_steps), int(z.skipped_steps)))
        assert seen == [(1024.0, 1, 0), (512.0, 1, 1), (512.0, 2, 1)], seen
        assert z.stats["steps"] == 3 and bool(_bits(m).view(torch.float32).isfinite().all())

        # 3. checkpoint round trip: the resumed instance takes call 4 to the same bits
        sd = z.state_dict()
        assert sd["step"] == 2 and sd["steps"] == 3
        assert sd["loss_scale"] == {"scale": 512.0, "growth_tracker": 1, "skipped": 1}
        sd = {k: ([{n: t.clone() for n, t in st.items()} for st in v] if k == "adamw" else v) for k, v in sd.items()}
        m2 = _model(1)
        z2 = ShardedDataParallel(m2, comm, None, loss_scale=spec, max_grad_norm=max_norm, **kw)
        for p, p2 in zip(m.parameters(), m2.parameters()):
            p2.data.copy_(p.data)
        z2.load_state_dict(sd)
        for mm, zz in ((m, z), (m2, z2)):
            zz.zero_grad()
            backward(mm, zz, data[0])
            zz.step()
        comm.check()
        assert torch.equal(_bits(m), _bits(m2))
        assert z2.state_dict()["loss_scale"] == z.state_dict()["loss_scale"] and z2.state_dict()["step"] == 3
        same_on_every_rank(_bits(m2), "resumed parameters differ between ranks")

        # 4. the unfused path, same script: same scale, tracker and counters
        mu = _model(0)
        zu = ShardedDataParallel(mu, comm, lambda ps: torch.optim.AdamW(ps, **hp), bucket_bytes=32 << 10,
                                 loss_scale=spec, max_grad_norm=max_norm)
        for call in (1, 2, 3):
            zu.zero_grad()
            backward(mu, zu, data[call], poison=float("inf") if call == 2 and rank == 1 else None)
            zu.step()
            assert int(zu.last_step_skipped) == int(call == 2)
        comm.check()
        fused_sd, unfused_sd = sd, zu.state_dict()
        assert unfused_sd["loss_scale"] == fused_sd["loss_scale"] and unfused_sd["step"] == fused_sd["step"] == 2
        assert (float(zu.loss_scale), int(zu.applied_steps), int(zu.skipped_steps)) == seen[-1]
        q.put((rank, True, ""))
    except Exception:  # noqa: BLE001
        import traceback

        q.put((rank, False, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_loss_scaled_fused_step_two_processes():
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad[0][2]
