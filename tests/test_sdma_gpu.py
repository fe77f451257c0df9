"""SDMA bucket allreduce (csrc/hip/sdma_comm.h): cross-rank copies on the copy engines, a
small-grid reduce and gather on the CUs. Compared with an fp32 torch reference summed in
rank order (one rounding)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from akka_allreduce_1_amd.ops import fill_uniform  # noqa: E402

DEV = torch.device("cuda", 0)


def _ref(xs):
    acc = torch.zeros(xs[0].numel(), device=xs[0].device)
    for x in xs:
        acc += x.float()
    return acc


def _tol(dtype, P):
    return 1e-6 * P if dtype == torch.float32 else 1e-2 * P


@pytest.mark.parametrize("P", [2, 3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [7, 4096 + 5, 1 << 20, 3_000_017])
def test_local_sdma_allreduce(P, dtype, n):
    from akka_allreduce_1_amd.parallel import LocalSdmaCluster

    cl = LocalSdmaCluster(P, slot_bytes=2 << 20, grid=8)
    for it in range(3):  # both slot parities, then reuse
        xs = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=50 * it + k) for k in range(P)]
        ys = cl.allreduce(xs)
        torch.cuda.synchronize()
        cl.check()
        ref = _ref(xs)
        for k, y in enumerate(ys):
            err = (y.float() - ref).abs().max().item()
            assert err <= _tol(dtype, P), (it, k, err)


def test_local_sdma_inplace_mean_and_many_calls():
    from akka_allreduce_1_amd.parallel import LocalSdmaCluster

    P = 2
    cl = LocalSdmaCluster(P, slot_bytes=1 << 20, grid=4)
    for it in range(40):  # more calls than the signal ring holds
        n = [1000, 300_001, 65_536][it % 3]
        xs = [fill_uniform(torch.empty(n, device=DEV), seed=it * 7 + k) for k in range(P)]
        ref = _ref(xs) / P
        cl.allreduce(xs, xs, op="avg")
        for y in xs:
            torch.testing.assert_close(y, ref, rtol=0, atol=1e-6)
    cl.check()
    assert cl.comms[0].stats["calls"] >= 40


@pytest.mark.parametrize("pieces", [1, 3, 8])
def test_local_sdma_pipeline_pieces(pieces):
    """The pipelined schedule (sdma_comm.hip): each block in `pieces` pieces - reduce of piece k
    beside the engines' copies of k + 1, phase 2 and the gather per piece - including pieces
    that end inside a short last block and blocks with fewer pieces than the others."""
    from akka_allreduce_1_amd.parallel import LocalSdmaCluster

    P = 3
    cl = LocalSdmaCluster(P, slot_bytes=4 << 20, grid=16)
    for c in cl.comms:
        c.pieces = pieces
    for n in (2_500_003, 1_000_000, 12_289):
        xs = [fill_uniform(torch.empty(n, dtype=torch.bfloat16, device=DEV), seed=n + k) for k in range(P)]
        ys = cl.allreduce(xs)
        torch.cuda.synchronize()
        cl.check()
        ref = _ref(xs)
        for y in ys:
            assert (y.float() - ref).abs().max().item() <= _tol(torch.bfloat16, P)


def _mp_worker(rank, world, port, results):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import SdmaCommunicator

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok, msg = True, ""
    try:
        comm = SdmaCommunicator(device=0, slot_bytes=2 << 20, grid=8, engines_per_peer=1, timeout_s=15.0)
        for it, (n, dtype) in enumerate([(100_003, torch.float32), (1 << 20, torch.bfloat16), (5, torch.float32),
                                         (3_000_001, torch.bfloat16)] * 2):
            xs = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=100 * it + k) for k in range(world)]
            y = comm.allreduce(xs[rank])
            torch.cuda.synchronize()
            comm.check()
            err = (y.float() - _ref(xs)).abs().max().item()
            if err > _tol(dtype, world):
                ok, msg = False, f"it {it} n={n} {dtype} err={err}"
                break
    except Exception as e:  # report, never hang the parent
        ok, msg = False, repr(e)
    results.put((rank, ok, msg))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_multiprocess_sdma_allreduce(world):
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_mp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad



def _reuse_worker(rank, world, port, results):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import SdmaCommunicator

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok, msg = True, ""
    try:
        n = 24 << 20  # 48 MiB bf16 per rank: ~24 MiB engine copies per peer and phase, one engine each
        comm = SdmaCommunicator(device=0, slot_bytes=(2 * n) // world + (1 << 20), grid=64, engines_per_peer=1,
                                timeout_s=15.0)
        xs = [fill_uniform(torch.empty(n, dtype=torch.bfloat16, device=DEV), seed=70 + k) for k in range(world)]
        ref = _ref(xs)
        for it in range(6):
            y = comm.allreduce(xs[rank])
            snap = y.clone()  # stream-ordered after the call
            y.fill_(float("nan"))  # the caller reuses `out` at once: the peers must not see it
            torch.cuda.synchronize()
            comm.check()
            err = (snap.float() - ref).abs().max().item()
            if not err <= _tol(torch.bfloat16, world):
                ok, msg = False, f"it {it}: err {err}"
                break
            dist.barrier()
    except Exception as e:  # noqa: BLE001 - report, never hang the parent
        ok, msg = False, repr(e)
    results.put((rank, ok, msg))
    dist.destroy_process_group()


def test_multiprocess_sdma_output_reusable_right_after_the_call():
    """The engines read each rank's reduced block out of `out` for the peers (phase 2): the
    call must not count as done on the caller's stream before those copies are.
    Every rank overwrites its output with NaN right after each call; the peers' results must
    still be the sums."""
    from akka_allreduce_1_amd.parallel import free_port

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_reuse_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        res = [q.get(timeout=180) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad


def test_sdma_xdev_children_validate():
    """bench.py's N > 1 copy-engine section (benchmarks/sdma_xdev.py): one child process per
    rank, a gloo group of their own, validated against the exact sum and timed. Two 'ranks'
    share this GPU here (the same path a multi-GPU node takes, same-device copies)."""
    import threading

    from akka_allreduce_1_amd.parallel import free_port
    from benchmarks.sdma_xdev import run_children

    port = free_port()
    rows = [None, None]

    def go(r):
        rows[r] = run_children(r, 2, 0, port, mib=16, timeout=120.0)

    th = [threading.Thread(target=go, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(r and r.get("validated") for r in rows), rows
    assert all(r.get("p50_ms", 0) > 0 for r in rows), rows


def test_submitted_copies_are_the_planned_schedule():
    """Ties the CPU-tested schedule (tests/test_sdma_schedule.py) to what SdmaComm submits: after
    each call every rank's copy and byte counters moved by exactly the count and byte total of
    hip.plan_sdma_copies for that rank and each segment; integer-valued fp32, so the sum is exact."""
    from akka_allreduce_1_amd._native import C
    from akka_allreduce_1_amd.parallel import LocalSdmaCluster

    P, slot = 3, 64 << 10
    cl = LocalSdmaCluster(P, slot_bytes=slot, grid=4)
    for c in cl.comms:
        c.pieces = 3
    seg = P * (slot // 4)
    epoch = 0
    for n in (4096 + 5, seg + 7):  # one segment, then two
        xs = [torch.randint(-1000, 1000, (n,), generator=torch.Generator().manual_seed(n + k)).float().to(DEV)
              for k in range(P)]
        before = [dict(c.stats) for c in cl.comms]
        ys = cl.allreduce(xs)
        torch.cuda.synchronize()
        cl.check()
        lens = [min(seg, n - off) for off in range(0, n, seg)]
        for r, c in enumerate(cl.comms):
            plans = [C.hip.plan_sdma_copies(P, r, m, 4, c.engines_per_peer, c.slot_bytes, 3, (epoch + 1 + i) & 1)
                     for i, m in enumerate(lens)]
            assert all(len(p["copies"]) > 0 for p in plans)
            assert c.stats["calls"] - before[r]["calls"] == len(lens) == (1 if n <= seg else 2)
            assert c.stats["copies"] - before[r]["copies"] == sum(len(p["copies"]) for p in plans)
            assert c.stats["bytes"] - before[r]["bytes"] == sum(p["bytes"] for p in plans)
        epoch += len(lens)
        ref = xs[0] + xs[1] + xs[2]
        for y in ys:
            assert torch.equal(y, ref)
