"""The fused xGMI allreduce kernels on one MI355X.

* LocalCluster: P logical ranks in one process, one HIP stream each (connect_local).
* Multi-process: P processes on the same GPU exchange hipIpcMemHandles over gloo and map
  each other's slabs - the exact one-process-per-GPU path, minus the xGMI hop.
Every result is compared with an fp32 torch reference summed in rank order.
"""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from akka_allreduce_1_amd.ops import fill_uniform  # noqa: E402
from akka_allreduce_1_amd.parallel import LocalCluster  # noqa: E402

DEV = torch.device("cuda", 0)


def _ref(xs):
    acc = torch.zeros(xs[0].numel(), device=xs[0].device)
    for x in xs:
        acc += x.float()
    return acc


def _tol(dtype, P, algo=""):
    if dtype == torch.float32:
        return 0.0
    if algo == "ring_native":  # one rounding per hop of partials |p| <= P: (P - 1) x half an ulp of P
        return 1e-2 * P * P
    return 1e-2 * P


def _diag(y, ref, xs, rank):
    """Where a wrong result differs (helps tell a stale read from a missing contribution)."""
    bad = ((y.float() - ref).abs() > 1e-3).nonzero().flatten()
    if bad.numel() == 0:
        return "no bad elements"
    i = int(bad[0])
    own = xs[rank].float()[i].item()
    return (f"{bad.numel()} bad, first idx {i} last {int(bad[-1])}, y={y[i].item():.4f} ref={ref[i].item():.4f} "
            f"own={own:.4f}")


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("algo", ["twoshot", "oneshot", "ring", "ring_native", "ll"])
@pytest.mark.parametrize("n", [1, 7, 1000, 65536 + 3, 1 << 20])
def test_local_cluster_allreduce(P, dtype, algo, n):
    cl = LocalCluster(P, slot_bytes=4 << 20, grid=32, timeout_s=10.0)
    xs = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=100 * P + k) for k in range(P)]
    ys = cl.allreduce(xs, algo=algo)
    cl.check()
    ref = _ref(xs)
    for k, y in enumerate(ys):
        err = (y.float() - ref).abs().max().item() if n else 0.0
        if err > _tol(dtype, P, algo) + (1e-6 if dtype == torch.float32 else 0):
            pytest.fail(f"P={P} {dtype} {algo} n={n} rank {k}: err {err}: {_diag(y, ref, xs, k)}")


def test_local_cluster_inplace_and_repeated_epochs():
    P = 4
    cl = LocalCluster(P, slot_bytes=1 << 20, grid=8, timeout_s=10.0)
    for it in range(6):
        n = [4096, 300_000, 17][it % 3]
        xs = [fill_uniform(torch.empty(n, device=DEV), seed=it * 10 + k) for k in range(P)]
        ref = _ref(xs)
        ys = cl.allreduce(xs, xs, algo="auto")  # in place
        cl.check()
        for y in ys:
            assert torch.allclose(y, ref, atol=1e-5)


@pytest.mark.parametrize("algo", ["twoshot", "ring", "ring_native", "ll"])
def test_local_cluster_segments_larger_than_slab(algo):
    P = 2
    cl = LocalCluster(P, slot_bytes=64 << 10, grid=8, timeout_s=10.0)
    n = 100_000 if algo != "ll" else 300_000  # > P * 64 KiB (> ll_max_bytes for ll) -> several launches
    xs = [fill_uniform(torch.empty(n, device=DEV), seed=k) for k in range(P)]
    ys = cl.allreduce(xs, algo=algo)
    cl.check()
    assert cl.comms[0].stats.launches > 1
    for y in ys:
        assert torch.allclose(y, _ref(xs), atol=1e-5)


def _mp_worker(rank, world, port, results):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import XgmiCommunicator

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok = True
    msg = ""
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=2 << 20, grid=8, timeout_s=15.0)
        for dtype in (torch.float32, torch.bfloat16):
            # "~1": the coarse two-shot geometry the tuner tries on large blocks (one scatter
            # unit per workgroup), then the default geometry again
            for n, algo in ((100_003, "twoshot"), (5_000, "oneshot"), (1 << 20, "auto"), (3_333, "ll"),
                            (300_001, "ll"), (100_003, "twoshot~1"), (1 << 20, "twoshot@4~1"), (1 << 20, "twoshot"),
                            (1 << 20, "twoshot@full"), (100_003, "twoshot")):
                xs = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=k) for k in range(world)]
                y = comm.allreduce(xs[rank], algo=algo)
                comm.check()
                err = (y.float() - _ref(xs)).abs().max().item()
                if err > _tol(dtype, world) + 1e-5:
                    ok, msg = False, f"{dtype} {algo} n={n} err={err}"
        comm.barrier()
        comm.check()
    except Exception as e:  # report, never hang the parent
        ok, msg = False, repr(e)
    results.put((rank, ok, msg))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_multiprocess_ipc_allreduce(world):
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_mp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in range(world):
        res.append(q.get(timeout=240))
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad


_SLOW_READER_SEQ = {
    # one-shot S -> one-shot, two-shot R -> all-gather, all-to-all S -> all-to-all
    "mixed": ["oneshot", "oneshot", "twoshot", "all_gather", "all_to_all", "all_to_all", "oneshot", "twoshot",
              "all_gather", "all_gather", "reduce_scatter", "oneshot"],
    # the ring's hop flags next to the other kernels' writer-row flags (round-3 collision)
    "ring": ["ring", "all_gather", "ring", "twoshot", "ring_native", "all_gather", "ring", "ring", "all_gather",
             "oneshot", "ring", "reduce_scatter", "ring_native", "twoshot"],
}


def _slot_reuse_worker(rank, world, port, results, slow=1, seq="mixed", env=None):
    """Rank `slow` idles 2 ms before every slab-reading phase; a rank that needs nothing more
    from it once its pushes are in runs ahead into the next launch and would push into the
    slots the slow rank is about to read without the entry guard (xgmi_device.h). In a ring of
    >= 3 ranks the slow rank's late forwards also land after a peer's next launch has begun:
    with the round-3 flag layout (row = hop) such a late ring flag overwrote a newer
    all-gather flag of another writer (profiles/round3/soak8_run4_ring_flag_collision.log)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", **(env or {}))
    import datetime

    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import XgmiCommunicator

    torch.cuda.set_device(0)
    ok, msg = True, ""
    try:  # a lost rendezvous (the port taken meanwhile) must fail fast, not hang the parent
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    except Exception as e:  # noqa: BLE001
        results.put((rank, False, f"rendezvous: {e!r}"))
        return
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=5.0)
        comm.native.set_read_delay(slow, 2000.0)
        n = 8192 * world
        for it, op in enumerate(_SLOW_READER_SEQ[seq] * 2):
            xs = [fill_uniform(torch.empty(n, device=DEV), seed=1000 * it + k) for k in range(world)]
            m = n // world
            if op == "all_gather":
                y, ref = comm.all_gather(xs[rank][:m].clone()), torch.cat([x[:m] for x in xs])
            elif op == "all_to_all":
                y, ref = comm.all_to_all(xs[rank]), torch.cat([x[rank * m:(rank + 1) * m] for x in xs])
            elif op == "reduce_scatter":
                y, ref = comm.reduce_scatter(xs[rank], op="sum"), _ref(xs)[rank * m:(rank + 1) * m]
            else:
                y, ref = comm.allreduce(xs[rank], algo=op), _ref(xs)
            comm.check()
            err = (y.float() - ref).abs().max().item()
            if err > 1e-5:
                ok, msg = False, f"launch {it} ({op}) rank {rank}: err {err}"
                break
        comm.native.set_read_delay(-1, 0.0)
        comm.barrier()
        comm.check()
    except Exception as e:  # report, never hang the parent
        ok, msg = False, repr(e)
    results.put((rank, ok, msg))
    dist.destroy_process_group()


def _run_slow_reader(world, slow, seq, env=None):
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_slot_reuse_worker, args=(r, world, port, q, slow, seq, env)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        res = [q.get(timeout=150) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return [r for r in res if not r[1]]


@pytest.mark.parametrize("world,slow,seq", [(2, 1, "mixed"), (3, 2, "ring"), (4, 3, "ring"), (3, 1, "mixed")])
def test_multiprocess_slot_reuse_slow_reader(world, slow, seq):
    bad = _run_slow_reader(world, slow, seq)
    assert not bad, bad


def _big_slab_worker(rank, world, port, slot, results):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import XgmiCommunicator

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok, msg = True, ""
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=slot, grid=16, timeout_s=15.0)
        alloc, slab = comm.native.alloc_bytes, comm.native.slab_bytes
        if not (alloc >= slab and not (alloc >> 31) & 1):
            ok, msg = False, f"allocation {alloc} keeps bit 31 (slab {slab})"
        n = world * slot // 4  # fill every slot of the slab
        xs = [fill_uniform(torch.empty(n, device=DEV), seed=k) for k in range(world)]
        y = comm.allreduce(xs[rank], algo="twoshot")
        comm.check()
        err = (y - _ref(xs)).abs().max().item()
        if err > 1e-5:
            ok, msg = False, f"err {err}"
    except Exception as e:  # noqa: BLE001
        ok, msg = False, repr(e)
    results.put((rank, ok, msg))
    dist.destroy_process_group()


def test_multiprocess_slab_in_ipc_size_hole():
    """A 2.3 GiB slab (size bit 31 set) hangs hipIpcOpenMemHandle on this stack unless the
    allocation is padded to 4 GiB: the communicator must connect and reduce correctly."""
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    slot = 600 << 20
    procs = [ctx.Process(target=_big_slab_worker, args=(r, 2, port, slot, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=100) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_local_cluster_mean_fused(dtype, P):
    cl = LocalCluster(P, slot_bytes=1 << 20, grid=16)
    n = 50_001
    xs = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=k) for k in range(P)]
    ys = cl.allreduce(xs, op="avg")
    cl.check()
    ref = _ref(xs) / P
    for y in ys:
        assert (y.float() - ref).abs().max().item() <= (1e-6 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("algo", ["oneshot", "twoshot", "ring", "ll"])
@pytest.mark.parametrize("P", [2, 4])
def test_inplace_no_input_overwrite_race(algo, P):
    """In-place: a rank's reduced output must never leak into what a peer receives as that
    rank's contribution (the input may only be overwritten after every push read it)."""
    cl = LocalCluster(P, slot_bytes=2 << 20, grid=64)
    for it in range(8):
        n = 60_001 if algo in ("oneshot", "ll") else 200_003
        xs = [fill_uniform(torch.empty(n, device=DEV), seed=1000 * it + k) for k in range(P)]
        ref = _ref(xs)
        cl.allreduce(xs, xs, algo=algo)
        cl.check()
        for k, y in enumerate(xs):
            err = (y - ref).abs().max().item()
            if err > 1e-5:
                pytest.fail(f"it {it} rank {k}: err {err}: {_diag(y, ref, xs, k)}")


def test_stress_cluster_churn():
    """Clusters created and destroyed with changing rank counts, slot sizes and lengths: new
    slabs land on memory that old slabs (with other layouts) just used, the pattern that
    exposes any flag-before-data ordering hole (a stale slab read shows as a wrong sum)."""
    import random

    rng = random.Random(1234)
    for it in range(40):
        P = rng.choice([2, 3, 4])
        slot = rng.choice([1 << 20, 2 << 20, 4 << 20])
        dtype = rng.choice([torch.float32, torch.bfloat16])
        es = 4 if dtype == torch.float32 else 2
        n = rng.randint(1, (slot * P) // es)
        algo = rng.choice(["auto", "twoshot", "oneshot", "ll"]) if n * es <= slot else rng.choice(["twoshot", "ll"])
        cl = LocalCluster(P, slot_bytes=slot, grid=rng.choice([8, 32, 64]))
        xs = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=rng.randint(0, 1 << 30)) for _ in range(P)]
        ref = _ref(xs)
        ys = cl.allreduce(xs, algo=algo)
        cl.check()
        for k, y in enumerate(ys):
            err = (y.float() - ref).abs().max().item()
            if err > _tol(dtype, P) + (1e-5 if dtype == torch.float32 else 0):
                pytest.fail(f"it {it} P={P} n={n} {dtype} {algo} rank {k}: err {err}: {_diag(y, ref, xs, k)}")
        del cl, xs, ys


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ring_eight_ranks_mean_and_repeats(dtype):
    """P = 8 ring (7 reduce-scatter + 7 all-gather hops per chunk), mean fused, repeated
    launches reusing the same slots (the cross-launch slot-reuse argument of ring_kernel)."""
    P = 8
    cl = LocalCluster(P, slot_bytes=1 << 20, grid=64, timeout_s=10.0)
    for it in range(5):
        n = [1 << 20, 12_345, 3 * (1 << 18) + 5][it % 3]
        xs = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=50 * it + k) for k in range(P)]
        ref = _ref(xs) / P
        ys = cl.allreduce(xs, op="avg", algo="ring")
        cl.check()
        for k, y in enumerate(ys):
            err = (y.float() - ref).abs().max().item()
            assert err <= (1e-6 if dtype == torch.float32 else 1e-2), f"it {it} rank {k}: {err}"
    assert cl.comms[0].stats.ring >= 5


def test_mxar_bench_local_cli(tmp_path):
    from akka_allreduce_1_amd.bench_cli import main

    out = tmp_path / "rows.jsonl"
    assert main(["--local", "4", "--algos", "twoshot", "ring", "oneshot", "ll", "all_to_all", "all_gather",
                 "reduce_scatter", "--sizes", "64K", "4M", "--iters", "3", "--json", str(out)]) == 0
    import json

    rows = [json.loads(l) for l in out.read_text().splitlines()]
    assert {(r["bytes"], r["algo"]) for r in rows} >= {(65536, "twoshot"), (65536, "ring"), (4 << 20, "twoshot"),
                                                       (65536, "ll"), (4 << 20, "all_to_all"),
                                                       (4 << 20, "reduce_scatter"), (65536, "all_gather")}


@pytest.mark.parametrize("algo", ["oneshot", "twoshot", "ring", "ll"])
def test_hipgraph_capture_and_replay(algo):
    """The allreduce launch is graph-safe: flags carry an epoch read from a device counter at
    run time, so one captured launch replays correctly many times (new data each replay)."""
    P, n = 4, 100_003
    cl = LocalCluster(P, slot_bytes=1 << 20, grid=32, timeout_s=10.0)
    xs = [torch.empty(n, device=DEV) for _ in range(P)]
    ys = [torch.empty(n, device=DEV) for _ in range(P)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cl.allreduce(xs, ys, algo=algo)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cl.allreduce(xs, ys, algo=algo, op="avg")
    for it in range(6):
        for k in range(P):
            fill_uniform(xs[k], seed=700 + 10 * it + k)
        g.replay()
        cl.check()
        ref = _ref(xs) / P
        for k in range(P):
            assert (ys[k] - ref).abs().max().item() <= 1e-6, f"replay {it} rank {k}"


@pytest.mark.parametrize("P", [2, 4, 8])
def test_local_cluster_large_blocks_fine_geometry(P):
    """Blocks >= 32 MiB switch the two-shot to one chunk per workgroup, reduced in <= 2
    pieces (plan_twoshot); odd sizes, in place, bf16."""
    n = P * (20 << 20) + 12_345  # 40 MiB bf16 blocks
    cl = LocalCluster(P, slot_bytes=48 << 20, grid=512, timeout_s=20.0)
    xs = [fill_uniform(torch.empty(n, dtype=torch.bfloat16, device=DEV), seed=3000 + k) for k in range(P)]
    ref = _ref(xs)
    ys = cl.allreduce(xs, xs, algo="twoshot")  # in place
    cl.check()
    for k, y in enumerate(ys):
        err = (y.float() - ref).abs().max().item()
        assert err <= 1e-2 * P, (k, err)


def _recover_worker(rank, world, port, results):
    """Rank 1 skips one collective: rank 0 times out (CommError). After a collective reset()
    both ranks reduce exactly again, with every algorithm."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import CommError, XgmiCommunicator

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok, msg = True, ""
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=2.0, max_lag=1)
        x = fill_uniform(torch.empty(50_000, device=DEV), seed=rank)
        if rank == 0:
            comm.allreduce(x, algo="twoshot")
            try:
                comm.check()
                ok, msg = False, "expected a CommError"
            except CommError:
                pass
        dist.barrier()
        comm.reset()
        assert comm.error() == 0
        xs = [fill_uniform(torch.empty(50_000, device=DEV), seed=10 + k) for k in range(world)]
        for algo in ("twoshot", "oneshot", "ll", "ring", "threshold", "twoshot"):
            y = comm.allreduce(xs[rank], algo=algo)
            comm.check()
            err = (y - _ref(xs)).abs().max().item()
            if err > 1e-5:
                ok, msg = False, f"{algo} after reset: err {err}"
        g = comm.all_gather(xs[rank][:1024].contiguous())
        comm.check()
        if not torch.equal(g[1024:2048] if rank == 0 else g[:1024], xs[1 - rank][:1024]):
            ok, msg = False, "all_gather after reset"
    except Exception as e:  # noqa: BLE001
        ok, msg = False, repr(e)
    results.put((rank, ok, msg))
    dist.destroy_process_group()


def test_reset_recovers_after_a_missed_collective():
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_recover_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=100) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad


def _links_worker(rank, world, port, results):
    """The xGMI bring-up pack (utils/links.py) between processes sharing the GPU: every probe
    returns rates and latencies, and the collectives around it still validate (the probes
    touch no flag or control word)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import datetime

    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import XgmiCommunicator
    from akka_allreduce_1_amd.utils.links import probe_links

    torch.cuda.set_device(0)
    ok, msg, info = True, "", None
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=8 << 20, grid=8, timeout_s=10.0)
        n = 100_003
        xs = [fill_uniform(torch.empty(n, device=DEV), seed=k) for k in range(world)]
        y0 = comm.allreduce(xs[rank], algo="twoshot")
        info = probe_links(comm, nbytes=4 << 20, reps=2, iters=200, grid=4)
        y1 = comm.allreduce(xs[rank], algo="twoshot")
        y2 = comm.allreduce(xs[rank], algo="oneshot")
        comm.check()
        for y in (y0, y1, y2):
            err = (y - _ref(xs)).abs().max().item()
            if err > 1e-5:
                ok, msg = False, f"err {err} after the probe"
        singles = [v for i, row in enumerate(info["push_GBps"]) for k, v in enumerate(row) if k != i]
        if not (len(info["all_GBps"]) == world and min(singles) > 0 and min(info["all_GBps"]) > 0):
            ok, msg = False, f"rates {info}"
        for key in ("coarse", "pull"):  # the coarse-grained push and the pull ran and moved bytes
            m = info.get(key) or {}
            if not (min(m.get("single_GBps_min_med_max") or [0]) > 0 and min(m.get("all_GBps_min_max") or [0]) > 0):
                ok, msg = False, f"{key} rates {info}"
        lat = info["flag_us"]
        if rank == 0 and not all(lat[m][k] and lat[m][k] > 0 for m in ("bare", "fenced") for k in range(1, world)):
            ok, msg = False, f"latencies {lat}"
    except Exception as e:  # noqa: BLE001 - report, never hang the parent
        ok, msg = False, repr(e)
    results.put((rank, ok, msg, info if rank == 0 else None))
    dist.destroy_process_group()


def test_multiprocess_link_probes():
    from akka_allreduce_1_amd.parallel import free_port

    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_links_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        res = [q.get(timeout=150) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    bad = [r[:3] for r in res if not r[1]]
    assert not bad, bad
    info = next(r[3] for r in res if r[0] == 0)
    print("link probes:", info["single_GBps_min_med_max"], info["all_GBps"], info["flag_us"])


def _flag_owner_worker(rank, world, port, results, env=None):
    """Flag ownership, deterministically (verdict r4 #8): rank 2 of 3 holds its ring's LAST
    all-gather forward (the flag into rank 0's slab) for 3 ms. Rank 1 needs nothing more from
    rank 2, finishes the ring and starts an all_gather, whose flag into rank 0 is, in the
    round-3 layout (MXAR_RING_FLAGS=hop: ring flag row = hop index 1), the SAME word as rank 2's
    late ring flag - rank 0 then takes rank 1's newer epoch for rank 2's data (stale ring
    output), or rank 2's late store overwrites rank 1's newer epoch (the all_gather times out).
    In the shipped layout every flag word has one writer and both results are exact."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", **(env or {}))
    import datetime

    import torch.distributed as dist

    from akka_allreduce_1_amd.parallel import XgmiCommunicator

    torch.cuda.set_device(0)
    ok, msg = True, ""
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    except Exception as e:  # noqa: BLE001
        results.put((rank, False, f"rendezvous: {e!r}"))
        return
    try:
        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=4.0)
        comm.native.set_forward_delay(2, 3000.0)
        n = 8192 * world
        m = n // world
        for it in range(4):
            xs = [fill_uniform(torch.empty(n, device=DEV), seed=300 * it + k) for k in range(world)]
            y = comm.allreduce(xs[rank], algo="ring")
            comm.check()
            err = (y - _ref(xs)).abs().max().item()
            if err > 1e-5:
                ok, msg = False, f"iteration {it} ring rank {rank}: err {err}"
                break
            y2 = comm.all_gather(xs[rank][:m].clone())
            comm.check()
            err = (y2 - torch.cat([x[:m] for x in xs])).abs().max().item()
            if err > 1e-6:
                ok, msg = False, f"iteration {it} all_gather rank {rank}: err {err}"
                break
        comm.native.set_forward_delay(-1, 0.0)
        comm.barrier()
        comm.check()
    except Exception as e:  # report, never hang the parent
        ok, msg = False, repr(e)[:300]
    results.put((rank, ok, msg))
    dist.destroy_process_group()


def _run_flag_owner(env=None):
    from akka_allreduce_1_amd.parallel import free_port

    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_flag_owner_worker, args=(r, world, port, q, env)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        res = [q.get(timeout=150) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return [r for r in res if not r[1]]


def test_ring_flag_ownership_late_forward():
    bad = _run_flag_owner()
    assert not bad, bad


def test_solo_rehearsal_comm_runs_one_rank_of_an_8_rank_two_shot():
    """benchmarks/sections.py SoloRehearsalComm (the DP-overlap rehearsal's comm): rank 0 of an
    8-rank two-shot runs alone with its peers' flags pre-armed - it never waits, and since the
    synthetic peers contribute zeros and never reduce, the own block keeps the input and the
    gathered blocks read zeros. Repeated calls (epochs advance) keep doing exactly that."""
    from benchmarks.sections import SoloRehearsalComm

    class _B:
        def __init__(self, t):
            self.buffer, self.nbytes = t, t.numel() * t.element_size()

    n = (3 << 20) + 40  # bf16 elements: blocks of ceil(n / 8) rounded to 16 B
    t = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    comm = SoloRehearsalComm([_B(t)], 8, 64)
    blk = -(-(-(-n // 8)) // 8) * 8
    for _ in range(3):
        t.fill_(1.0)
        comm.allreduce_(t, op="sum")
        comm.check()
        assert bool((t[:blk] == 1).all()) and bool((t[blk:] == 0).all())
    assert SoloRehearsalComm.hbm_bytes(1 << 30, 8) == int(2 * ((1 << 30) + 2 * (1 << 30) * 7 / 8))
