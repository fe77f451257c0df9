"""xGMI broadcast and reduce (csrc/hip/xgmi_rooted.hip) on one MI355X: P logical ranks in one
launch (LocalCluster) and 2 / 3 processes with IPC-mapped slabs. A broadcast is checked
bit-exact; a reduce against the fp32 rank-order sum, and bit-exact against the reduce-scatter
of the same inputs where the blocks line up (the same reduce_to: same order, one rounding)."""
import os
import time

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from akka_allreduce_1_amd._native import C  # noqa: E402
from akka_allreduce_1_amd.ops import fill_uniform  # noqa: E402
from akka_allreduce_1_amd.ops.kernels import dtype_code  # noqa: E402
from akka_allreduce_1_amd.parallel import LocalCluster  # noqa: E402

DEV = torch.device("cuda", 0)
SIZES = [1, 10, 4099, 300_000]  # all but the first block empty (1, 10); a short last block and a
#                                 tail that is not 16 bytes; several segments at 256 KiB slots
_CLUSTERS: dict = {}
_INPUTS: dict = {}


def _cluster(P):
    if P not in _CLUSTERS:
        _CLUSTERS[P] = LocalCluster(P, slot_bytes=256 << 10, grid=64, timeout_s=10)
    return _CLUSTERS[P]


def _inputs(P, n, dtype):
    """The P rank tensors of a case (made once, never written: every test works on copies or
    reads them only)."""
    key = (P, n, dtype)
    if key not in _INPUTS:
        _INPUTS[key] = [fill_uniform(torch.empty(n, dtype=dtype, device=DEV), seed=31 * n + 7 * P + k)
                        for k in range(P)]
    return _INPUTS[key]


def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _run_broadcast(P, root, n, dtype):
    cl = _cluster(P)
    xs = _inputs(P, n, dtype)
    ts = [x.clone() for x in xs]  # non-roots hold other data beforehand
    got = cl.broadcast(ts, src=root)
    cl.check()
    assert all(g is t for g, t in zip(got, ts))
    for r in range(P):
        assert torch.equal(ts[r], xs[root]), (r, root)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("last_root", [False, True])
@pytest.mark.parametrize("P", [2, 3, 4, 8])
def test_broadcast(P, last_root, n, dtype):
    _run_broadcast(P, P - 1 if last_root else 0, n, dtype)


def test_broadcast_float16():
    _run_broadcast(4, 3, 4099, torch.float16)


def test_broadcast_one_rank_is_a_noop():
    cl = _cluster(1)
    t = fill_uniform(torch.empty(4099, device=DEV), seed=5)
    want = t.clone()
    launches = cl.comms[0].stats.launches
    cl.broadcast([t], src=0)
    cl.check()
    assert torch.equal(t, want) and cl.comms[0].stats.launches == launches


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("last_root", [False, True])
@pytest.mark.parametrize("P", [2, 3, 4, 8])
def test_reduce(P, last_root, n, dtype, scale):
    root = P - 1 if last_root else 0
    cl = _cluster(P)
    xs = _inputs(P, n, dtype)
    # every rank passes an output: off the root it is ignored and keeps its sentinel
    outs = [torch.full((n,), -7.0, dtype=dtype, device=DEV) for _ in range(P)]
    C.hip.XgmiComm.reduce_local(cl.comms, [x.data_ptr() for x in xs], [o.data_ptr() for o in outs], n,
                                dtype_code(dtype), root, torch.cuda.current_stream(DEV).cuda_stream, scale)
    cl.check()
    ref = torch.zeros(n, device=DEV)
    for s in range(P):
        ref += xs[s].float()
    err = (outs[root].float() - scale * ref).abs().max().item()
    print(f"reduce P={P} root={root} n={n} {dtype} scale={scale}: max abs err {err:.3e}")
    assert err <= (1e-6 if dtype == torch.float32 else 1e-2 * P), err
    for r in range(P):
        if r != root:
            assert torch.all(outs[r] == -7.0), r
    # the cluster's own entry allocates the output on the root
    out = cl.reduce(xs, root, scale=scale)
    cl.check()
    assert torch.equal(out, outs[root])
    m = n // P
    if n % P == 0 and (m * _es(dtype)) % 16 == 0:
        rs = cl.collective("reduce_scatter", xs, scale=scale)
        cl.check()
        assert torch.equal(outs[root], torch.cat(rs))


def test_reduce_one_rank_copies_and_scales():
    cl = _cluster(1)
    x = fill_uniform(torch.empty(4099, device=DEV), seed=6)
    assert torch.equal(cl.reduce([x], 0), x)
    assert torch.equal(cl.reduce([x], 0, scale=0.5), x * 0.5)
    cl.check()


def test_reduce_rejects_overlap_and_bad_roots():
    cl = _cluster(2)
    xs = _inputs(2, 4099, torch.float32)
    with pytest.raises(ValueError, match="overlap"):
        cl.reduce(xs, 1, xs[1])
    with pytest.raises(ValueError, match="overlap"):
        cl.reduce([x[:4000] for x in xs], 0, xs[0][96:4096])  # partly
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="root"):
            cl.reduce(xs, bad)
        with pytest.raises(ValueError, match="root"):
            cl.broadcast([x.clone() for x in xs], src=bad)
        with pytest.raises(ValueError, match="root"):
            C.hip.XgmiComm.broadcast_local(cl.comms, [x.data_ptr() for x in xs], 16, dtype_code(torch.float32), bad, 0)
    with pytest.raises(ValueError, match="16-byte aligned"):
        cl.broadcast([x.clone()[1:] for x in xs], src=0)
    cl.check()


SEQUENCE = ["ll", "broadcast", "ll", "broadcast", "oneshot", "reduce", "all_gather", "broadcast", "twoshot", "reduce",
            "all_to_all", "broadcast", "broadcast"]


def _rank_order_sum(xs):
    ref = xs[0].float().clone()
    for x in xs[1:]:
        ref += x.float()
    return ref


def test_rooted_interleaved_with_the_other_kernels():
    """Slots and flag rows are shared with every other kernel and reused across epochs; the
    low-latency kernel's parity slots rely on the broadcast root's acknowledgement wait."""
    P, n = 4, 65536
    m = n // P
    cl = LocalCluster(P, slot_bytes=1 << 20, grid=64, timeout_s=10)
    rooted = 0
    for it, kind in enumerate(SEQUENCE):
        xs = [fill_uniform(torch.empty(n, device=DEV), seed=1000 * it + k) for k in range(P)]
        root = rooted % P
        if kind == "broadcast":
            ts = [x.clone() for x in xs]
            cl.broadcast(ts, src=root)
            cl.check()
            assert all(torch.equal(t, xs[root]) for t in ts), (it, root)
            rooted += 1
        elif kind == "reduce":
            out = cl.reduce(xs, root)
            cl.check()
            assert torch.equal(out, _rank_order_sum(xs)), (it, root)
            rooted += 1
        elif kind == "all_gather":
            gs = [x[:m].contiguous() for x in xs]
            ys = cl.collective(kind, gs)
            cl.check()
            assert all(torch.equal(y, torch.cat(gs)) for y in ys), it
        elif kind == "all_to_all":
            ys = cl.collective(kind, xs)
            cl.check()
            assert all(torch.equal(ys[r][s * m:(s + 1) * m], xs[s][r * m:(r + 1) * m])
                       for r in range(P) for s in range(P)), it
        else:
            ys = cl.allreduce(xs, algo=kind)
            cl.check()
            ref = _rank_order_sum(xs)
            assert all((y - ref).abs().max().item() < 1e-5 for y in ys), (it, kind)
    assert rooted >= 2 * P - 1  # every rank was a root


def _spawn(target, world, *args, timeout=100.0):
    from akka_allreduce_1_amd.parallel import free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        res = [q.get(timeout=timeout) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=30 if len(res) == world else 1)
            if p.is_alive():
                p.kill()
    bad = [r for r in res if not r[1]]
    assert not bad, bad
    return res


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _sequence(comm, rank, world, roots, seed0):
    """The interleaved sequence on one process rank; every launch against rank-order fp32
    references. Returns "" or what differed."""
    n = 8192 * world
    m = n // world
    rooted = 0
    for it, kind in enumerate(SEQUENCE):
        xs = [fill_uniform(torch.empty(n, device=DEV), seed=seed0 + 100 * it + k) for k in range(world)]
        root = roots[rooted % len(roots)]
        if kind == "broadcast":
            t = comm.broadcast(xs[rank].clone(), src=root)
            ok = torch.equal(t, xs[root])
            rooted += 1
        elif kind == "reduce":
            out = comm.reduce(xs[rank], dst=root)
            ok = (out is None) if rank != root else torch.equal(out, _rank_order_sum(xs))
            rooted += 1
        elif kind == "all_gather":
            ok = torch.equal(comm.all_gather(xs[rank][:m].contiguous()), torch.cat([x[:m] for x in xs]))
        elif kind == "all_to_all":
            y = comm.all_to_all(xs[rank])
            ok = all(torch.equal(y[s * m:(s + 1) * m], xs[s][rank * m:(rank + 1) * m]) for s in range(world))
        else:
            y = comm.allreduce(xs[rank], algo=kind)
            ok = (y - _rank_order_sum(xs)).abs().max().item() < 1e-5
        comm.check()
        if not ok:
            return f"launch {it} ({kind}, root {root}) differs on rank {rank}"
    return ""


def _slow_reader_worker(rank, world, port, q):
    dist = _init(rank, world, port)
    ok, msg = True, ""
    try:
        from akka_allreduce_1_amd.parallel import XgmiCommunicator

        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=5)
        slow = world - 1
        comm.native.set_read_delay(slow, 2000.0)
        # the slow reader among the roots, then never a root
        for roots, seed0 in ((list(range(world))[::-1], 10_000), ([r for r in range(world) if r != slow], 50_000)):
            msg = _sequence(comm, rank, world, roots, seed0)
            if msg:
                ok = False
                break
    except Exception as e:  # noqa: BLE001
        ok, msg = False, repr(e)
    q.put((rank, ok, msg))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_processes_with_a_slow_reader(world):
    """A rank held inside its launch before its slab reads (2 ms): the fast ranks' next
    launches must not overwrite what it still reads, as a root and as a receiver."""
    _spawn(_slow_reader_worker, world)


def _invariant_worker(rank, world, port, q):
    dist = _init(rank, world, port)
    ok, msg = True, ""
    try:
        from akka_allreduce_1_amd.parallel import XgmiCommunicator

        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=5)
        n = 8192
        x0 = fill_uniform(torch.empty(n, device=DEV), seed=77)
        t = x0.clone() if rank == 0 else torch.zeros(n, device=DEV)
        comm.broadcast(t.clone(), src=0)  # code objects loaded, slabs touched
        comm.check()
        dist.barrier()
        t0 = time.perf_counter()
        if rank == 1:
            time.sleep(0.2)
        comm.broadcast(t, src=0)
        torch.cuda.synchronize(DEV)
        dt = time.perf_counter() - t0
        comm.check()
        if not torch.equal(t, x0):
            ok, msg = False, "broadcast result differs"
        elif rank == 0 and dt < 0.15:
            ok, msg = False, f"the root completed {dt:.3f} s after the barrier: before its peer entered the launch"
        else:
            msg = f"{dt:.3f} s"
    except Exception as e:  # noqa: BLE001
        ok, msg = False, repr(e)
    q.put((rank, ok, msg))
    dist.destroy_process_group()


def test_broadcast_root_waits_for_its_peers_entry():
    """The launch-sequence invariant: no rank completes launch e before it saw an epoch-e flag
    from every peer. A broadcast's root receives no data, so its peers acknowledge."""
    res = _spawn(_invariant_worker, 2)
    print("wall time barrier -> synchronized:", sorted(res))


def _fallback_worker(rank, world, port, q):
    dist = _init(rank, world, port)
    ok, msg = True, ""
    try:
        from akka_allreduce_1_amd.parallel import XgmiCommunicator

        comm = XgmiCommunicator(device=0, slot_bytes=1 << 20, grid=8, timeout_s=5)
        ints = [torch.arange(1000, device=DEV, dtype=torch.int64) * (k + 3) for k in range(world)]
        offs = [fill_uniform(torch.empty(1001, device=DEV), seed=300 + k)[1:] for k in range(world)]
        assert offs[rank].data_ptr() % 16 == 4
        launches = comm.native.stats.launches
        for xs in (ints, offs):
            t = torch.empty(xs[rank].numel() + 1, dtype=xs[rank].dtype, device=DEV)[1:].copy_(xs[rank])
            assert t.data_ptr() % 16 or t.dtype == torch.int64  # a clone would be aligned again
            if comm.broadcast(t, src=1) is not t or not torch.equal(t, xs[1]):
                ok, msg = False, f"{xs[0].dtype} broadcast differs"
            out = comm.reduce(xs[rank], dst=1)
            if rank == 1:
                ref = sum(x.double() for x in xs)
                if out is None or (out.double() - ref).abs().max().item() > 1e-5:
                    ok, msg = False, f"{xs[0].dtype} reduce differs"
            elif out is not None:
                ok, msg = False, "reduce returned an output off the root"
        if comm.native.stats.launches != launches:
            ok, msg = False, "the fall-back cases ran on the kernels"
        # a misaligned output alone stays on the kernels (every rank must take the same path)
        xs = [fill_uniform(torch.empty(1000, device=DEV), seed=400 + k) for k in range(world)]
        out = comm.reduce(xs[rank], torch.empty(1001, device=DEV)[1:] if rank == 0 else None, dst=0)
        comm.check()
        if rank == 0 and not torch.equal(out, _rank_order_sum(xs)):
            ok, msg = False, "reduce into a misaligned output differs"
        for bad in (-1, world):
            for call in (lambda: comm.broadcast(xs[rank], src=bad), lambda: comm.reduce(xs[rank], dst=bad)):
                try:
                    call()
                    ok, msg = False, f"root {bad} was accepted"
                except ValueError:
                    pass
    except Exception as e:  # noqa: BLE001
        ok, msg = False, repr(e)
    q.put((rank, ok, msg))
    dist.destroy_process_group()


def test_communicator_falls_back_to_torch_distributed():
    _spawn(_fallback_worker, 2)
