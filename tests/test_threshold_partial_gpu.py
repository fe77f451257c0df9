"""Threshold rounds that really leave a contribution out, bit for bit, in every element type.

tests/test_exact_numerics_gpu.py pins the threshold kernel (csrc/hip/xgmi_threshold.hip) at
thresholds 1.0. Here one rank straggles (XgmiComm.set_straggler: a bounded 5 ms idle at the start
of its part of the launch) under thReduce = thComplete = (P - 1) / P, so the fast ranks reduce
without it, give its block up, and everything that differs from a full round runs: reduce_masked
with a partial mask (sources outside the mask add +0) in its 2-, 4- and 8-source instantiations
and its scalar tail, zero_fill of given-up chunks, the rescale coefficient scale * P / count,
rounds in place and rounds cycling through the lag-ring rows. The protocol plane (PlaneJob, a
causal host-side straggler) adds the element-wise twins that geometry off the 16-byte grid takes
(reduce_masked_scalar, copy_in_scalar, copy_out_scalar, the unaligned zero_fill), in bf16 and
fp16 too.

Every output is held to `check_partial_round` (akka_allreduce_1_amd/utils/exact_data.py; its own
tests and the case table are tests/test_partial_round.py): per chunk, +0 bits where the count
is 0, else the ONE round-to-nearest-even of the exact sum over a contributor set of exactly
`count` ranks times the fp32 coefficient. Which fast chunk a fast rank still takes before it
completes is a matter of timing, so the expectation comes from the counts the kernel reports;
what does not depend on timing is asserted on the counts themselves. No tolerance anywhere but
the fp64 cross-check of the rescaled mean, whose bound is derived: the result is
RN_type(RN_32(s * c)) with s exact and c = float32(1 / count) (tests/test_partial_round.py), so it
is within 2^-p (half an ulp of the type) + 2^-24 (c) + 2^-24 (the product) + their products
< 2^-p + 2^-22 of the fp64 mean, relative.

The straggler knob keeps the rounds on the launch path of LocalCluster (one launch per round, all
ranks in it); the resident kernels are not covered here, the group kernel only as far as
PlaneJob's co-located workers take it.
"""
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

from akka_allreduce_1_amd._native import C  # noqa: E402
from akka_allreduce_1_amd.engine import PlaneJob  # noqa: E402
from akka_allreduce_1_amd.parallel import LocalCluster  # noqa: E402
from akka_allreduce_1_amd.utils.exact_data import (PRECISION, check_partial_round, chunk_ranges,  # noqa: E402
                                                   exact_inputs)
from test_partial_round import (DTYPES, FULL_BATCH_PACKS, GRID, LAGS, NMAX, PLANE_CHUNKS, PLANE_N,  # noqa: E402
                                PLANE_P, PLANE_ROUNDS, SLOT, SMALL_GRID, WORLDS, chunks_per_block, cluster_knobs,
                                direct_cases, direct_seed, es_of, full_batch_size, partial_th, plane_ranges,
                                plane_seed)

H = C.hip
DEV = torch.device("cuda", 0)
GUARD = 64       # sentinel elements behind every out-of-place output
SENTINEL = -7.0  # and in the output itself before the round: a given-up chunk must really be written
IDLE_US = 5000.0
KNOBS = ("world", "rows", "grid", "default_grid", "size_grid", "maxch", "slot_bytes", "th_oneshot_max",
         "no_gate_shortcut")

_CLUSTERS: dict = {}
_DATA: dict = {}


def _cluster(P, max_lag, grid=GRID):
    key = (P, max_lag, grid)
    if key not in _CLUSTERS:
        cl = LocalCluster(P, slot_bytes=SLOT, grid=grid, timeout_s=10, max_lag=max_lag)
        # the case table was planned on the CPU for exactly these knobs
        k, want = cl.comms[0].knobs, cluster_knobs(P, max_lag, grid)
        assert [getattr(k, f) for f in KNOBS] == [getattr(want, f) for f in KNOBS]
        _CLUSTERS[key] = cl
    return _CLUSTERS[key]


class _Data:
    """The NMAX-element rank tensors of (P, dtype, mode), on the CPU and on the GPU, never written;
    a round works on clones of a prefix. `memo[n]` keeps the checker's expected sums of that prefix."""

    def __init__(self, P, dtype, mode):
        self.cpu = exact_inputs(P, NMAX, dtype, mode, seed=direct_seed(P, dtype, mode))
        self.xs = [x.to(DEV) for x in self.cpu]
        self.dtype = dtype
        self.memo: dict = {}
        self.means: dict = {}

    def inputs(self, n):
        return [x[:n].clone() for x in self.xs]

    def mean(self, S):
        """fp64 mean over the ranks in S."""
        if S not in self.means:
            self.means[S] = torch.stack([self.cpu[k].double() for k in sorted(S)]).sum(0) / len(S)
        return self.means[S]


def _data(P, dtype, mode):
    key = (P, dtype, mode)
    if key not in _DATA:
        _DATA[key] = _Data(P, dtype, mode)
    return _DATA[key]


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _allowed(P, slow):
    everyone = frozenset(range(P))
    return {P: [everyone], P - 1: [everyone - {slow}]}


def _check_round(xs_cpu, xs_gpu, ins, bufs, ys, counts, plan, slow, scale, rescale, memo, what, th_full=False):
    """Every assertion on one round. xs_cpu / xs_gpu: the round's rank tensors; ins: what the
    kernel was given (clones; the outputs themselves when in place, then bufs is None)."""
    P, n = len(xs_cpu), xs_cpu[0].numel()
    dtype = xs_cpu[0].dtype
    geo = (plan["block"], plan["chunk"], plan["nch"])
    nch = plan["nch"]
    per = chunks_per_block(plan, n, P)
    counts = counts.cpu()
    assert tuple(counts.shape) == (P, P, nch), f"{what}: counts {tuple(counts.shape)}"
    allowed = {P: [frozenset(range(P))]} if th_full else _allowed(P, slow)
    ranges = chunk_ranges(n, P, *geo)
    lens = torch.tensor([hi - lo for lo, hi in ranges])
    outs, taken, found = [], [], []
    for k in range(P):
        y = ys[k].cpu()
        ck = counts[k]
        f = check_partial_round(xs_cpu, y, ck, geo, dtype, scale, rescale, allowed=allowed, memo=memo,
                                what=f"{what} rank {k} (counts {ck.tolist()})")
        outs.append(y)
        found.append(f)
        taken.append(torch.repeat_interleave(ck.flatten() > 0, lens))
        # what does not depend on timing
        for j in range(P):
            cj = ck[j, :per[j]].tolist()
            if th_full:
                want = [P] * per[j]
            elif j == slow:  # complete on the straggler, given up everywhere else
                want = [P if k == slow else 0] * per[j]
            elif j == k:     # a fast rank's own block: reduced without the straggler, always taken
                want = [P - 1] * per[j]
            else:
                continue
            assert cj == want, f"{what} rank {k} block {j}: counts {cj}, expected {want} (all: {ck.tolist()})"
        if k != slow:
            got = int((ck > 0).sum())
            assert got >= plan["min_complete"], f"{what} rank {k}: {got} chunks taken, min_complete {plan['min_complete']}"
        if bufs is not None:
            assert bool((bufs[k][n:] == SENTINEL).all()), f"{what} rank {k}: wrote past the end of the output"
            assert torch.equal(_bits(ins[k]), _bits(xs_gpu[k][:n])), f"{what} rank {k}: the input was written"
    for a in range(P):  # the ranks that took a chunk agree on it bit for bit
        for b in range(a + 1, P):
            both = taken[a] & taken[b]
            assert torch.equal(_bits(outs[a])[both], _bits(outs[b])[both]), f"{what}: ranks {a} and {b} differ on a chunk both took"
    return outs, found, ranges


def _cross_check_mean(data, outs, found, ranges, what):
    """avg with rescale against the fp64 mean over the contributors the checker identified."""
    bound = 2.0 ** -PRECISION[data.dtype] + 2.0 ** -22
    for k, y in enumerate(outs):
        for (lo, hi), S in zip(ranges, found[k]):
            if hi <= lo or not S:
                continue
            mean = data.mean(S)[lo:hi]
            got = y[lo:hi].double()
            over = ((got - mean).abs() > bound * mean.abs()).nonzero().flatten()
            assert over.numel() == 0, (f"{what} rank {k} [{lo}, {hi}): {over.numel()} elements beyond the bound, first "
                                       f"{lo + int(over[0])}: got {float(got[over[0]])!r} mean {float(mean[over[0]])!r}")


def _run_round(cl, data, n, plan, slow, op, rescale, inplace, what, th=None):
    P, dtype = cl.world, data.dtype
    th = partial_th(P) if th is None else th
    ins = data.inputs(n)
    bufs = None if inplace else [torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV) for _ in range(P)]
    ys, counts = cl.allreduce_threshold(ins, ins if inplace else [b[:n] for b in bufs], th_reduce=th, th_complete=th,
                                        op=op, rescale=rescale)
    cl.check()
    scale = 1.0 / P if op == "avg" else 1.0
    xs_cpu = [x[:n] for x in data.cpu]
    outs, found, ranges = _check_round(xs_cpu, data.xs, ins, bufs, ys, counts, plan, slow, scale, rescale,
                                       data.memo.setdefault(n, {}), what, th_full=th >= 1.0)
    if op == "avg" and rescale:
        _cross_check_mean(data, outs, found, ranges, what)
    return counts


def _planned(cl, P, dtype, cases):
    """The CPU table's plans are the plans of this cluster."""
    th, es = partial_th(P), es_of(dtype)
    for n, plan, _ in cases:
        assert H.plan_threshold(cl.comms[0].knobs, n, es, P, th, th) == plan, n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("max_lag", LAGS)
@pytest.mark.parametrize("P", WORLDS)
def test_partial_rounds_are_once_rounded_over_their_contributors(P, max_lag, dtype):
    cl = _cluster(P, max_lag)
    cases = direct_cases(cluster_knobs(P, max_lag), P, dtype)
    _planned(cl, P, dtype, cases)
    wide = _data(P, dtype, "wide")
    launches, rounds, partial = cl.comms[0].stats.threshold, 0, 0
    try:
        for slow in (P - 1, 0):  # the last rank; rank 0: the low mask bit and the first source missing
            cl.comms[0].set_straggler(slow, IDLE_US)
            for n, plan, slows in cases:  # consecutive rounds on one cluster: the lag rows cycle
                if slow not in slows:
                    continue
                for op, rescale, inplace in (("sum", False, False), ("avg", False, False), ("sum", True, False),
                                             ("avg", True, False), ("sum", False, True), ("avg", True, True)):
                    what = (f"P={P} max_lag={max_lag} {dtype} wide n={n} straggler {slow} {op}"
                            f"{' rescale' if rescale else ''}{' in place' if inplace else ''}")
                    counts = _run_round(cl, wide, n, plan, slow, op, rescale, inplace, what)
                    rounds += 1
                    partial += int(((counts > 0) & (counts < P)).any())
            if slow == P - 1:  # narrow data at one size
                n, plan, _ = cases[2]
                counts = _run_round(cl, _data(P, dtype, "narrow"), n, plan, slow, "sum", False, False,
                                    f"P={P} max_lag={max_lag} {dtype} narrow n={n} straggler {slow}")
                rounds += 1
                partial += int(((counts > 0) & (counts < P)).any())
    finally:
        cl.comms[0].set_straggler(-1, 0.0)
    assert cl.comms[0].stats.threshold - launches == rounds and rounds > max_lag + 1
    assert partial == rounds  # every round left the straggler out of a chunk somewhere


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_ranks_reduce_a_full_batch_with_a_partial_and_a_full_mask(dtype):
    """The 2-source instantiation of reduce_masked takes 8 packs per lane: a chunk of at least
    8 x 256 packs runs one full batch (nu == U). At the grid of the other clusters no chunk is
    that large, so this cluster's grid is 8."""
    P, max_lag = 2, 0
    cl = _cluster(P, max_lag, SMALL_GRID)
    n = full_batch_size(dtype)
    cases = direct_cases(cluster_knobs(P, max_lag, SMALL_GRID), P, dtype, [n])
    _planned(cl, P, dtype, cases)
    (_, plan, slows), = cases
    assert plan["chunk"] // (16 // es_of(dtype)) >= FULL_BATCH_PACKS and slows == [1, 0]
    data = _data(P, dtype, "wide")
    try:
        for slow in slows:
            cl.comms[0].set_straggler(slow, IDLE_US)
            for op, rescale, inplace in (("sum", False, False), ("avg", True, False), ("sum", False, True)):
                _run_round(cl, data, n, plan, slow, op, rescale, inplace,
                           f"full batch {dtype} n={n} straggler {slow} {op}{' in place' if inplace else ''}")
    finally:
        cl.comms[0].set_straggler(-1, 0.0)
    full = H.plan_threshold(cl.comms[0].knobs, n, es_of(dtype), P, 1.0, 1.0)
    assert (full["full"], full["oneshot"], full["chunk"]) == (1, 0, plan["chunk"])
    _run_round(cl, data, n, full, -1, "sum", False, False, f"full batch {dtype} n={n} thresholds 1.0", th=1.0)


# ------------------------------------------------------------------------------------------
# Non-finite values and the fp16 overflow of the sum in a round with a straggler.
# ------------------------------------------------------------------------------------------
PX, NX = 4, 4099


def _edge_positions(n, dtype, block):
    """As in tests/test_exact_numerics_gpu.py: index 0; the last element (in the ragged tail);
    the last element of a pack; the first element of a rank's block other than block 0."""
    pack = 16 // es_of(dtype)
    pos = [0, n - 1, 5 * pack - 1, 2 * block]
    assert len(set(pos)) == 4 and max(pos) < n
    return pos


@pytest.mark.parametrize("where", ["fast ranks", "straggler"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_values_show_where_they_were_summed_and_nowhere_else(dtype, where):
    """+inf, a NaN, +inf again and the pair 65504 + 16 (inf in fp16, by the tie) at the four
    positions: held by fast ranks they show at that element in every chunk that was summed;
    held by the straggler they show in the straggler's own block on the straggler alone. A
    given-up chunk is +0 whatever the straggler's block held."""
    slow = PX - 1
    cl = _cluster(PX, 0)
    (n, plan, _), = direct_cases(cluster_knobs(PX, 0), PX, dtype, [NX])
    _planned(cl, PX, dtype, [(n, plan, None)])
    block = plan["block"]
    pos = _edge_positions(n, dtype, block)
    xs = [x[:n].clone() for x in _data(PX, dtype, "wide").cpu]
    inf, nan = float("inf"), float("nan")
    # position -> {rank: value}; the pair's position is set on every rank (65504 + 16 + grid values
    # would not be exact in fp32)
    if where == "fast ranks":
        put = [{0: inf}, {1: nan}, {0: 65504.0, 1: 16.0, 2: 0.0, 3: 0.0}, {2: inf}]
    else:
        put = [{slow: inf}, {slow: nan}, {slow: 65504.0, 0: 16.0, 1: 0.0, 2: 0.0}, {slow: inf}]
    for i, vals in zip(pos, put):
        for k, v in vals.items():
            xs[k][i] = torch.tensor(v, dtype=torch.float16).to(dtype)
    gpu = [x.to(DEV) for x in xs]
    ins = [x.clone() for x in gpu]
    bufs = [torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV) for _ in range(PX)]
    th = partial_th(PX)
    try:
        cl.comms[0].set_straggler(slow, IDLE_US)
        ys, counts = cl.allreduce_threshold(ins, [b[:n] for b in bufs], th_reduce=th, th_complete=th)
        cl.check()
    finally:
        cl.comms[0].set_straggler(-1, 0.0)
    what = f"edge values on the {where} {dtype}"
    outs, found, ranges = _check_round(xs, gpu, ins, bufs, ys, counts, plan, slow, 1.0, False, {}, what)
    special = {i: set(k for k, v in vals.items() if v != 0.0) for i, vals in zip(pos, put)}
    for k, y in enumerate(outs):
        odd = (~y.isfinite()).nonzero().flatten().tolist()
        want = []
        for i in pos:
            (S,) = [S for (lo, hi), S in zip(ranges, found[k]) if lo <= i < hi]
            holders = special[i] & S
            if i == pos[2]:  # the pair overflows fp16 only where both halves were summed
                if dtype == torch.float16 and holders == special[i]:
                    want.append(i)
            elif holders:
                want.append(i)
        assert odd == sorted(want), f"{what} rank {k}: non-finite at {odd}, expected at {sorted(want)}"
        lo, hi = slow * block, n
        if k != slow:  # the straggler's block, given up: +0 although (on the straggler) it held an inf
            assert bool((_bits(y[lo:hi]) == 0).all()), f"{what} rank {k}: the given-up block is not +0"
            if where == "straggler":
                assert odd == [], f"{what} rank {k}: the straggler's values reached a fast rank"
        elif where == "straggler":
            assert odd == [pos[1]] and lo <= pos[1] < hi  # the last element: the one position in its own block
    if where == "fast ranks":  # they did arrive: the owners of blocks 0 and 2 always take their own chunks
        assert outs[0][pos[0]] == inf and outs[2][pos[3]] == inf
        assert outs[slow][pos[1]].isnan()  # and the straggler summed everyone into its own block


# ------------------------------------------------------------------------------------------
# The protocol plane: reference block ranges and maxChunkSize chunks, a causal straggler.
# ------------------------------------------------------------------------------------------
class _Gate:
    """A causal straggler (as in tests/test_plane_gpu.py): its fetch of round r waits until every
    other worker's sink has received round r, so its data arrives strictly after the others
    completed the round, whatever the host or device speed."""

    def __init__(self, others: int):
        self.others = others
        self.cv = threading.Condition()
        self.seen: dict[int, int] = {}

    def sink(self, it: int) -> None:
        with self.cv:
            self.seen[it] = self.seen.get(it, 0) + 1
            self.cv.notify_all()

    def wait(self, it: int) -> None:
        with self.cv:
            assert self.cv.wait_for(lambda: self.seen.get(it, 0) >= self.others, timeout=300), it


@pytest.mark.parametrize("chunk", PLANE_CHUNKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_plane_partial_rounds_are_once_rounded_over_their_contributors(dtype, chunk):
    """thReduce = thComplete = 2/3 at 3 workers: 250-element chunks put every 16-bit chunk but a
    block's first off the 16-byte grid (the element-wise reduce, copies and zero fill), 256 is
    the aligned twin. The contributor set of a chunk is whichever set of the reported size gives
    its bits (no two agree on 8 elements of this data: tests/test_partial_round.py)."""
    P, n, rounds, straggler = PLANE_P, PLANE_N, PLANE_ROUNDS, PLANE_P - 1
    cpu = [exact_inputs(P, n, dtype, "wide", seed=plane_seed(dtype, it)) for it in range(rounds)]
    gpu = [[x.to(DEV) for x in xs] for xs in cpu]
    torch.cuda.synchronize()
    gate = _Gate(P - 1)

    def source(k):
        def f(req):
            if k == straggler:
                gate.wait(req.iteration)
            return gpu[req.iteration][k]
        return f

    job = PlaneJob(P, n, max_chunk_size=chunk, th_reduce=2.0 / 3.0, th_complete=2.0 / 3.0, max_lag=1,
                   max_round=rounds - 1, dtype=dtype, sources=[source(k) for k in range(P)], timeout_s=60.0,
                   on_output=lambda k, out: gate.sink(out.iteration) if k != straggler else None)
    try:
        job.run(timeout=120)
        nch = job.planes[0].chunks
        lay = C.BlockLayout(n, P, chunk)
        assert nch == max(lay.num_chunks(j) for j in range(P))
        ranges = plane_ranges(n, P, chunk, nch)
        below = 0
        for k in range(P):
            st = job.system.plane_worker_state(job.workers[k])
            assert st["stats"]["plane_errors"] == 0 and st["stats"]["rounds_completed"] == rounds, st
            for it in range(rounds):
                data, counts = job.outputs[k][it]
                assert data.dtype == dtype and data.numel() == n and len(counts) == P * nch
                check_partial_round(cpu[it], data, counts, ranges, dtype,
                                    what=f"plane {dtype} chunk {chunk} worker {k} round {it} (counts {counts})")
                below += sum(1 for c, (lo, hi) in zip(counts, ranges) if hi > lo and c < P)
                assert torch.equal(gpu[it][k].cpu(), cpu[it][k]), f"worker {k} round {it}: the source was written"
            if k != straggler:  # round 0: its own block reduced from the two fast workers
                own = job.outputs[k][0][1][k * nch:k * nch + lay.num_chunks(k)]
                assert own == [P - 1] * lay.num_chunks(k), (k, own)
        assert below > 0  # else no round was partial at all
    finally:
        job.shutdown()
