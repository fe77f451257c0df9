""""fp32 accumulation, one rounding", bit for bit, in every reducing kernel of the data plane.

The inputs come from akka_allreduce_1_amd/utils/exact_data.py: multiples of 2^-10 whose sum is
exact in fp32 in EVERY order (tests/test_exact_data.py), so each kernel - whatever order it
sums in - must return the one round-to-nearest-even of that sum, and every comparison here is
`torch.equal` against `exact_sum` and nothing else. A kernel that rounds a partial sum to the
element type, truncates, multiplies by its scale anywhere but on the fp32 sum, or reads a stale
contribution differs in hundreds of elements of the `wide` data (12-33 % of its results are
inexact, most of those exact ties); `ring_native`, which rounds at every hop by design, is held
to `narrow` data (every partial sum representable), to its error bound on `wide` data, and to
NOT equalling the once-rounded result there.

All in one process on one GPU: LocalCluster / LocalSdmaCluster, one cluster per (P, max_lag),
256 KiB slots so that the largest size spans several launches.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from akka_allreduce_1_amd._native import C  # noqa: E402
from akka_allreduce_1_amd.ops.kernels import dtype_code  # noqa: E402
from akka_allreduce_1_amd.parallel import LocalCluster, LocalSdmaCluster  # noqa: E402
from akka_allreduce_1_amd.parallel.comm import ALGOS  # noqa: E402
from akka_allreduce_1_amd.utils.exact_data import exact_inputs, exact_sum, per_hop_bound  # noqa: E402

H = C.hip
DEV = torch.device("cuda", 0)
SLOT = 256 << 10
GRID = 64
NMAX = 300_000  # the largest size: several segments at 256 KiB slots (2 ranks: 3 two-shot launches of bf16)
GUARD = 64      # sentinel elements behind every out-of-place output
SENTINEL = -7.0
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
WORLDS = [2, 3, 4, 8]

_CLUSTERS: dict = {}
_SDMA: dict = {}
_DATA: dict = {}


def _cluster(P, max_lag=None):
    key = (P, max_lag)
    if key not in _CLUSTERS:
        _CLUSTERS[key] = LocalCluster(P, slot_bytes=SLOT, grid=GRID, timeout_s=10, max_lag=max_lag)
    return _CLUSTERS[key]


def _sdma(P):
    if P not in _SDMA:
        _SDMA[P] = LocalSdmaCluster(P, slot_bytes=SLOT, grid=8)
    return _SDMA[P]


def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


class _Data:
    """The NMAX-element rank tensors of (P, dtype, mode), made once on the CPU and copied to the
    GPU, never written; a case works on clones of a prefix. The expected result is elementwise,
    so the prefix of the expectation is the expectation of the prefix."""

    def __init__(self, P, dtype, mode):
        self.cpu = exact_inputs(P, NMAX, dtype, mode, seed=1000 * P + 10 * _es(dtype) + len(mode))
        self.xs = [x.to(DEV) for x in self.cpu]
        self.dtype = dtype
        self._want: dict = {}

    def want(self, scale=1.0, dtype=None):
        key = (scale, dtype)
        if key not in self._want:
            self._want[key] = exact_sum(self.cpu, dtype or self.dtype, scale).to(DEV)
        return self._want[key]

    def inputs(self, n):
        return [x[:n].clone() for x in self.xs]


def _data(P, dtype, mode):
    key = (P, dtype, mode)
    if key not in _DATA:
        _DATA[key] = _Data(P, dtype, mode)
    return _DATA[key]


def _same(got, want):
    """Bit-equal, NaN where and only where the expectation is NaN."""
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(got[~nan], want[~nan])


def _report(got, want, xs, lo=0):
    """Where a result differs: a stale read, a missing contribution and a wrong rounding look
    different here."""
    bad = ((got != want) & ~(got.isnan() & want.isnan())).nonzero().flatten()
    if bad.numel() == 0:
        return "no differing element"
    i = int(bad[0])
    ins = [float(x[lo + i]) for x in xs]
    return (f"{bad.numel()} of {got.numel()} elements differ, first {i} last {int(bad[-1])}: got "
            f"{float(got[i])!r} want {float(want[i])!r}, inputs at {lo + i}: {ins}")


def _expect(got, want, xs, what, lo=0):
    if not _same(got, want):
        pytest.fail(f"{what}: {_report(got, want, xs, lo)}")


def _guarded(n, dtype):
    """An output of n elements with GUARD sentinel elements behind it (16-byte aligned start)."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _guard_intact(buf, n, what):
    assert bool((buf[n:] == SENTINEL).all()), f"{what}: wrote past the end of the output"


def _around(limit_bytes, es):
    """Element counts just below, at and just above a byte limit."""
    n = limit_bytes // es
    return [n - 1, n, n + 1]


def _base_sizes(dtype):
    pack = 16 // _es(dtype)
    # 1, 7: less than one pack (bf16 / fp16), every block but the first empty; one pack +- 1;
    # 4099: ragged tail and a short last block; 65536 + 3; NMAX: several segments
    return [1, 7, pack - 1, pack, pack + 1, 4099, 65536 + 3, NMAX]


def _sizes(algo, P, dtype, comm):
    es = _es(dtype)
    ns = _base_sizes(dtype)
    if algo == "oneshot":
        # the one-shot limit: up to one slot the one-shot body, past it the two-shot kernel (resolve)
        ns += _around(comm.slot_bytes, es)
    elif algo == "ll":
        # ll_max_bytes: up to it one low-latency launch, past it a second segment
        ns += _around(comm.ll_max_bytes, es)
    elif algo == "auto":
        # ll_auto_max_bytes: the low-latency kernel up to it, then one-shot / two-shot
        ns += _around(comm.ll_auto_max_bytes, es)
        # oneshot_max_bytes: the one-shot body up to it, the two-shot past it (when the
        # low-latency limit lies below; see the second pass of the auto case)
        ns += _around(comm.oneshot_max_bytes, es)
    elif algo in ("twoshot", "ring_native"):
        # world x slot: one launch up to it, a second segment past it
        ns += _around(P * comm.slot_bytes, es)
    elif algo == "ring":
        # the ring's slots carry fp32 partials: a segment is world x slot / 4 elements
        ns += _around(P * comm.slot_bytes // 4 * es, es)
    return sorted({n for n in ns if 1 <= n <= NMAX})


def _run_allreduce(cl, algo, data, n, op, inplace, what):
    P = cl.world
    want = data.want(1.0 / P if op == "avg" else 1.0)[:n]
    ins = data.inputs(n)
    if inplace:
        outs = cl.allreduce(ins, ins, algo=algo, op=op)
        cl.check()
    else:
        bufs = [_guarded(n, data.dtype) for _ in range(P)]
        outs = cl.allreduce(ins, [o for _, o in bufs], algo=algo, op=op)
        cl.check()
        for r, (buf, _) in enumerate(bufs):
            _guard_intact(buf, n, f"{what} rank {r}")
            assert torch.equal(ins[r], data.xs[r][:n]), f"{what} rank {r}: the input was written"
    for r, y in enumerate(outs):
        _expect(y, want, data.xs, f"{what} rank {r}")


def _allreduce_case(algo, P, dtype, sizes=None):
    cl = _cluster(P)
    ops = ["sum", "avg"] if P in (3, 4) else ["sum"]
    for mode in ("wide", "narrow"):
        data = _data(P, dtype, mode)
        for n in sizes or _sizes(algo, P, dtype, cl.comms[0]):
            for op in ops:
                for inplace in (False, True):
                    _run_allreduce(cl, algo, data, n, op, inplace,
                                   f"{algo} P={P} {dtype} {mode} n={n} {op} {'in place' if inplace else 'out of place'}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
@pytest.mark.parametrize("algo", ["twoshot", "oneshot", "ring", "ll"])
def test_allreduce_is_once_rounded(algo, P, dtype):
    cl = _cluster(P)
    st0 = cl.comms[0].stats
    before = (st0.twoshot, st0.oneshot, st0.ring, st0.ll)
    _allreduce_case(algo, P, dtype)
    st = cl.comms[0].stats
    ran = [b - a for a, b in zip(before, (st.twoshot, st.oneshot, st.ring, st.ll))]
    # the kernel asked for ran (and, past the one-shot limit, the two-shot it falls back to)
    assert ran[["twoshot", "oneshot", "ring", "ll"].index(algo)] > 0, ran
    assert all(c == 0 for k, c in zip(["twoshot", "oneshot", "ring", "ll"], ran)
               if k != algo and not (algo == "oneshot" and k == "twoshot")), ran
    if algo == "oneshot":
        assert ran[0] > 0, ran


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_auto_allreduce_is_once_rounded(P, dtype):
    """The size policy: every kernel it picks returns the same bits. The cluster's slots (256 KiB)
    put its one-shot limit at or below its low-latency limit, so a second pass lowers the
    low-latency limit to 64 KiB and walks low-latency -> one-shot -> two-shot."""
    cl = _cluster(P)
    code, es = dtype_code(dtype), _es(dtype)
    _allreduce_case("auto", P, dtype)
    c0 = cl.comms[0]
    saved = [c.ll_auto_max_bytes for c in cl.comms]
    try:
        for c in cl.comms:
            c.ll_auto_max_bytes = 64 << 10
        # 64 KiB: the low-latency kernel at and below, the one-shot body above;
        # oneshot_max_bytes: the one-shot body at and below, the two-shot kernel above
        sizes = _around(64 << 10, es) + _around(c0.oneshot_max_bytes, es)
        picked = [c0.resolve(n, code, H.Algo.Auto) for n in sizes]
        assert picked == [H.Algo.LL, H.Algo.LL, H.Algo.OneShot, H.Algo.OneShot, H.Algo.OneShot, H.Algo.TwoShot], picked
        _allreduce_case("auto", P, dtype, sizes)
    finally:
        for c, v in zip(cl.comms, saved):
            c.ll_auto_max_bytes = v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_ring_native_rounds_at_every_hop_and_nowhere_else(P, dtype):
    """`ring_native` carries its partial sums in the element type: bit-exact where they are
    representable (narrow data, fp32), within (P - 1) half-ulps of the largest partial sum of the
    exact sum on wide bf16 / fp16 data - and, from 3 ranks on, NOT the once-rounded result there:
    the bench headline must not count it among the once-rounded kernels."""
    cl = _cluster(P)
    sizes = _sizes("ring_native", P, dtype, cl.comms[0])
    narrow = _data(P, dtype, "narrow")
    for n in sizes:
        for inplace in (False, True):
            _run_allreduce(cl, "ring_native", narrow, n, "sum", inplace, f"ring_native P={P} {dtype} narrow n={n}")
    wide = _data(P, dtype, "wide")
    if dtype == torch.float32:
        for n in sizes:
            _run_allreduce(cl, "ring_native", wide, n, "sum", False, f"ring_native P={P} fp32 wide n={n}")
        return
    exact = wide.want(dtype=torch.float64)
    bound = per_hop_bound(wide.cpu, dtype).to(DEV)
    for n in sizes:
        ys = cl.allreduce(wide.inputs(n), algo="ring_native")
        cl.check()
        for r, y in enumerate(ys):
            over = ((y.double() - exact[:n]).abs() > bound[:n]).nonzero().flatten()
            assert over.numel() == 0, (f"rank {r} n={n}: {over.numel()} elements beyond (P - 1) half-ulps, first "
                                       f"{int(over[0])}: got {float(y[int(over[0])])!r} exact {float(exact[int(over[0])])!r}")
            assert torch.equal(y, ys[0]), f"rank {r} n={n}: ranks disagree"
        if P >= 3 and n >= 4099:
            assert not torch.equal(ys[0], wide.want()[:n]), f"n={n}: ring_native equals the once-rounded result"


def _threshold_switch(knobs, P, es):
    """The largest n (a multiple of 64) whose full-threshold round takes the one-shot body of the
    threshold kernel, from the launch planner for this cluster's knobs (th_oneshot_max, and the
    LL-encoded round must fit one slot), and the next multiple of 64, which takes the two-shot body."""
    def oneshot(n):
        return H.plan_threshold(knobs, n, es, P, 1.0, 1.0)["oneshot"]

    lo, hi = 1, knobs.th_oneshot_max // es // 64 + 1  # in units of 64 elements
    assert oneshot(64 * lo) == 1 and oneshot(64 * hi) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if oneshot(64 * mid):
            lo = mid
        else:
            hi = mid
    return 64 * lo, 64 * hi


def _full_counts(cl, n, dtype):
    """counts[rank, block, chunk] of a round every contribution arrived in: P for every chunk
    that exists, 0 past the end of the data (a short or empty last block), on every rank."""
    P = cl.world
    p = H.plan_threshold(cl.comms[0].knobs, n, _es(dtype), P, 1.0, 1.0)
    first = (torch.arange(P).view(P, 1) * p["block"] + torch.arange(p["nch"]).view(1, p["nch"]) * p["chunk"])
    inside = (first < n) & (torch.arange(p["nch"]).view(1, p["nch"]) * p["chunk"] < p["block"])
    return (inside.to(torch.int32) * P).expand(P, P, p["nch"]).contiguous().to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("max_lag", [0, 2])
@pytest.mark.parametrize("P", WORLDS)
def test_threshold_round_at_full_thresholds_is_once_rounded(P, max_lag, dtype):
    cl = _cluster(P, max_lag)
    es = _es(dtype)
    below, above = _threshold_switch(cl.comms[0].knobs, P, es)
    # below / above: the one-shot body limit of the threshold kernel (th_oneshot_max, or half a
    # slot where that is less: the round's LL words must fit one); a round is one launch, so
    # sizes stop at world x slot
    sizes = [n for n in _base_sizes(dtype)[:-1] + [below, above] if n * es <= P * cl.comms[0].slot_bytes]
    assert len(sizes) >= 4  # more rounds than lag-ring rows: the rows cycle
    launches = cl.comms[0].stats.threshold
    for mode in ("wide", "narrow"):
        data = _data(P, dtype, mode)
        for op in (["sum", "avg"] if P in (3, 4) else ["sum"]):
            want = data.want(1.0 / P if op == "avg" else 1.0)
            for n in sizes:  # consecutive rounds
                ins = data.inputs(n)
                bufs = [_guarded(n, dtype) for _ in range(P)]
                ys, counts = cl.allreduce_threshold(ins, [o for _, o in bufs], th_reduce=1.0, th_complete=1.0, op=op)
                cl.check()
                what = f"threshold P={P} max_lag={max_lag} {dtype} {mode} n={n} {op}"
                assert torch.equal(counts, _full_counts(cl, n, dtype)), f"{what}: counts {counts.unique().tolist()}"
                for r, y in enumerate(ys):
                    _expect(y, want[:n], data.xs, f"{what} rank {r}")
                    _guard_intact(bufs[r][0], n, f"{what} rank {r}")
            ins = data.inputs(4099)  # and in place
            cl.allreduce_threshold(ins, ins, op=op, counts=False)
            cl.check()
            for r, y in enumerate(ins):
                _expect(y, want[:4099], data.xs, f"threshold in place P={P} {dtype} {mode} rank {r}")
    assert cl.comms[0].stats.threshold > launches


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_reduce_scatter_is_once_rounded(P, dtype):
    cl = _cluster(P)
    pack = 16 // _es(dtype)
    # per-rank blocks of whole 16-byte packs: one pack, three, 1032 elements, 16 Ki + a pack,
    # and the largest the data holds (2 ranks of bf16: more than a slot per block, two segments)
    for m in (pack, 3 * pack, 1032, 16384 + pack, NMAX // P // pack * pack):
        n = P * m
        for mode in ("wide", "narrow"):
            data = _data(P, dtype, mode)
            for scale in (1.0, 0.5):
                want = data.want(scale)
                ins = data.inputs(n)
                bufs = [_guarded(m, dtype) for _ in range(P)]
                ys = cl.collective("reduce_scatter", ins, [o for _, o in bufs], scale=scale)
                cl.check()
                for r, y in enumerate(ys):
                    what = f"reduce_scatter P={P} {dtype} {mode} m={m} scale={scale} rank {r}"
                    _expect(y, want[r * m:(r + 1) * m], data.xs, what, lo=r * m)
                    _guard_intact(bufs[r][0], m, what)


def _reduce_to_root(cl, ins, root, scale, dtype):
    """Every rank passes an output; off the root it is ignored and keeps its sentinel."""
    n = ins[0].numel()
    outs = [torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV) for _ in range(cl.world)]
    H.XgmiComm.reduce_local(cl.comms, [x.data_ptr() for x in ins], [o.data_ptr() for o in outs], n, dtype_code(dtype),
                            root, torch.cuda.current_stream(DEV).cuda_stream, scale)
    cl.check()
    for r, o in enumerate(outs):
        if r != root:
            assert bool((o == SENTINEL).all()), f"reduce to {root}: rank {r}'s buffer was written"
    _guard_intact(outs[root], n, f"reduce to {root}")
    return outs[root][:n]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_reduce_to_a_root_is_once_rounded(P, dtype):
    cl = _cluster(P)
    for mode in ("wide", "narrow"):
        data = _data(P, dtype, mode)
        for n in _base_sizes(dtype):
            ins = data.inputs(n)
            for root in (0, P - 1):
                for scale in (1.0, 0.5):
                    y = _reduce_to_root(cl, ins, root, scale, dtype)
                    _expect(y, data.want(scale)[:n], data.xs, f"reduce P={P} root={root} {dtype} {mode} n={n} scale={scale}")
            for r in range(P):
                assert torch.equal(ins[r], data.xs[r][:n]), f"reduce n={n}: rank {r}'s input was written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [2, 4])
def test_sdma_allreduce_is_once_rounded(P, dtype):
    cl = _sdma(P)
    for mode in ("wide", "narrow"):
        data = _data(P, dtype, mode)
        for n in _base_sizes(dtype):
            for op in ("sum", "avg"):
                want = data.want(1.0 / P if op == "avg" else 1.0)[:n]
                for inplace in (False, True):
                    ins = data.inputs(n)
                    bufs = [_guarded(n, dtype) for _ in range(P)]
                    ys = cl.allreduce(ins, ins if inplace else [o for _, o in bufs], op=op)
                    torch.cuda.synchronize()
                    cl.check()
                    for r, y in enumerate(ys):
                        what = f"sdma P={P} {dtype} {mode} n={n} {op} {'in place' if inplace else 'out of place'} rank {r}"
                        _expect(y, want, data.xs, what)
                        _guard_intact(bufs[r][0], n, what)


# ------------------------------------------------------------------------------------------
# Non-finite values, fp16 overflow of the sum and fp16 subnormals through every entry above, at
# 4 ranks and 4099 elements (reduce_scatter: 4 x 1032, its blocks are whole packs).
# ------------------------------------------------------------------------------------------
PX = 4
ENTRIES = ["twoshot", "oneshot", "ring", "ll", "auto", "ring_native", "threshold_lag0", "threshold_lag2",
           "reduce_scatter", "reduce_root0", "reduce_last_root", "sdma"]


def _entry_n(entry):
    return 4 * 1032 if entry == "reduce_scatter" else 4099


def _run_entry(entry, ins, dtype):
    """Run `entry` on the 4 rank tensors; returns [(rank, output, lo, hi)]: output must equal
    expectation[lo:hi]."""
    n = ins[0].numel()
    if entry in ALGOS:
        cl = _cluster(PX)
        ys = cl.allreduce(ins, algo=entry)
        cl.check()
        return [(r, y, 0, n) for r, y in enumerate(ys)]
    if entry.startswith("threshold"):
        cl = _cluster(PX, int(entry[-1]))
        ys, counts = cl.allreduce_threshold(ins, th_reduce=1.0, th_complete=1.0)
        cl.check()
        assert torch.equal(counts, _full_counts(cl, n, dtype)), counts.unique().tolist()
        return [(r, y, 0, n) for r, y in enumerate(ys)]
    if entry == "reduce_scatter":
        cl = _cluster(PX)
        m = n // PX
        ys = cl.collective("reduce_scatter", ins)
        cl.check()
        return [(r, y, r * m, (r + 1) * m) for r, y in enumerate(ys)]
    if entry.startswith("reduce"):
        root = 0 if entry == "reduce_root0" else PX - 1
        return [(root, _reduce_to_root(_cluster(PX), ins, root, 1.0, dtype), 0, n)]
    cl = _sdma(PX)
    ys = cl.allreduce(ins)
    torch.cuda.synchronize()
    cl.check()
    return [(r, y, 0, n) for r, y in enumerate(ys)]


def _check_entry(entry, cpu_xs, dtype, what):
    want = exact_sum(cpu_xs, dtype).to(DEV)
    ins = [x.to(DEV) for x in cpu_xs]
    for r, y, lo, hi in _run_entry(entry, [x.clone() for x in ins], dtype):
        w = want[lo:hi]
        assert torch.equal(y.isnan(), w.isnan()) and torch.equal(y.isinf(), w.isinf()), \
            f"{entry} {dtype} {what} rank {r}: NaN / inf where none belongs, or none where one does: {_report(y, w, ins, lo)}"
        _expect(y, w, ins, f"{entry} {dtype} {what} rank {r}", lo)
    return want


def _narrow_base(dtype, n):
    return [x[:n].clone() for x in _data(PX, dtype, "narrow").cpu]


def _edge_positions(n, dtype, block):
    """Index 0; the last element (in the ragged tail); the last element of a pack; the first
    element of a rank's block other than block 0."""
    pack = 16 // _es(dtype)
    pos = [0, n - 1, 5 * pack - 1, 2 * block]
    assert len(set(pos)) == 4 and max(pos) < n
    return pos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["+inf", "-inf", "nan", "+inf and -inf"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_non_finite_values_arrive_everywhere_and_spread_nowhere(entry, kind, dtype):
    """An inf or NaN in ONE rank's gradient (fp16 loss scaling relies on it) shows on every rank,
    at that element only; +inf on one rank and -inf on another give NaN."""
    n = _entry_n(entry)
    block = n // PX if entry == "reduce_scatter" else _cluster(PX).comms[0].block_elems(n, dtype_code(dtype))
    xs = _narrow_base(dtype, n)
    inf, nan = float("inf"), float("nan")
    pos = _edge_positions(n, dtype, block)
    for j, i in enumerate(pos):  # a different rank at each position
        xs[j % PX][i] = {"+inf": inf, "-inf": -inf, "nan": nan, "+inf and -inf": inf}[kind]
        if kind == "+inf and -inf":
            xs[(j + 1) % PX][i] = -inf
    want = _check_entry(entry, xs, dtype, kind)
    # the expectation itself: non-finite at the four positions and nowhere else
    special = (want.isnan() if kind in ("nan", "+inf and -inf") else want.isinf()).nonzero().flatten().tolist()
    assert special == sorted(pos) and int((~want.isfinite()).sum()) == 4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_fp16_overflow_of_the_sum(entry, dtype):
    """Finite inputs whose sum passes 65504: 65504 + 16 = 65520 is the tie round-to-nearest-even
    sends to inf; 65504 + 15.9921875 stays 65504; 4 x 32768 is inf. The same values taken to
    bf16 and fp32 stay finite and exact."""
    n = _entry_n(entry)
    xs = _narrow_base(dtype, n)
    at = [100, 2000, 4000]
    vals = [[65504.0, 16.0, 0.0, 0.0], [65504.0, 15.9921875, 0.0, 0.0], [32768.0] * 4]
    for i, v in zip(at, vals):
        for k in range(PX):
            xs[k][i] = torch.tensor(v[k], dtype=torch.float16).to(dtype)
    want = _check_entry(entry, xs, dtype, "overflow")
    w = want[at].cpu()
    if dtype == torch.float16:
        assert w.tolist() == [float("inf"), 65504.0, float("inf")]
    else:  # bf16 holds 65504 as 65536 and 15.9921875 as 16
        assert w.tolist() == ([65520.0, 65519.9921875, 131072.0] if dtype == torch.float32 else [65536.0, 65536.0, 131072.0])
    assert int((~want.isfinite()).sum()) == (2 if dtype == torch.float16 else 0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_fp16_subnormals_are_summed_and_rounded_correctly(entry):
    """fp16 subnormal inputs are multiples of 2^-24: normal numbers in fp32, so the sum is exact
    and the output is its correctly rounded fp16 value, subnormal results included. (fp32 and
    bf16 subnormals follow the denormal mode; the project makes no promise about them.)"""
    n = _entry_n(entry)
    mode = "narrow" if entry == "ring_native" else "wide"  # |m| < 2^8: every partial sum an exact subnormal
    xs = exact_inputs(PX, n, torch.float16, mode, seed=24, grid_exp=24)
    tiny = torch.finfo(torch.float16).tiny
    assert all(bool(((x != 0) & (x.abs() < tiny)).any()) for x in xs)
    want = _check_entry(entry, xs, torch.float16, "subnormal")
    assert bool(((want != 0) & (want.abs() < tiny)).any())
    if mode == "wide":  # some results are rounded: not every sum is an fp16 value
        assert not torch.equal(want.double(), exact_sum(xs, torch.float64).to(DEV))
