"""`check_partial_round` (akka_allreduce_1_amd/utils/exact_data.py) on the CPU, and the case table
of tests/test_threshold_partial_gpu.py walked through the launch planner alone.

The checker is what the GPU file's partial threshold rounds are held to, so this file shows that
it accepts the output a correct round would give and REJECTS the wrong kernels it is there to
catch - a sum rounded at every hop, a truncated one, a coefficient applied to the inputs or
taken as `scale` where `scale * P / count` is due, a stale contribution, a contributor set of
the wrong size, a -0 or a leftover sentinel in a given-up chunk, a chunk boundary off by one -
each with a message that names the chunk. It also states what makes "any set of the reported
size" a real check: on the data the GPU file uses, no two contributor sets of one size agree on
8 consecutive elements.

The helpers without a `test_` prefix (cluster_knobs, direct_cases, ...) are the GPU file's case
table: it imports them, so both files walk the same cases.
"""
import itertools
import re

import pytest
import torch

from akka_allreduce_1_amd._native import C
from akka_allreduce_1_amd.utils.exact_data import (PartialRoundError, check_partial_round, chunk_ranges,
                                                   exact_inputs, exact_sum, partial_coef, per_hop_sum, truncated_sum)

H = C.hip
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
WORLDS = [2, 3, 4, 8]
LAGS = [0, 2]
SLOT = 256 << 10   # bytes per slot of the GPU file's clusters
GRID = 64
SMALL_GRID = 8     # the 2-rank cluster whose chunks hold a full batch of the 2-source reduce
NMAX = 300_000
FULL_BATCH_PACKS = 8 * 256  # 8 packs per lane x 256 lanes: one full batch of the 2-source instantiation
PLANE_P, PLANE_N, PLANE_ROUNDS = 3, 3001, 3
PLANE_CHUNKS = [250, 256]  # 16-bit chunks of 500 B (no 16-byte multiple: element-wise paths) and the aligned twin


def es_of(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def cluster_knobs(P, max_lag, grid=GRID):
    """The GridKnobs of LocalCluster(P, slot_bytes=SLOT, grid=grid, max_lag=max_lag) on an MI355X
    (256 CUs: default grid 512), from the slab layout alone."""
    L = H.slab_layout(P, SLOT, max_lag + 1)
    k = H.GridKnobs()
    k.world, k.rows, k.grid, k.default_grid = P, max_lag + 2, grid, 512
    k.maxch, k.slot_bytes = L["maxch"], L["slot_bytes"]
    return k


def partial_th(P):
    return (P - 1) / P


def base_sizes(dtype):
    pack = 16 // es_of(dtype)
    # 7: less than a pack of a 16-bit type (only the scalar tail of the reduce runs), every block
    # but the first empty; two tiny blocks; a ragged tail and a short last block; chunks of about
    # 1030 elements (partial batches); the largest size of the exact-numerics file
    return [7, pack + 1, 4099, 65536 + 3, NMAX]


def chunks_per_block(plan, n, P):
    """Chunks that exist in each block."""
    out = []
    for j in range(P):
        bl = max(0, min(plan["block"], n - j * plan["block"]))
        out.append(-(-bl // plan["chunk"]))
    return out


def direct_cases(knobs, P, dtype, sizes=None):
    """[(n, plan, stragglers)] of one (P, dtype) of the GPU file's direct rounds: every size the
    planner accepts in one launch, with the stragglers (last rank, rank 0) under which the fast
    ranks can complete the round from the chunks outside the straggler's block."""
    es, th = es_of(dtype), partial_th(P)
    cases = []
    for n in sizes or base_sizes(dtype):
        if n * es > P * knobs.slot_bytes:
            continue
        try:
            plan = H.plan_threshold(knobs, n, es, P, th, th)
        except ValueError:
            continue
        per = chunks_per_block(plan, n, P)
        slows = [s for s in (P - 1, 0) if plan["min_complete"] <= sum(per) - per[s]]
        cases.append((n, plan, slows))
    return cases


def full_batch_size(dtype):
    """The largest ragged size one launch of the 2-rank cluster carries."""
    return 2 * SLOT // es_of(dtype) - 3


def direct_seed(P, dtype, mode):
    return 7000 + 100 * P + 10 * es_of(dtype) + len(mode)


def plane_seed(dtype, it):
    return 9000 + 10 * es_of(dtype) + it


def plane_ranges(n, P, chunk, nch):
    """(lo, hi) of chunk c of block j at j * nch + c, from the reference's block ranges."""
    lay = C.BlockLayout(n, P, chunk)
    out = []
    for j in range(P):
        for c in range(nch):
            lo = min(lay.end[j], lay.start[j] + c * chunk)
            out.append((lo, min(lay.end[j], lo + chunk)))
    return out


# ------------------------------------------------------------------------------------------
# A synthetic round: 4 ranks, 4099 elements, rank 3 the straggler, the geometry the planner
# gives the GPU file's cluster.
# ------------------------------------------------------------------------------------------
P0, N0, SLOW0 = 4, 4099, 3
FAST0 = frozenset(range(P0)) - {SLOW0}
ALLOWED0 = {P0: [frozenset(range(P0))], P0 - 1: [FAST0]}


def _geometry(dtype):
    p = H.plan_threshold(cluster_knobs(P0, 0), N0, es_of(dtype), P0, partial_th(P0), partial_th(P0))
    assert p["nch"] >= 2 and chunks_per_block(p, N0, P0)[P0 - 1] < p["nch"]  # several chunks, a short last block
    return p["block"], p["chunk"], p["nch"]


def _counts(geo, rank, given_up=()):
    """What rank `rank` reports: the straggler's block complete on the straggler and given up
    elsewhere, the fast blocks without the straggler; `given_up`: fast (block, chunk) it left out."""
    block, chunk, nch = geo
    ranges = chunk_ranges(N0, P0, block, chunk, nch)
    cnt = []
    for j in range(P0):
        for c in range(nch):
            lo, hi = ranges[j * nch + c]
            v = 0 if hi <= lo else (P0 if rank == SLOW0 else 0) if j == SLOW0 else P0 - 1
            cnt.append(0 if (j, c) in given_up else v)
    return cnt


def _sets(counts):
    return [frozenset() if c == 0 else frozenset(range(P0)) if c == P0 else FAST0 for c in counts]


def _assemble(xs, geo, counts, sets, dtype, scale=1.0, rescale=False, sum_fn=None):
    block, chunk, nch = geo
    out = torch.full((N0,), -7.0, dtype=dtype)
    for (lo, hi), c, S in zip(chunk_ranges(N0, P0, block, chunk, nch), counts, sets):
        if hi <= lo:
            continue
        if not S:
            out[lo:hi] = 0
        else:
            sub = [xs[k] for k in sorted(S)]
            coef = partial_coef(scale, P0, c, rescale)
            out[lo:hi] = (sum_fn(sub, coef) if sum_fn else exact_sum(sub, dtype, coef))[lo:hi]
    return out


def _xs(dtype, seed=5):
    return exact_inputs(P0, N0, dtype, "wide", seed=seed)


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("scale", [1.0, 1.0 / P0])
@pytest.mark.parametrize("rank", [0, SLOW0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_accepts_a_correct_partial_round(dtype, rank, scale, rescale):
    xs, geo = _xs(dtype), _geometry(dtype)
    counts = _counts(geo, rank, given_up=[(1, 1)] if rank == 0 else [])
    out = _assemble(xs, geo, counts, _sets(counts), dtype, scale, rescale)
    for allowed in (ALLOWED0, None):
        found = check_partial_round(xs, out, counts, geo, dtype, scale, rescale, allowed=allowed)
        assert found == _sets(counts)
    # the same through explicit ranges, counts given as a [P][nch] tensor
    ranges = chunk_ranges(N0, P0, *geo)
    found = check_partial_round(xs, out, torch.tensor(counts).view(P0, -1), ranges, dtype, scale, rescale)
    assert found == _sets(counts)
    assert 0 in counts and (P0 - 1 in counts or P0 in counts)


def _rejects(xs, out, counts, geo, dtype, chunk_name, count, scale=1.0, rescale=False, allowed=ALLOWED0, also=()):
    with pytest.raises(PartialRoundError) as e:
        check_partial_round(xs, out, counts, geo, dtype, scale, rescale, allowed=allowed, what="mutant")
    msg = str(e.value)
    print(msg)
    assert msg.startswith("mutant: ") and chunk_name in msg and f"count {count}" in msg, msg
    for pattern in also:
        assert re.search(pattern, msg), (pattern, msg)
    return msg


def _mutate_chunk(good, wrong, geo, j, c):
    lo, hi = chunk_ranges(N0, P0, *geo)[j * geo[2] + c]
    assert hi > lo and not torch.equal(good[lo:hi], wrong[lo:hi]), "the mutant does not differ in this chunk"
    out = good.clone()
    out[lo:hi] = wrong[lo:hi]
    return out


@pytest.mark.parametrize("mutant", ["per_hop", "truncated"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_checker_rejects_a_wrong_rounding(dtype, mutant):
    xs, geo = _xs(dtype), _geometry(dtype)
    counts = _counts(geo, 0)
    good = _assemble(xs, geo, counts, _sets(counts), dtype)
    fn = per_hop_sum if mutant == "per_hop" else truncated_sum
    wrong = _assemble(xs, geo, counts, _sets(counts), dtype, sum_fn=lambda sub, coef: fn(sub, dtype))
    out = _mutate_chunk(good, wrong, geo, 1, 1)  # ONE chunk of a fast block: the message must name it
    _rejects(xs, out, counts, geo, dtype, "block 1 chunk 1", P0 - 1, also=[r"first \d+: got \S+ want \S+",
                                                                            "no contributor set of any size"])
    _rejects(xs, out, counts, geo, dtype, "block 1 chunk 1", P0 - 1, allowed=None)


def test_checker_rejects_the_coefficient_applied_to_the_inputs():
    """The mean over 3 contributors as the fp32 sum of (x * coef) instead of (sum of x) * coef.
    The two differ in the last bits of the fp32 value: an fp32 output shows them in a third of
    its elements, a 16-bit output almost never (its rounding hides them), so fp32 is the type
    that pins where the coefficient is applied."""
    dtype = torch.float32
    xs, geo = _xs(dtype), _geometry(dtype)
    counts = _counts(geo, 0)

    def scaled_inputs(sub, coef):
        acc = torch.zeros(N0, dtype=torch.float32)
        for x in sub:
            acc = acc + x.float() * torch.tensor(coef, dtype=torch.float32)
        return acc.to(dtype)

    good = _assemble(xs, geo, counts, _sets(counts), dtype, 1.0 / P0, True)
    wrong = _assemble(xs, geo, counts, _sets(counts), dtype, 1.0 / P0, True, sum_fn=scaled_inputs)
    out = _mutate_chunk(good, wrong, geo, 0, 0)
    _rejects(xs, out, counts, geo, dtype, "block 0 chunk 0", P0 - 1, 1.0 / P0, True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_scale_where_the_rescaled_coefficient_is_due(dtype):
    xs, geo = _xs(dtype), _geometry(dtype)
    counts = _counts(geo, 0)
    out = _assemble(xs, geo, counts, _sets(counts), dtype, 1.0 / P0, rescale=False)  # the mean over P, not over cnt
    _rejects(xs, out, counts, geo, dtype, "block 0 chunk 0", P0 - 1, 1.0 / P0, True,
             also=[r"ranks \[0, 1, 2\] with coefficient float32\(scale\) = 0\.25"])
    # and the other way round; on the straggler the two rules agree where the count is P
    good = _assemble(xs, geo, counts, _sets(counts), dtype, 1.0 / P0, rescale=True)
    _rejects(xs, good, counts, geo, dtype, "block 0 chunk 0", P0 - 1, 1.0 / P0, False,
             also=[r"with coefficient scale \* P / 3 = 0\.3333"])


def test_rescaled_coefficient_is_the_fp32_reciprocal_of_the_count():
    """(float32(1 / P) * P) / cnt in fp32 is float32(1 / cnt) for every membership the kernels
    take up to 8 ranks: the rescaled mean divides the fp32 sum by the count and nothing else."""
    for P in range(2, 9):
        for cnt in range(1, P + 1):
            assert partial_coef(1.0 / P, P, cnt, True) == float(torch.tensor(1.0 / cnt, dtype=torch.float32)), (P, cnt)
            assert partial_coef(1.0 / P, P, cnt, False) == float(torch.tensor(1.0 / P, dtype=torch.float32))
    assert partial_coef(0.3, 4, 0, True) == float(torch.tensor(0.3, dtype=torch.float32))  # count 0: no division


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_a_stale_contribution(dtype):
    """One contribution read from another round's data."""
    xs, geo = _xs(dtype), _geometry(dtype)
    stale = _xs(dtype, seed=6)
    counts = _counts(geo, 0)
    good = _assemble(xs, geo, counts, _sets(counts), dtype)
    wrong = _assemble([xs[0], stale[1]] + xs[2:], geo, counts, _sets(counts), dtype)
    out = _mutate_chunk(good, wrong, geo, 2, 0)
    for allowed in (ALLOWED0, None):
        _rejects(xs, out, counts, geo, dtype, "block 2 chunk 0", P0 - 1, allowed=allowed,
                 also=["no contributor set of any size"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_a_contributor_set_of_the_wrong_size(dtype):
    xs, geo = _xs(dtype), _geometry(dtype)
    counts = _counts(geo, 0)
    everyone = [frozenset(range(P0)) if S else S for S in _sets(counts)]
    out = _assemble(xs, geo, counts, everyone, dtype)  # the straggler's data is in, the count says it is not
    for allowed in (ALLOWED0, None):
        _rejects(xs, out, counts, geo, dtype, "block 0 chunk 0", P0 - 1, allowed=allowed,
                 also=[r"it equals the result of ranks \[0, 1, 2, 3\]"])
    # the right size, the wrong set: only `allowed` tells
    other = [frozenset({1, 2, 3}) if S else S for S in _sets(counts)]
    out = _assemble(xs, geo, counts, other, dtype)
    assert check_partial_round(xs, out, counts, geo, dtype)[0] == frozenset({1, 2, 3})
    _rejects(xs, out, counts, geo, dtype, "block 0 chunk 0", P0 - 1, also=[r"it equals the result of ranks \[1, 2, 3\]"])
    # a count the round cannot have
    bad = list(counts)
    bad[0] = 2
    _rejects(xs, out, bad, geo, dtype, "block 0 chunk 0", 2, also=["cannot have"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_what_is_not_plus_zero_in_a_given_up_chunk(dtype):
    xs, geo = _xs(dtype), _geometry(dtype)
    counts = _counts(geo, 0)
    good = _assemble(xs, geo, counts, _sets(counts), dtype)
    lo, hi = chunk_ranges(N0, P0, *geo)[SLOW0 * geo[2]]
    assert counts[SLOW0 * geo[2]] == 0 and hi - lo > 2
    name = f"block {SLOW0} chunk 0"
    for at, value in ((lo + 1, -0.0), (hi - 1, -7.0), (lo, float("nan"))):
        out = good.clone()
        out[at] = value
        assert at == lo or bool((out[lo:hi] == 0).all()) == (value == 0)  # -0 == 0: only the bits tell
        msg = _rejects(xs, out, counts, geo, dtype, name, 0, also=[f"element {at} is", "not \\+0 bit for bit"])
        if value == 0:  # the -0: the bits of the element type
            assert f"bits {1 << (8 * es_of(dtype) - 1):#x}" in msg
    out = good.clone()  # the whole chunk summed although it was given up
    out[lo:hi] = exact_sum(xs, dtype)[lo:hi]
    _rejects(xs, out, counts, geo, dtype, name, 0, also=[r"it equals the result of ranks \[0, 1, 2, 3\]"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_rejects_a_chunk_boundary_off_by_one(dtype):
    xs, geo = _xs(dtype), _geometry(dtype)
    nch = geo[2]
    counts = _counts(geo, 0, given_up=[(1, 1)])
    good = _assemble(xs, geo, counts, _sets(counts), dtype)
    ranges = chunk_ranges(N0, P0, *geo)
    lo, hi = ranges[1 * nch + 1]
    full = exact_sum([xs[k] for k in sorted(FAST0)], dtype)
    assert full[lo] != 0 and full[hi] != 0 and full[lo - 1] != 0 and full[hi - 1] != 0
    out = good.clone()
    out[hi] = 0          # the zeros reach one element into the next chunk
    nxt = "block 1 chunk 2" if nch > 2 and ranges[nch + 2][1] > ranges[nch + 2][0] else "block 2 chunk 0"
    _rejects(xs, out, counts, geo, dtype, nxt, P0 - 1, also=[f"first {hi}:"])
    out = good.clone()
    out[lo - 1] = 0      # ... or start one element early
    _rejects(xs, out, counts, geo, dtype, "block 1 chunk 0", P0 - 1, also=[f"first {lo - 1}:"])
    out = good.clone()
    out[lo] = full[lo]   # the neighbour's sum reaches one element into the given-up chunk
    _rejects(xs, out, counts, geo, dtype, "block 1 chunk 1", 0, also=[f"element {lo} is"])
    out = good.clone()
    out[hi - 1] = full[hi - 1]
    _rejects(xs, out, counts, geo, dtype, "block 1 chunk 1", 0, also=[f"element {hi - 1} is"])
    # and a geometry that is off: the ranges must tile [0, n) and the counts must fit them
    shifted = [(a, b + 1) if (a, b) == (lo, hi) else (a, b) for a, b in ranges]
    with pytest.raises(PartialRoundError, match="does not continue the tiling"):
        check_partial_round(xs, good, counts, shifted, dtype)
    with pytest.raises(PartialRoundError, match=r"cover \[0, \d+\) of"):
        check_partial_round(xs, good, counts[:-nch], ranges[:-nch], dtype)
    with pytest.raises(PartialRoundError, match="counts for"):
        check_partial_round(xs, good, counts[:-1], ranges, dtype)


def test_checker_rejects_a_count_for_a_chunk_that_does_not_exist():
    dtype = torch.bfloat16
    xs, geo = _xs(dtype), _geometry(dtype)
    nch = geo[2]
    counts = _counts(geo, SLOW0)
    good = _assemble(xs, geo, counts, _sets(counts), dtype)
    ranges = chunk_ranges(N0, P0, *geo)
    missing = [i for i, (lo, hi) in enumerate(ranges) if hi <= lo]
    assert missing and missing[0] // nch == P0 - 1  # the short last block
    bad = list(counts)
    bad[missing[0]] = P0
    _rejects(xs, good, bad, geo, dtype, f"block {P0 - 1} chunk {missing[0] % nch}", P0, also=["does not exist"])


def test_checker_takes_nan_where_the_sum_is_nan_and_nowhere_else():
    dtype = torch.float16
    xs, geo = _xs(dtype), _geometry(dtype)
    xs[0][3] = float("nan")
    xs[1][5] = float("inf")
    xs[SLOW0][9] = float("inf")  # the straggler's: left out of this chunk
    counts = _counts(geo, 0)
    out = _assemble(xs, geo, counts, _sets(counts), dtype)
    assert out[3].isnan() and out[5] == float("inf") and out[9].isfinite()
    check_partial_round(xs, out, counts, geo, dtype, allowed=ALLOWED0)
    out[9] = float("nan")
    _rejects(xs, out, counts, geo, dtype, "block 0 chunk 0", P0 - 1, also=["first 9:"])


# ------------------------------------------------------------------------------------------
# What makes "any set of the reported size" a check: the chunk identifies its contributors.
# ------------------------------------------------------------------------------------------
def _agreeing_window(a, b, w=8):
    """Whether a and b agree on w consecutive elements somewhere."""
    eq = (a == b).to(torch.int8)
    return bool((eq.unfold(0, w, 1).sum(1) == w).any())


@pytest.mark.parametrize("mode", ["wide", "narrow"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_no_two_sets_without_one_rank_agree_on_8_elements_of_the_direct_data(P, dtype, mode):
    xs = exact_inputs(P, NMAX, dtype, mode, seed=direct_seed(P, dtype, mode))
    res = [exact_sum([xs[k] for k in range(P) if k != out], dtype) for out in range(P)]
    for a, b in itertools.combinations(range(P), 2):
        assert not _agreeing_window(res[a], res[b]), (a, b)
    full = exact_sum(xs, dtype)
    assert all(not _agreeing_window(full, r) for r in res)  # nor does a full sum pass for a partial one


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_two_sets_of_one_size_agree_on_8_elements_of_the_plane_data(dtype):
    P = PLANE_P
    per_round = []
    for it in range(PLANE_ROUNDS):
        xs = exact_inputs(P, PLANE_N, dtype, "wide", seed=plane_seed(dtype, it))
        res = {S: exact_sum([xs[k] for k in S], dtype) for c in range(1, P + 1) for S in itertools.combinations(range(P), c)}
        for S, T in itertools.combinations(res, 2):
            if len(S) == len(T):
                assert not _agreeing_window(res[S], res[T]), (it, S, T)
        per_round.append(res)
    for a, b in itertools.combinations(range(PLANE_ROUNDS), 2):  # and no round passes for another (a stale read)
        for S in per_round[a]:
            assert not _agreeing_window(per_round[a][S], per_round[b][S]), (a, b, S)


# ------------------------------------------------------------------------------------------
# The case table of the GPU file, through the planner alone.
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_lag", LAGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_every_direct_case_can_complete_without_its_straggler(P, dtype, max_lag):
    es, pack = es_of(dtype), 16 // es_of(dtype)
    cases = direct_cases(cluster_knobs(P, max_lag), P, dtype)
    kept = [n for n, _, _ in cases]
    # every size but the largest fits every cluster; the largest wherever n * es <= P * slot
    assert kept == [n for n in base_sizes(dtype) if n * es <= P * SLOT], kept
    assert kept[:4] == [7, pack + 1, 4099, 65539] and (NMAX in kept) == (NMAX * es <= P * SLOT)
    for n, plan, slows in cases:
        per = chunks_per_block(plan, n, P)
        assert (plan["full"], plan["oneshot"], plan["sub"], plan["min_reduce"]) == (0, 0, 1, P - 1), (n, plan)
        assert sum(per) >= plan["min_complete"] >= 1
        assert slows[0] == P - 1, (n, plan)  # the last rank can always straggle
        for s in slows:  # the precondition: the fast ranks complete from the chunks outside the straggler's block
            assert plan["min_complete"] <= sum(per) - per[s], (n, s, plan)
        if 0 not in slows:  # rank 0 is left out only where block 0 is the only block that exists
            assert per[0] > 0 and sum(per[1:]) == 0, (n, per)
    n, plan, _ = cases[0]  # 7 elements: less than a pack of a 16-bit type and one block; two blocks of fp32
    assert chunks_per_block(plan, n, P) == ([1, 1] + [0] * (P - 2) if es == 4 else [1] + [0] * (P - 1))
    assert es == 4 or n < pack
    n, plan, _ = cases[1]  # pack + 1: two tiny blocks (from 3 ranks on the last ones are empty)
    assert [c for c in chunks_per_block(plan, n, P) if c] == [1, 1]
    n, plan, _ = cases[2]  # 4099: several chunks per block and a short last block
    per = chunks_per_block(plan, n, P)
    assert 2 <= per[0] <= 9 and (n - (P - 1) * plan["block"]) % plan["chunk"] != 0 and n % pack != 0
    n, plan, _ = cases[3]  # 65539: chunks of about 1030 elements, less than one batch of any instantiation (nu < U)
    assert 1024 <= plan["chunk"] <= 1056 and plan["chunk"] // pack < 2 * 256, plan


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_two_rank_small_grid_chunks_hold_a_full_batch(dtype):
    P, es = 2, es_of(dtype)
    n = full_batch_size(dtype)
    for max_lag in LAGS:
        k = cluster_knobs(P, max_lag, SMALL_GRID)
        (m, plan, slows), = direct_cases(k, P, dtype, [n])
        assert m == n and n * es <= P * SLOT < (n + 4) * es and slows == [1, 0]
        assert plan["chunk"] // (16 // es) >= FULL_BATCH_PACKS, plan
        full = H.plan_threshold(k, n, es, P, 1.0, 1.0)  # the full-mask round there: the same chunks, the two-shot body
        assert (full["full"], full["oneshot"], full["chunk"]) == (1, 0, plan["chunk"]), full
        # at the grid of the other clusters no size of the table reaches a full batch: this cluster is needed
        for _, p64, _ in direct_cases(cluster_knobs(P, max_lag), P, dtype):
            assert p64["chunk"] // (16 // es) < FULL_BATCH_PACKS, p64


def test_plane_geometries():
    for chunk in PLANE_CHUNKS:
        lay = C.BlockLayout(PLANE_N, PLANE_P, chunk)
        nch = max(lay.num_chunks(j) for j in range(PLANE_P))
        ranges = [r for r in plane_ranges(PLANE_N, PLANE_P, chunk, nch) if r[1] > r[0]]
        assert ranges[0][0] == 0 and ranges[-1][1] == PLANE_N and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        # 250 elements of a 16-bit type are 500 B: chunks start off the 16-byte grid within a block
        assert any((lo - lay.start[0]) * 2 % 16 for lo, _ in ranges[:nch]) == (chunk == 250)
