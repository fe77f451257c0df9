"""The order-free data of akka_allreduce_1_amd/utils/exact_data.py, on the CPU: the claims the
bit-exact GPU comparisons (tests/test_exact_numerics_gpu.py) rest on. The sum of the inputs is
the same in every order, the expected result needs real roundings and real ties (so the GPU
tests cannot silently exercise no rounding), and the two classic wrong kernels - one that
rounds its partial sum at every hop, one that truncates - do differ from it."""
import pytest
import torch

from akka_allreduce_1_amd.utils.exact_data import (BITS, PRECISION, exact_inputs, exact_sum, per_hop_bound,
                                                   per_hop_sum, rounding_profile, truncated_sum)

N = 4099
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
WORLDS = [2, 3, 4, 8]


def _chain32(xs, order):
    acc = torch.zeros(xs[0].numel(), dtype=torch.float32)
    for k in order:
        acc = acc + xs[k].float()
    return acc


@pytest.mark.parametrize("mode", ["wide", "narrow"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", WORLDS)
def test_the_sum_is_the_same_in_every_order(P, dtype, mode):
    xs = exact_inputs(P, N, dtype, mode, seed=7 * P + 1)
    assert len(xs) == P and all(x.dtype == dtype and x.shape == (N,) for x in xs)
    b = BITS[mode][dtype]
    for x in xs:  # exact in the type: on the grid, within the range, unchanged through fp64
        m = x.double() * 1024.0
        assert torch.equal(m, m.round()) and float(m.abs().max()) < (1 << b)
        assert torch.equal(x.double().to(dtype), x)
    assert float(torch.stack(xs).double().abs().max()) * 1024.0 >= (1 << b) * 0.9  # and the range is used
    s64 = torch.stack([x.double() for x in xs]).sum(0)
    ranks = list(range(P))
    for order in (ranks, ranks[::-1], ranks[1:] + ranks[:1], ranks[P // 2:] + ranks[:P // 2]):
        assert torch.equal(_chain32(xs, order).double(), s64), order
    assert torch.equal(exact_sum(xs, torch.float64), s64)
    assert torch.equal(exact_sum(xs, torch.float32).double(), s64)  # an fp32 result is exact
    assert torch.equal(exact_sum(xs, dtype), s64.float().to(dtype))
    inv = torch.tensor(1.0 / P, dtype=torch.float32)
    assert torch.equal(exact_sum(xs, dtype, scale=1.0 / P), (s64.float() * inv).to(dtype))
    if mode == "narrow":  # every partial sum is representable in the element type
        assert torch.equal(per_hop_sum(xs, dtype), exact_sum(xs, dtype))
        assert torch.equal(exact_sum(xs, dtype).double(), s64)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("P", WORLDS)
def test_wide_results_round_and_tie_and_the_mutants_differ(P, dtype):
    xs = exact_inputs(P, N, dtype, "wide", seed=7 * P + 1)
    inexact, ties = rounding_profile(xs, dtype)
    print(f"P={P} {dtype}: {inexact:.1%} of the results are inexact, {ties:.1%} exact ties")
    assert inexact >= 0.05 and ties >= 0.01
    want = exact_sum(xs, dtype)
    trunc = int((truncated_sum(xs, dtype) != want).sum())
    hop = int((per_hop_sum(xs, dtype) != want).sum())
    print(f"  truncation differs in {trunc} elements, rounding at every hop in {hop}")
    assert trunc >= 1
    # the truncated result never lies beyond the sum, and differs only where RNE went away from zero
    t = truncated_sum(xs, dtype).double()
    s = exact_sum(xs, torch.float64)
    differs = t != want.double()
    assert bool((t.abs() <= s.abs()).all()) and bool((want.double().abs()[differs] > s.abs()[differs]).all())
    assert bool((t[~differs] == want.double()[~differs]).all()) and bool((t.sign() * s.sign() >= 0).all())
    if P >= 3:
        assert hop >= 1
    else:  # two ranks: one add, one rounding
        assert hop == 0
    # and the chain stays within the bound the ring_native comparison uses
    assert bool(((per_hop_sum(xs, dtype).double() - s).abs() <= per_hop_bound(xs, dtype)).all())


def test_swapping_the_reference_for_the_per_hop_chain_fails_wide_bf16():
    """What the GPU file would report with a per-hop-rounded reference in place of exact_sum:
    its comparison is torch.equal, and on this data the two differ in hundreds of elements."""
    for P in (3, 4, 8):
        xs = exact_inputs(P, N, torch.bfloat16, "wide", seed=7 * P + 1)
        differ = int((per_hop_sum(xs, torch.bfloat16) != exact_sum(xs, torch.bfloat16)).sum())
        print(f"P={P}: the per-hop chain differs from exact_sum in {differ} of {N} elements")
        assert differ >= N // 50
        assert not torch.equal(per_hop_sum(xs, torch.bfloat16), exact_sum(xs, torch.bfloat16))


def test_exact_sum_refuses_data_whose_sum_depends_on_order():
    xs = [torch.tensor([1.0]), torch.tensor([2.0 ** -30])]
    with pytest.raises(ValueError, match="not exact"):
        exact_sum(xs, torch.float32)


def test_non_finite_and_overflow_follow_ieee():
    inf, nan = float("inf"), float("nan")
    xs = [torch.tensor([inf, inf, nan, 65504.0, 65504.0, 32768.0], dtype=torch.float16),
          torch.tensor([1.0, -inf, 1.0, 16.0, 15.9921875, 32768.0], dtype=torch.float16)]
    y = exact_sum(xs, torch.float16)
    assert y[0] == inf and y[1].isnan() and y[2].isnan()
    assert y[3] == inf and y[4] == 65504.0 and y[5] == inf  # 65520 is the tie RNE sends to inf
    assert torch.equal(exact_sum(xs, torch.float32)[3:], torch.tensor([65520.0, 65519.9921875, 65536.0]))


@pytest.mark.parametrize("mode", ["wide", "narrow"])
def test_fp16_subnormal_inputs_on_the_2_pow_minus_24_grid(mode):
    """Multiples of 2^-24 are exact in fp16 (subnormal below 2^-14) and normal in fp32: the sum
    is exact there, and its fp16 rounding includes subnormal results."""
    xs = exact_inputs(4, N, torch.float16, mode, seed=24, grid_exp=24)
    tiny = torch.finfo(torch.float16).tiny
    for x in xs:
        m = x.double() * 2.0 ** 24
        assert torch.equal(m, m.round()) and bool(((x != 0) & (x.abs() < tiny)).any())
    s64 = torch.stack([x.double() for x in xs]).sum(0)
    assert float(s64.abs()[s64 != 0].min()) >= 2.0 ** -24 > torch.finfo(torch.float32).tiny
    want = exact_sum(xs, torch.float16)
    assert bool(((want != 0) & (want.abs() < tiny)).any())
    assert torch.equal(want.double(), s64) == (mode == "narrow")
    assert torch.equal(per_hop_sum(xs, torch.float16), want) == (mode == "narrow")


def test_precision_table():
    for dt, p in PRECISION.items():
        assert torch.finfo(dt).eps == 2.0 ** (1 - p)
