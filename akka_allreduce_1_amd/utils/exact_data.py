"""Rank inputs whose sum does not depend on the order it is taken in.

Every reducing kernel of the data plane promises fp32 accumulation and ONE rounding to the
element type, but each sums in an order of its own (two-shot per block owner, ring per hop,
one-shot in rank order), and fp32 addition of arbitrary values depends on the order. Inputs on
a grid take the order out: x[k][i] = m * 2^-10 with a uniform integer |m| < 2^b, so every
partial sum of at most 16 ranks has at most b + 4 <= 24 significant bits and is exact in fp32
whatever the order. The expected result is then ONE round-to-nearest-even of an exact value,
the same for every once-rounded kernel, and `torch.equal` applies.

  wide    b = 8 (bf16), 11 (fp16), 20 (fp32): every input is exact in its type and the result
          needs one real rounding (bf16 / fp16; an fp32 result is exact).
  narrow  b = 5 (bf16), 8 (fp16), 20 (fp32): every partial sum of at most 8 ranks is
          representable in the element type, so a kernel that rounds at every hop by design
          is bit-exact too.

Everything here runs on the CPU; tests/test_exact_data.py checks the claims above.
"""
from __future__ import annotations

from typing import Sequence

import torch

GRID_EXP = 10  # inputs are multiples of 2^-10
MAX_RANKS = 16  # b + log2(MAX_RANKS) <= 24 for every b below (the kernels take 16 ranks at most)
BITS = {
    "wide": {torch.bfloat16: 8, torch.float16: 11, torch.float32: 20},
    "narrow": {torch.bfloat16: 5, torch.float16: 8, torch.float32: 20},
}
# significant bits of the element types (implicit one included)
PRECISION = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}


def exact_inputs(P: int, n: int, dtype: torch.dtype, mode: str = "wide", seed: int = 0,
                 grid_exp: int = GRID_EXP) -> list[torch.Tensor]:
    """The P rank tensors (CPU, n elements of `dtype`): m * 2^-grid_exp, |m| < 2^BITS[mode][dtype],
    from a seeded generator."""
    if not 1 <= P <= MAX_RANKS:
        raise ValueError(f"exact_inputs: P must be in [1, {MAX_RANKS}]")
    b = BITS[mode][dtype]
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-(1 << b) + 1, 1 << b, (P, n), generator=g, dtype=torch.int64)
    x = (m.double() * 2.0 ** -grid_exp).to(dtype)
    return [x[k].contiguous() for k in range(P)]


def exact_sum(xs: Sequence[torch.Tensor], dtype: torch.dtype, scale: float = 1.0) -> torch.Tensor:
    """What a once-rounded kernel must return for the rank tensors `xs`: the fp64 sum, which
    must be exact in fp32 (ValueError otherwise: the data is not order-free), times
    float32(scale) in fp32 where scale != 1 (the kernels multiply their fp32 sum by the fp32
    scale), rounded to `dtype` once. dtype=torch.float64 returns the unrounded sum. NaN and
    infinities follow IEEE addition."""
    s = torch.stack([x.double() for x in xs]).sum(0)
    s32 = s.float()
    if not bool(((s32.double() == s) | s.isnan()).all()):
        raise ValueError("exact_sum: the sum of these inputs is not exact in fp32")
    if scale != 1.0:
        s32 = s32 * torch.tensor(scale, dtype=torch.float32)
    return s32.to(dtype)


def per_hop_sum(xs: Sequence[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """The mutant a once-rounded kernel must differ from: a chain in rank order that rounds
    its partial sum to `dtype` after every add (what `ring_native` does by design)."""
    q = xs[0].to(dtype)
    for x in xs[1:]:
        q = (q.float() + x.float()).to(dtype)
    return q


def truncated_sum(xs: Sequence[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """The second mutant: the exact fp32 sum converted to bf16 / fp16 by truncation (round
    toward zero) instead of round-to-nearest-even."""
    s32 = exact_sum(xs, torch.float32)
    if dtype == torch.float32:
        return s32
    r = s32.to(dtype)
    over = r.float().abs() > s32.abs()  # RNE went away from zero: one step back
    bits = r.view(torch.int16).to(torch.int32) & 0xFFFF
    bits = torch.where(over, bits - 1, bits)  # sign-magnitude: the magnitude is the low 15 bits
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits)
    return bits.to(torch.int16).view(dtype)


def rounding_profile(xs: Sequence[torch.Tensor], dtype: torch.dtype) -> tuple[float, float]:
    """(fraction of results that are inexact in `dtype`, fraction that are exact ties), read from
    the fp32 bit pattern of the exact sum: the bits below the target's mantissa."""
    drop = 24 - PRECISION[dtype]
    if drop == 0:
        return 0.0, 0.0
    low = exact_sum(xs, torch.float32).view(torch.int32) & ((1 << drop) - 1)
    n = low.numel()
    return float((low != 0).sum()) / n, float((low == (1 << (drop - 1))).sum()) / n


def per_hop_bound(xs: Sequence[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """Per element, the most a sum rounded to `dtype` after each of its P - 1 adds can differ
    from the exact (unrounded) sum, in any order: (P - 1) half-ulps of the largest value a
    partial sum can take. B = sum_k |x_k| bounds every exact partial sum; the rounded ones stay
    below B' = B * (1 + (P - 1) * 2^-p) (by induction: each rounding adds at most 2^-p of a
    value below B'), so each add errs by at most half an ulp of B'. fp64."""
    P, p = len(xs), PRECISION[dtype]
    B = torch.stack([x.double().abs() for x in xs]).sum(0) * (1.0 + (P - 1) * 2.0 ** -p)
    _, e = torch.frexp(B)  # B < 2^e: values up to B have ulp 2^(e - p) at most
    return torch.where(B > 0, (P - 1) * torch.ldexp(torch.ones_like(B), e - p - 1), torch.zeros_like(B))
