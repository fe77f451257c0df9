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

A threshold round that leaves contributions out is held to the same standard chunk by chunk:
`check_partial_round` takes one rank's output and the counts it reported and demands, for every
chunk, +0 bits (count 0) or the once-rounded sum over one set of exactly `count` ranks times the
fp32 coefficient of that count (`partial_coef`). On this data the result of a chunk identifies
its contributors (no two sets of one size agree on 8 consecutive elements).

Everything here runs on the CPU; tests/test_exact_data.py and tests/test_partial_round.py check
the claims above.
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


def partial_coef(scale: float, P: int, count: int, rescale: bool) -> float:
    """The fp32 coefficient a threshold round multiplies the fp32 sum of a chunk of `count`
    contributions by, as a Python float (pass it to `exact_sum` as its scale): float32(scale),
    or with rescale (float32(scale) * P) / count, evaluated in fp32 from left to right."""
    c = torch.tensor(scale, dtype=torch.float32)
    if rescale and count > 0:
        c = (c * torch.tensor(float(P), dtype=torch.float32)) / torch.tensor(float(count), dtype=torch.float32)
    return float(c)


class PartialRoundError(AssertionError):
    """check_partial_round: the output does not follow from its counts."""


def chunk_ranges(n: int, P: int, block: int, chunk: int, nch: int) -> list[tuple[int, int]]:
    """The element range [lo, hi) of chunk c of block j at index j * nch + c, for the kernel
    geometry (block, chunk, nch); lo == hi for a chunk past the end of a short or empty block."""
    out = []
    for j in range(P):
        bend = min(n, (j + 1) * block)
        for c in range(nch):
            lo = min(bend, j * block + min(c * chunk, block))
            out.append((lo, max(lo, min(bend, j * block + min((c + 1) * chunk, block)))))
    return out


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _agree(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Per element: the same value (`torch.equal`'s comparison), or NaN where NaN is expected."""
    return (got == want) | (got.isnan() & want.isnan())


def check_partial_round(xs: Sequence[torch.Tensor], out: torch.Tensor, counts, geometry, dtype: torch.dtype,
                        scale: float = 1.0, rescale: bool = False, allowed=None, memo: dict | None = None,
                        what: str = "") -> list[frozenset]:
    """One rank's output of one threshold round against the counts it reported.

    xs        the P rank tensors of the round (n elements of `dtype`)
    out       the rank's output, n elements
    counts    one count per chunk, flat or [P][nch]: how many contributions the chunk holds
    geometry  (block, chunk, nch) of the kernel (chunk j * nch + c is chunk c of block j), or the
              list of (lo, hi) element ranges of the chunks, in the order of `counts`
    scale, rescale   the coefficient rule (partial_coef)
    allowed   {count: contributor sets} - the only sets a chunk of that count may hold, and a
              count that is no key fails; None: any set of `count` ranks
    memo      a dict the caller keeps for these `xs`: the expected sums are computed once

    The rule: the ranges of the chunks that exist tile [0, n) exactly, in order; a chunk that
    does not exist reports count 0; a chunk of count 0 is +0 in every element, bit for bit; a
    chunk of count c > 0 equals exact_sum over ONE set of exactly c ranks, times the
    coefficient of c, rounded once (NaN where and only where that sum is NaN).
    Returns the contributor set of every chunk (the first that fits; empty for count 0), or
    raises PartialRoundError naming the first bad chunk, its count, the first differing element
    with got / want, and the contributor set and coefficient, if any, that would have matched."""
    import itertools

    P, n = len(xs), out.numel()
    xs = [x.detach().cpu() for x in xs]
    out = out.detach().cpu()
    counts = [int(c) for c in torch.as_tensor(counts).flatten().tolist()]
    if isinstance(geometry, tuple) and len(geometry) == 3 and not isinstance(geometry[0], (tuple, list)):
        block, chunk, nch = geometry
        ranges = chunk_ranges(n, P, block, chunk, nch)
        names = [f"block {j} chunk {c}" for j in range(P) for c in range(nch)]
    else:
        ranges = [(int(lo), int(hi)) for lo, hi in geometry]
        names = [f"chunk {i}" for i in range(len(ranges))]
    memo = {} if memo is None else memo

    def fail(msg):
        raise PartialRoundError(f"{what}: {msg}" if what else msg)

    if out.dtype != dtype or any(x.dtype != dtype or x.numel() != n for x in xs):
        fail(f"the output and the {P} rank tensors must hold {n} elements of {dtype}")
    if len(counts) != len(ranges):
        fail(f"{len(counts)} counts for {len(ranges)} chunks")
    at = 0
    for i, (lo, hi) in enumerate(ranges):
        if hi <= lo:
            if counts[i] != 0:
                fail(f"{names[i]} does not exist (past the end of its block) but reports count {counts[i]}")
            continue
        if lo != at or hi > n:
            fail(f"{names[i]} [{lo}, {hi}) does not continue the tiling of [0, {n}) at element {at}")
        at = hi
    if at != n:
        fail(f"the chunks cover [0, {at}) of [0, {n})")

    def want(S, coef):
        key = (tuple(sorted(S)), coef)
        if key not in memo:
            memo[key] = exact_sum([xs[k] for k in key[0]], dtype, coef)
        return memo[key]

    def sets_of(c):
        if allowed is not None:
            return [frozenset(S) for S in allowed[c]]
        return [frozenset(S) for S in itertools.combinations(range(P), c)]

    def bad_prefix(ok):  # bad_prefix[i] = number of disagreeing elements before i
        return torch.cat([torch.zeros(1, dtype=torch.int64), (~ok).to(torch.int64).cumsum(0)])

    def explain(i, lo, hi):
        """Which set and coefficient, of any size, gives out[lo:hi]."""
        fits = []
        if bool((_bits(out[lo:hi]) == 0).all()):
            fits.append("no contribution (+0)")
        coefs = {"float32(scale)": partial_coef(scale, P, 1, False)}
        for c in range(1, P + 1):
            coefs[f"scale * P / {c}"] = partial_coef(scale, P, c, True)
        for c in range(1, P + 1):
            for S in itertools.combinations(range(P), c):
                for label, coef in coefs.items():
                    if bool(_agree(out[lo:hi], want(S, coef)[lo:hi]).all()):
                        fits.append(f"ranks {list(S)} with coefficient {label} = {coef!r}")
        return ("it equals the result of " + " / ".join(dict.fromkeys(fits))) if fits else \
            "no contributor set of any size gives it"

    found: list[frozenset] = [frozenset()] * len(ranges)
    zero_ok = bad_prefix(_bits(out) == 0)
    per: dict = {}  # (count, set) -> prefix of disagreements with that expectation
    for i, (lo, hi) in enumerate(ranges):
        c = counts[i]
        if hi <= lo:
            continue
        if c == 0:
            if int(zero_ok[hi] - zero_ok[lo]):
                e = lo + int((_bits(out[lo:hi]) != 0).nonzero()[0])
                fail(f"{names[i]} [{lo}, {hi}) has count 0 but is not +0 bit for bit: element {e} is "
                     f"{float(out[e])!r} (bits {int(_bits(out[e:e + 1])[0]) & ((1 << 8 * out.element_size()) - 1):#x}); "
                     f"{explain(i, lo, hi)}")
            continue
        if c < 0 or c > P or (allowed is not None and c not in allowed):
            fail(f"{names[i]} [{lo}, {hi}) reports count {c}, which this round cannot have "
                 f"(counts of the rank: {counts})")
        coef = partial_coef(scale, P, c, rescale)
        cands = sets_of(c)
        for S in cands:
            if (c, S) not in per:
                per[(c, S)] = bad_prefix(_agree(out, want(S, coef)))
            if int(per[(c, S)][hi] - per[(c, S)][lo]) == 0:
                found[i] = S
                break
        else:
            S = cands[0]
            w = want(S, coef)
            e = lo + int((~_agree(out[lo:hi], w[lo:hi])).nonzero()[0])
            nbad = int(per[(c, S)][hi] - per[(c, S)][lo])
            fail(f"{names[i]} [{lo}, {hi}) has count {c} but equals the once-rounded sum of none of the "
                 f"{len(cands)} contributor sets of that size (coefficient {coef!r}); against ranks {sorted(S)}: "
                 f"{nbad} of {hi - lo} elements differ, first {e}: got {float(out[e])!r} want {float(w[e])!r}, "
                 f"inputs there {[float(x[e]) for x in xs]}; {explain(i, lo, hi)}")
    return found


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
