"""Numerics of the HIP data-plane kernels vs plain PyTorch fp32 references (gfx950)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from akka_allreduce_1_amd.ops import bucket_copy, cast, fill_iota, fill_uniform, reduce_slots  # noqa: E402
from akka_allreduce_1_amd.ops.kernels import BucketTable  # noqa: E402

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("P,n", [(1, 1000), (2, 4096), (3, 12345), (8, 1 << 20), (5, 7)])
def test_reduce_slots_matches_fp32_reference(dtype, P, n):
    padded = torch.randn(P, (n + 7) // 8 * 8, device=DEV).to(dtype)  # 16-B aligned rows
    slots = padded[:, :n]
    out = reduce_slots(slots)
    ref = torch.zeros(n, device=DEV)
    for p in range(P):  # same summation order as the kernel and the reference's reduce loop
        ref += slots[p].float()
    torch.cuda.synchronize()
    if dtype == torch.float32:
        assert torch.equal(out, ref)
    else:  # one rounding of the fp32 sum (RNE), like torch's conversion
        assert torch.equal(out, ref.to(dtype))


def test_reduce_slots_scale_and_tail():
    slots = torch.randn(4, 1008, device=DEV)[:, :1003]
    out = reduce_slots(slots, scale=0.25)
    ref = slots.sum(0) * 0.25
    torch.cuda.synchronize()
    assert torch.allclose(out, ref, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_fill_iota_is_reference_data_source(dtype):
    t = fill_iota(torch.empty(1000, dtype=dtype, device=DEV), offset=3)
    ref = (torch.arange(1000, device=DEV, dtype=torch.float64) + 3).to(dtype)
    assert torch.equal(t, ref)


def test_fill_uniform_range_and_determinism():
    a = fill_uniform(torch.empty(1 << 16, device=DEV), seed=5)
    b = fill_uniform(torch.empty(1 << 16, device=DEV), seed=5)
    c = fill_uniform(torch.empty(1 << 16, device=DEV), seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.min() >= -1 and a.max() < 1 and abs(a.mean().item()) < 0.02


@pytest.mark.parametrize("low", [torch.bfloat16, torch.float16])
def test_cast_roundtrip_matches_torch(low):
    x = torch.randn(100_003, device=DEV)
    y = cast(x, low)
    assert torch.equal(y, x.to(low))
    z = cast(y, torch.float32)
    assert torch.equal(z, y.float())
    other = torch.float16 if low == torch.bfloat16 else torch.bfloat16
    assert torch.equal(cast(y, other), y.float().to(other))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bucket_copy_pack_unpack(dtype):
    ts = [torch.randn(s, device=DEV).to(dtype) for s in (17, 4096, 3, 1000, 64)]
    offs, o = [], 0
    for t in ts:
        offs.append(o)
        o += (t.numel() + 7) // 8 * 8  # 16-B aligned member offsets
    bucket = torch.zeros(o, dtype=dtype, device=DEV)
    table = BucketTable(ts, offs, DEV)
    bucket_copy(table, bucket, pack=True)
    for t, off in zip(ts, offs):
        assert torch.equal(bucket[off:off + t.numel()], t)
    bucket.mul_(2)
    bucket_copy(table, bucket, pack=False)
    torch.cuda.synchronize()
    for t, off in zip(ts, offs):
        assert torch.equal(t, bucket[off:off + t.numel()])


# ------------------------------------------------------------------------------------------
# Bit-exact checks on order-free data (akka_allreduce_1_amd/utils/exact_data.py): one rounding
# of an exact fp32 sum, whatever the kernel variant.
# ------------------------------------------------------------------------------------------
from akka_allreduce_1_amd._native import C  # noqa: E402
from akka_allreduce_1_amd.utils.exact_data import exact_inputs, exact_sum  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# packs of 16 B per lane in flight (U) of each reduce_slots variant (kernels.hip
# launch_reduce_typed); a tile is U x 256 packs. Variant 4 is the switch's default branch.
REDUCE_VARIANT_U = {0: 2, 1: 2, 2: 2, 3: 4, 4: 4, 5: 2, 6: 8, 7: None, 8: 4, 9: 4, 10: 4, 11: 8}


def _slot_rows(xs):
    """[P, n] view of the CPU rank tensors on the GPU with 16-byte aligned rows."""
    n = xs[0].numel()
    padded = torch.zeros(len(xs), (n + 7) // 8 * 8, dtype=xs[0].dtype, device=DEV)
    slots = padded[:, :n]
    slots.copy_(torch.stack(xs))
    return slots


def _differs(got, want):
    bad = (got != want).nonzero().flatten()
    return f"{bad.numel()} of {got.numel()} differ, first {int(bad[0])}: got {float(got[bad[0]])!r} want {float(want[bad[0]])!r}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [9, 16])
def test_reduce_slots_runtime_slot_count_is_once_rounded(P, dtype):
    """More than 8 slots take the runtime-P kernel (reduce_slots_kernel): tiles of 2 x 256 packs."""
    pack = 16 // torch.empty(0, dtype=dtype).element_size()
    for n in (7, 4099, 3 * 2 * 256 * pack + 5):
        xs = exact_inputs(P, n, dtype, "wide", seed=P + n)
        for scale in (1.0, 0.25):
            want = exact_sum(xs, dtype, scale).to(DEV)
            slots = _slot_rows(xs)
            out = reduce_slots(slots, scale=scale)
            assert torch.equal(out, want), (n, scale, _differs(out, want))
            assert torch.equal(slots, torch.stack(xs).to(DEV))  # the slots were only read
            assert reduce_slots(slots, out=slots[0], scale=scale) is not None  # out aliases slot row 0
            assert torch.equal(slots[0], want), (n, scale, "in place", _differs(slots[0], want))
            assert torch.equal(slots[1:], torch.stack(xs[1:]).to(DEV))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", range(12))
def test_reduce_slots_variants_are_once_rounded(variant, dtype):
    """Every variant the benchmarks select through set_reduce_variant, at 4 and 8 slots (the
    templated kernels; variant 7 picks its tile by the slot count) and out aliasing slot row 0."""
    pack = 16 // torch.empty(0, dtype=dtype).element_size()
    try:
        C.hip.set_reduce_variant(variant)
        for P in (4, 8):
            U = REDUCE_VARIANT_U[variant] or (2 if P > 4 else 4)
            for n in (7, 4099, 3 * U * 256 * pack + 5):
                xs = exact_inputs(P, n, dtype, "wide", seed=100 * variant + P)
                want = exact_sum(xs, dtype).to(DEV)
                slots = _slot_rows(xs)
                out = reduce_slots(slots)
                assert torch.equal(out, want), (P, n, _differs(out, want))
                reduce_slots(slots, out=slots[0], scale=0.5)
                want = exact_sum(xs, dtype, 0.5).to(DEV)
                assert torch.equal(slots[0], want), (P, n, "in place, scaled", _differs(slots[0], want))
                assert torch.equal(slots[1:], torch.stack(xs[1:]).to(DEV))
    finally:
        C.hip.set_reduce_variant(-1)


@pytest.mark.parametrize("variant", range(8))
def test_copy_variants_are_bit_exact_and_stay_in_bounds(variant):
    """hip.copy is the 1-rank allreduce of the bench headline. Byte counts: less than a pack, a
    pack, a ragged tail, one tile of the tiled variants (4 / 8 packs x 256 lanes) +- 16, and a
    unit of the unit variant (512 KiB) + 24."""
    guard = 256
    sizes = [1, 15, 16, 4097, (16 << 10) - 16, 16 << 10, (16 << 10) + 16, (32 << 10) - 16, (32 << 10) + 16, (512 << 10) + 24]
    g = torch.Generator().manual_seed(variant)
    src = torch.randint(0, 256, (max(sizes),), generator=g, dtype=torch.uint8).to(DEV)
    try:
        C.hip.set_copy_variant(variant)
        for nbytes in sizes:
            dst = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
            C.hip.copy(src.data_ptr(), dst.data_ptr(), nbytes, torch.cuda.current_stream(DEV).cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(dst[:nbytes], src[:nbytes]), nbytes
            assert bool((dst[nbytes:] == 0xA5).all()), f"{nbytes} bytes: wrote past the end"
    finally:
        C.hip.set_copy_variant(-1)


def _bits_equal_nan_by_mask(got, want):
    ints = {2: torch.int16, 4: torch.int32}[got.element_size()]
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(got.view(ints)[~nan], want.view(ints)[~nan])


@pytest.mark.parametrize("low", [torch.bfloat16, torch.float16])
def test_cast_every_16_bit_pattern_to_fp32(low):
    x = torch.arange(-32768, 32768, dtype=torch.int16).view(low)  # subnormals, infinities and NaNs included
    got = cast(x.to(DEV), torch.float32)
    assert _bits_equal_nan_by_mask(got.cpu(), x.float())


def _crafted_fp32():
    """Where a conversion to bf16 / fp16 goes wrong: exact ties that round down and up to even,
    their fp32 neighbours, the fp16 overflow tie, fp16 subnormal targets and their ties, the
    largest finite values, zeros, infinities and NaN; each with both signs. (No fp32 subnormal.)"""
    one = torch.tensor(1.0)
    ties = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,     # bf16: to 1.0 (even), to 1 + 2^-6 (even)
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,   # fp16: likewise
            65520.0,                               # fp16: the tie between 65504 and 2^16 -> inf
            2.0 ** -25, 3 * 2.0 ** -25,            # fp16 subnormals: to 0 (even), to 2^-23 (even)
            2.0 ** -14 - 2.0 ** -25]               # the largest fp16 subnormal | the smallest normal
    vals = []
    for t in ties:
        t32 = torch.tensor(t, dtype=torch.float32)
        assert float(t32) == t
        vals += [t32, torch.nextafter(t32, 2 * t32), torch.nextafter(t32, 0 * one)]
    vals += [torch.tensor(v, dtype=torch.float32) for v in (
        0.0, 1.0, 2.0 ** -24, 2.0 ** -14, 1023 * 2.0 ** -24, 65504.0, 65536.0,
        float(torch.finfo(torch.bfloat16).max), float(torch.finfo(torch.float32).max),
        (2 - 2.0 ** -8) * 2.0 ** 127,  # the tie between the largest bf16 and 2^128 -> inf
        float("inf"), float("nan"))]
    x = torch.stack(vals)
    return torch.cat([x, -x])


@pytest.mark.parametrize("low", [torch.bfloat16, torch.float16])
def test_cast_fp32_ties_limits_and_non_finite(low):
    x = _crafted_fp32()
    want = x.to(low)
    t = 0 if low == torch.bfloat16 else 6  # the type's two ties around 1: the reference rounds both to even
    assert want[t] == 1.0 and want[t + 3] == 1 + 2.0 ** (-6 if low == torch.bfloat16 else -9)
    got = cast(x.to(DEV), low).cpu()
    if not _bits_equal_nan_by_mask(got, want):
        bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero().flatten().tolist()
        pytest.fail(f"{low}: " + "; ".join(f"{float(x[i])!r} -> {float(got[i])!r}, want {float(want[i])!r}" for i in bad))
