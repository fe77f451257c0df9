"""plan_rooted (csrc/runtime/launch_geometry.cc) on the CPU: the invariants the broadcast and
reduce kernels (csrc/hip/xgmi_rooted.hip) rely on, over a sweep of worlds, element sizes, ranks
per launch, sizes and grid settings. Properties, not recorded values."""
import pytest

from akka_allreduce_1_amd._native import C

H = C.hip
KiB, MiB = 1 << 10, 1 << 20
SLOT = 64 * MiB
KINDS = ("broadcast", "reduce")
WORLDS = (2, 3, 4, 8, 16)
SIZES = (1, 10, 1000, 4099, 64 * KiB, 1000003, MiB, 4 * MiB, 16 * MiB, 64 * MiB)
GRIDS = ((512, 512, 1), (64, 512, 1), (1, 512, 1), (512, 512, 0))  # grid, default_grid, size_grid


def default_knobs(world, **kw):
    L = H.slab_layout(world, SLOT, 0)
    k = H.GridKnobs()
    for name, v in dict(world=world, rows=1, maxch=L["maxch"], slot_bytes=L["slot_bytes"], **kw).items():
        setattr(k, name, v)
    return k


def cases():
    for kind in KINDS:
        for world in WORLDS:
            for es in (2, 4):
                for rh in (1, world):
                    for grid, default_grid, size_grid in GRIDS:
                        yield kind, world, es, rh, grid, default_grid, size_grid


@pytest.mark.parametrize("kind", KINDS)
def test_geometry_invariants_over_the_sweep(kind):
    checked = thrown = 0
    for k_, world, es, rh, grid, default_grid, size_grid in cases():
        if k_ != kind:
            continue
        k = default_knobs(world, grid=grid, default_grid=default_grid, size_grid=bool(size_grid))
        for n in SIZES:
            ctx = (kind, world, es, rh, grid, size_grid, n)
            expect_block = -(-(-(-n // world)) // (16 // es)) * (16 // es)
            if expect_block * es > k.slot_bytes + 16:  # the host never plans such a segment
                with pytest.raises(RuntimeError, match="^XgmiComm:"):
                    H.plan_rooted(kind, k, n, es, rh)
                thrown += 1
                continue
            g = H.plan_rooted(kind, k, n, es, rh)
            assert g["block"] == expect_block, ctx
            assert g["block"] * es % 16 == 0 and g["block"] * world >= n, ctx
            assert g["chunk"] * g["nch"] >= g["block"] and g["chunk"] * es % 16 == 0, ctx
            assert g["chunk"] * es >= 1024, ctx  # a flag word per KiB of slot at most
            assert g["subchunk"] * g["sub"] >= g["chunk"] and g["subchunk"] * es % 16 == 0, ctx
            assert g["nch"] >= 1 and g["sub"] >= 1, ctx
            assert g["nch"] * g["sub"] <= k.maxch, ctx
            assert 1 <= g["gx"] <= max(1, grid // rh), ctx
            if kind == "broadcast":
                assert g["sub"] == 1 and g["subchunk"] == g["chunk"], ctx
            else:
                assert g["sub"] <= max(1, world - 1), ctx
            # every chunk lies inside one slot
            assert (g["nch"] - 1) * g["chunk"] < g["block"] or g["nch"] == 1, ctx
            checked += 1
    assert checked >= 500 and thrown >= 10


@pytest.mark.parametrize("kind", KINDS)
def test_a_block_larger_than_the_slot_throws(kind):
    """Default knobs (64 MiB slots): 2 ranks x 256 MiB fp32 would be blocks of 128 MiB."""
    k = default_knobs(2)
    with pytest.raises(RuntimeError) as e:
        H.plan_rooted(kind, k, 64 * MiB, 4, 1)
    assert type(e.value) is RuntimeError and str(e.value).startswith("XgmiComm:")
    assert H.plan_rooted(kind, k, 2 * (SLOT // 4), 4, 1)["block"] * 4 == SLOT  # a full slot fits


def test_kind_is_checked():
    with pytest.raises(ValueError, match="broadcast or reduce"):
        H.plan_rooted("gather", default_knobs(2), 1024, 4, 1)


def test_broadcast_of_8_x_1_mib_matches_the_all_gather_of_its_blocks():
    """A broadcast chunks a block by plan_coll's all-gather rule, a reduce by its reduce-scatter
    rule: 1 MiB over 8 ranks, one rank per launch, is blocks of 128 KiB."""
    k = default_knobs(8)
    n = MiB // 2
    b = H.plan_rooted("broadcast", k, n, 2, 1)
    ag = H.plan_coll("all_gather", k, n // 8, 2, 1)
    assert (b["block"], b["chunk"], b["nch"], b["gx"]) == (n // 8, ag["chunk"], ag["nch"], ag["gx"])
    r = H.plan_rooted("reduce", k, n, 2, 1)
    rs = H.plan_coll("reduce_scatter", k, n // 8, 2, 1)
    assert (r["chunk"], r["subchunk"], r["nch"], r["sub"]) == (rs["chunk"], rs["subchunk"], rs["nch"], rs["sub"])
