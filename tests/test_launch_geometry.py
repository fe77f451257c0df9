"""The launch planner (csrc/runtime/launch_geometry.cc) on the CPU: every geometry rule of the
data plane against tests/golden/launch_geometry.jsonl, the table the host code recorded
BEFORE the rules were split out of XgmiComm (the parent's unmodified launch_segment /
threshold_args / run_coll linked against stub HIP entry points, so the expected values never
came from the planner). All fields are integers: exact match, no tolerance.

A row: kind, world, rh (ranks in the launch), es, n; `knobs`: the GridKnobs that differ from
the defaults; `slab`: the layout inputs and the maxch / slot_bytes they gave where the slab is
not the default (64 MiB slots, 1 KiB per flag; threshold rounds: 2 lag rows); `th`, `spec`:
thresholds and RoundSpec of a threshold round; `out`: block chunk subchunk nch sub sgroup gx
(collectives: without block, their caller's m) and, for threshold rounds, min_reduce
min_complete full gate_shortcut oneshot lag_skip split; or `throws`: the message."""
import json
from pathlib import Path

import pytest

from akka_allreduce_1_amd._native import C

H = C.hip
KiB, MiB = 1 << 10, 1 << 20
ALLREDUCE = ("ll", "oneshot", "twoshot", "ring", "ring_native", "adamw")
COLL = ("all_to_all", "all_gather", "reduce_scatter")
GEO = ("block", "chunk", "subchunk", "nch", "sub", "sgroup", "gx")
TH = ("min_reduce", "min_complete", "full", "gate_shortcut", "oneshot", "lag_skip", "split")
ROWS = [json.loads(l) for l in (Path(__file__).parent / "golden" / "launch_geometry.jsonl").read_text().splitlines()]


def knobs(**kw):
    k = H.GridKnobs()
    for name, v in kw.items():
        setattr(k, name, v)
    return k


def trows(row):
    return row["slab"]["trows"] if "slab" in row else 2 if row["kind"] == "threshold" else 0


def plan(row):
    slab = row.get("slab", {"maxch": 65536, "slot_bytes": 64 * MiB})
    k = knobs(world=row["world"], rows=1 + trows(row), maxch=slab["maxch"], slot_bytes=slab["slot_bytes"],
              **row.get("knobs", {}))
    kind, args = row["kind"], (row["n"], row["es"], row["rh"])
    if kind in ALLREDUCE:
        return [H.plan_allreduce(kind, k, *args)[f] for f in GEO]
    if kind in COLL:
        return [H.plan_coll(kind, k, *args)[f] for f in GEO[1:]]
    p = H.plan_threshold(k, *args, *row["th"], **row.get("spec", {}))
    return [p[f] for f in GEO + TH]


def test_planner_reproduces_every_recorded_launch():
    differing = []
    for i, row in enumerate(ROWS):
        try:
            got = plan(row)
        except (ValueError, RuntimeError) as e:  # std::invalid_argument / std::logic_error
            got = str(e)
        if got != row.get("out", row.get("throws")):
            differing.append((i, row, got))
    assert not differing, f"{len(differing)} of {len(ROWS)} rows differ; first: {differing[0]}"


def test_throwing_rows_keep_their_exception_type():
    for row in ROWS:
        if "throws" in row:
            exc = RuntimeError if row["throws"].startswith("XgmiComm:") else ValueError  # logic_error / invalid_argument
            with pytest.raises(exc) as e:
                plan(row)
            assert type(e.value) is exc and str(e.value) == row["throws"]


def test_slab_layout_of_every_row():
    for row in ROWS:
        s = row.get("slab", {"slot": 64 * MiB, "gran": 0, "maxch": 65536, "slot_bytes": 64 * MiB})
        L = H.slab_layout(row["world"], s["slot"], trows(row), 0, s["gran"])
        assert (L["maxch"], L["slot_bytes"]) == (s["maxch"], s["slot_bytes"])
        assert L["off_R"] - L["off_S"] == (1 + trows(row)) * row["world"] * L["slot_stride"]
        assert L["slab_bytes"] == L["off_LL"] + 2 * row["world"] * L["ll_slot"] <= L["alloc_bytes"]


def test_the_table_is_not_thin():
    """Every kind, world, element size, grid setting, knob, threshold pair and throw the sweep
    asks for is in the table (and test_planner_reproduces_every_recorded_launch skips none)."""
    assert len(ROWS) >= 1000
    sizes = [4, 40, 4 * KiB, 64 * KiB, 128 * KiB, 256 * KiB, MiB, 2 * MiB, 4 * MiB, 16 * MiB, 32 * MiB, 64 * MiB, 256 * MiB]
    for kind in ALLREDUCE + COLL + ("threshold",):
        rows = [r for r in ROWS if r["kind"] == kind]
        assert len(rows) >= 40, kind  # the low-latency kernel has one rule and six sizes
        assert {r["world"] for r in rows} >= ({2, 3, 4, 8, 16} if kind in COLL else {1, 2, 3, 4, 8, 16}), kind
        assert {r["es"] for r in rows} == {2, 4}
        assert any(r["rh"] == 1 for r in rows) and any(r["rh"] == r["world"] > 1 for r in rows)
        # the low-latency kernel carries 512 KiB at most; a collective block is 16 B at least and
        # its first segment one slot at most
        want = sizes[:6] if kind == "ll" else sizes[2:12] if kind in COLL else sizes
        assert {r["n"] * r["es"] for r in rows} >= set(want), kind
        assert any(r["n"] == 1000003 for r in rows) or kind in COLL + ("ll",)
        grids = {tuple(r.get("knobs", {}).get(f, d) for f, d in (("grid", 512), ("default_grid", 512), ("size_grid", 1)))
                 for r in rows}
        assert grids >= {(512, 512, 1), (64, 512, 1), (1, 512, 1), (512, 512, 0), (64, 64, 1)}, kind

    def with_knob(kind, **kv):
        return [r for r in ROWS if r["kind"] == kind and all(r.get("knobs", {}).get(k) == v for k, v in kv.items())]

    for geom in (0, 1, 2):
        assert with_knob("twoshot", geom=geom)
    assert with_knob("twoshot", units_per_wg=1) and with_knob("twoshot", sub_max=2)
    assert with_knob("ring", ring_depth=2) and with_knob("ring_native", ring_grid=64)
    assert with_knob("threshold", th_oneshot_max=0) and with_knob("threshold", no_gate_shortcut=1)
    th = [dict(r, **dict(zip(GEO + TH, r["out"]))) for r in ROWS if r["kind"] == "threshold" and "out" in r]
    assert {tuple(r["th"]) for r in th} >= {(1.0, 1.0), (0.9, 0.8), (0.75, 0.75), (0.5, 0.5)}
    spec = [r for r in th if "spec" in r]
    assert {r["spec"]["order_ref"] for r in spec} == {0, 1}
    assert any(r["spec"]["block"] == 5 and r["spec"]["chunk"] == 2 and r["n"] == 10 for r in spec)
    assert any(r["n"] == MiB and r["spec"]["chunk"] == 4096 for r in spec)
    assert any(r["split"] and r["nch"] < r.get("knobs", {}).get("grid", 512) for r in spec)
    assert any(r["spec"]["split"] and not r["split"] for r in spec)
    assert any(r["spec"]["lag_skip"] and r["lag_skip"] for r in spec)
    assert any(r["spec"]["lag_skip"] and not r["lag_skip"] for r in spec)
    assert any(r["n"] <= (r["world"] - 1) * r["block"] for r in th)  # a short / empty last block
    assert any(r["oneshot"] for r in th) and any(r["full"] == 0 for r in th)
    throws = {r["throws"] for r in ROWS if "throws" in r}
    for prefix in ("XgmiComm: segment geometry exceeds slab", "allreduce_threshold: tensor exceeds one launch",
                   "allreduce_threshold: more than 4096 gather units", "round: more than 2048 chunks per workgroup",
                   "round: chunk must be > 0", "round: one rank per launch"):
        assert any(t.startswith(prefix) for t in throws), prefix
    assert any(r["kind"] == "ring" and "throws" in r for r in ROWS)  # the fp32 ring's partials exceed the slot


# Readable spot checks (defaults: grid 512 = 2 x 256 CUs, size grids on, 64 MiB slots).
SLOT = 64 * MiB


def default_knobs(world, rows=1, **kw):
    L = H.slab_layout(world, SLOT, rows - 1)
    return knobs(world=world, rows=rows, maxch=L["maxch"], slot_bytes=L["slot_bytes"], **kw)


def test_8_x_256_mib_bf16_two_shot_is_flat_at_the_full_grid():
    """profiles/round3/twoshot_geometry_ab.jsonl (README round 3): blocks of 2 MiB and more take
    the flat geometry - one chunk per workgroup, no reduce split, grouped scatter; 8 ranks x
    256 MiB is 2 GiB in the launch, so the full grid of 512 (profiles/round4 section 9)."""
    g = H.plan_allreduce("twoshot", default_knobs(8), 128 * MiB, 2, 8)
    assert g["gx"] * 8 == 512 and g["sub"] == 1 and g["subchunk"] == g["chunk"]
    assert g["nch"] == g["gx"] == 64 and g["chunk"] * 2 == 512 * KiB and g["sgroup"] == 8


def test_2_x_1_mib_two_shot_is_coarse():
    """Blocks under 2 MiB: ~one scatter unit per workgroup at the launch-size grid (2 MiB in the
    launch: 64 workgroups, 32 per rank), each chunk reduced in up to P - 1 pieces (no scatter
    groups: sgroup 0)."""
    g = H.plan_allreduce("twoshot", default_knobs(2), 512 * KiB, 2, 2)
    assert g["sgroup"] == 0 and g["nch"] == g["gx"] == 32 and g["sub"] == 1
    assert g["block"] == 256 * KiB and g["chunk"] == 8 * KiB


def test_reference_default_job_is_one_shot_in_one_workgroup():
    """The reference's default job (dataSize 10, maxChunkSize 2, 2 workers: block 5, 3 chunks;
    docs/PROTOCOL.md) runs the one-shot body of the threshold kernel in ONE workgroup."""
    L = H.slab_layout(2, 64 * KiB, 2, 0, 8)
    k = knobs(world=2, rows=3, maxch=L["maxch"], slot_bytes=L["slot_bytes"])
    p = H.plan_threshold(k, 10, 4, 1, 1.0, 1.0, block=5, chunk=2)
    assert (p["nch"], p["full"], p["oneshot"], p["gx"]) == (3, 1, 1, 1)
    assert (p["min_reduce"], p["min_complete"]) == (2, 6)


def test_grid_64_falls_back_from_one_shot_at_8_x_128_kib():
    """profiles/round6 section 12 (MXAR_GRID=64): 8 x 128 KiB full-threshold rounds need 128
    workgroups for the one-shot body's fast pass; a grid of 64 cannot hold them (need > cap), so
    the round takes the two-shot body at the whole grid. At the default grid it is one-shot."""
    small = H.plan_threshold(default_knobs(8, rows=3, grid=64, default_grid=64), 64 * KiB, 2, 1, 1.0, 1.0)
    assert (small["full"], small["oneshot"], small["gx"]) == (1, 0, 64)
    dflt = H.plan_threshold(default_knobs(8, rows=3), 64 * KiB, 2, 1, 1.0, 1.0)
    assert (dflt["full"], dflt["oneshot"], dflt["gx"]) == (1, 1, 128)
    assert small["nch"] == dflt["nch"] == 16
