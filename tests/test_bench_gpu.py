"""bench.py output contract (the driver parses it): stdout is exactly one JSON line with the
metric / value / config fields, the engine validated, and the DP-step section (BASELINE
configs 4 / 5) present without errors."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
def test_bench_prints_one_json_line_with_contract_fields(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    detail = tmp_path / "detail.json"
    # --full: the side sections asserted below run only with it
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--steps", "3", "--warmup", "1",
                        "--no-tune", "--no-rccl", "--no-threshold", "--no-collectives", "--no-fused-step", "--dp-timeout", "90",
                        "--detail-out", str(detail)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[:2000]
    assert len(lines[0].encode()) < 4096  # the driver parses the last line; long lines are truncated
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "bf16"
    assert d["engine_ok"] is True and d["validated_all"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0
    for k in ("model", "global_batch", "seq_len", "parallelism"):
        assert k in d["config"], k
    assert d["status"] == "ok" and d["config"]["algo"] == "copy (world=1)"
    assert d["detail"] == str(detail)
    for algo in ("twoshot", "ring", "ring_native"):  # [p50 ms, fraction of the copy roofline, ...]
        assert 0 < d["local_ranks"][algo][1] < 1.5, d["local_ranks"]
    assert d["protocol_us"]["validated"] is True, d["protocol_us"]

    full = json.loads(detail.read_text())  # everything else lives in the side file
    assert full["validated_max_abs_err"] == 0.0
    assert full["validated"] and all(full["validated"].values()), full.get("validation")
    assert full["topology"]["devices_visible"] >= 1
    loc = full["local_ranks"]
    assert "error" not in loc, loc
    for algo in ("twoshot", "ring", "ring_native"):
        assert loc[algo]["validated"] and 0 < loc[algo]["frac_copy_roofline"] < 1.5, loc
    proto = full["protocol"]  # the reference's master/worker protocol driving the GPU round engine
    assert "error" not in proto and proto["validated"] and proto["rounds_per_s"] > 0, proto
    for model in ("resnet50", "llama3_8b"):
        row = full["dp"][model]
        assert "error" not in row, row
        assert row["step_ms"] > 0 and row["compute_ms"] > 0
        # world = 1: no bandwidth figure for an allreduce that launches nothing
        assert "comm_algbw_per_rank" not in row and "note" in row


def _plain_run(cwd, *extra):
    """One plain (no --full) one-GPU run started in `cwd`; the parsed result line."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *extra],
                       cwd=cwd, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[:2000]
    return json.loads(lines[0])


@pytest.mark.timeout(120)
def test_plain_run_times_the_headline_only_and_dumps_its_output(tmp_path):
    """Without --full: the headline fields and nothing else, no side file, and --dump-outputs
    writes the last timed step's result. 32 MiB bf16 = 16 Mi elements, more than one rank's
    share of the dump, so the seeded sample path runs; at one rank the allreduce returns its
    input, which fill_uniform reproduces here from the bench's seed (rank 0: seed 0)."""
    import numpy as np
    import torch

    from akka_allreduce_1_amd.ops import fill_uniform
    from benchmarks.outputs import DUMP_ELEMS, dump_indices

    out = tmp_path / "out"
    d = _plain_run(tmp_path, "--steps", "4", "--warmup", "1", "--size-mib", "32", "--dump-outputs", str(out))
    assert d["metric"] == "allreduce_algbw" and d["unit"] == "GB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["steps"] == 4 and d["warmup"] == 1 and d["engine_ok"] is True
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx((32 << 20) / (d["ms_per_step"] / 1e3) / 1e9, rel=1e-2)
    for k in ("local_ranks", "lat_vs_size", "protocol_us", "stragglers", "dp", "adamw", "detail", "p50_ms"):
        assert k not in d, k
    assert [f.name for f in tmp_path.iterdir()] == ["out"]  # no side file next to the run
    assert [f.name for f in out.iterdir()] == ["allreduce_out_rank0.npy"]

    # the sample, checked without the code that drew it: head and tail kept whole, the rest
    # sorted indices strictly between them, spread evenly (16 bins of 393 216 expected draws
    # each, binomial sd 607: 5 % is 32 sd)
    n = (32 << 20) // 2
    idx = dump_indices(n, 1)
    q, m = DUMP_ELEMS // 4, DUMP_ELEMS // 2
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (DUMP_ELEMS,)
    assert torch.equal(idx[:q], torch.arange(q)) and torch.equal(idx[-q:], torch.arange(n - q, n))
    mid = idx[q:q + m]
    assert mid.min() >= q and mid.max() < n - q and bool((mid[1:] >= mid[:-1]).all())
    bins = torch.histc(mid.double(), bins=16, min=q, max=n - q)
    assert bins.min() > 0.95 * m / 16 and bins.max() < 1.05 * m / 16, bins
    assert torch.equal(idx, dump_indices(n, 1))  # the same in every run
    assert dump_indices(DUMP_ELEMS, 1) is None and dump_indices(DUMP_ELEMS // 2 + 1, 2) is not None

    got = np.load(out / "allreduce_out_rank0.npy")
    assert got.dtype == np.float32 and got.shape == (DUMP_ELEMS,)
    x = fill_uniform(torch.empty(n, dtype=torch.bfloat16, device="cuda"), seed=0)
    assert np.array_equal(got, x[idx.cuda()].float().cpu().numpy())


@pytest.mark.timeout(240)
def test_steps_sets_the_number_of_timed_steps(tmp_path):
    """ms_per_step is the timed window over --steps, so it must not depend on --steps: a step is
    one 256 MiB copy (about 0.09 ms), and the only fixed cost inside the window is one device
    synchronise (tens of us), 10 % of a step at 10 steps and 1 % at 100. A bench whose timed loop
    ran another number of steps than the --steps it divides by would be off by the ratio of the
    two step counts (10) in one of the runs; a factor 2 either way leaves room for a busy
    machine."""
    a = _plain_run(tmp_path, "--steps", "10", "--warmup", "5")
    b = _plain_run(tmp_path, "--steps", "100", "--warmup", "5")
    assert a["steps"] == 10 and b["steps"] == 100
    print("ms_per_step at 10 / 100 steps:", a["ms_per_step"], b["ms_per_step"])
    assert 0.5 < a["ms_per_step"] / b["ms_per_step"] < 2.0, (a["ms_per_step"], b["ms_per_step"])
