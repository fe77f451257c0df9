"""bench.py --dump-outputs: the result of the last timed step, written so that two builds of
the project can be compared output for output.

Each rank writes its own output buffer (what the caller of the timed allreduce holds) as
float32 to DIR/allreduce_out_rank<k>.npy. All ranks' files together stay under DUMP_ELEMS
elements (48 MiB): a buffer larger than the rank's share is sampled at fixed indices.
"""
from __future__ import annotations

import os

import torch

DUMP_ELEMS = 12 << 20  # float32 elements over all ranks' files


def dump_indices(n: int, world: int) -> torch.Tensor | None:
    """Which elements of an n-element output are kept: all of them (None) if they fit the
    rank's share of DUMP_ELEMS, else the first and last quarter of the share and, for the other
    half, seeded random indices in between (the same in every run and on every rank)."""
    share = DUMP_ELEMS // world
    if n <= share:
        return None
    q = share // 4
    g = torch.Generator().manual_seed(20240607)
    mid = torch.randint(q, n - q, (share - 2 * q,), generator=g).sort().values
    return torch.cat([torch.arange(q), mid, torch.arange(n - q, n)])


def dump_outputs(path: str, y: torch.Tensor, rank: int, world: int) -> str:
    import numpy as np

    idx = dump_indices(y.numel(), world)
    s = y if idx is None else y[idx.to(y.device)]
    os.makedirs(path, exist_ok=True)
    out = os.path.join(path, f"allreduce_out_rank{rank}.npy")
    np.save(out, s.float().cpu().numpy())
    return out
