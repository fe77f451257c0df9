"""Loss scaling for `ShardedDataParallel`: the rule, in one place.

`scale_step_rule` is what a loss-scaled step decides once the ranks' sums of squares are known:
whether the step is skipped, the coefficient the gradient shard is multiplied by, the norm of the
unscaled gradient, and the scale's growth and backoff (`torch.amp.GradScaler`'s rule). Plain
torch ops on 0-d tensors, no host sync: the unfused path runs it as it stands, on any device,
and it is the reference the step-control kernel (csrc/hip/xgmi_scale.hip) is held to, bit for bit.

Inputs: `recs`, float64 [world, 2], the ranks' `sq_record`s in rank order (comm.py); the state
words. With S the fp32 scale before the step and inv = 1 / S in fp32:

    total = recs[0, 0] + recs[1, 0] + ...             float64, rank order
    found = not isfinite(total)
    norm  = fl32(sqrt(total)) * inv
    clip  = min(1, max_norm / (norm + 1e-6))          exactly 1.0f when not clipping
    coef  = clip * inv
    found:  S *= backoff_factor, tracker = 0, skipped += 1
    else:   tracker += 1; when tracker == growth_interval: S *= growth_factor, tracker = 0;
            applied += 1
    a static scale and its tracker never change

`clip` is evaluated as `clip_coef_from_records` always has (torch turns `x / tensor` into
`tensor.reciprocal() * x`), so with S = 1 norm, clip and coef are that function's bits, and with
any power-of-two S - every S the default factors can reach - they still are: multiplying by a
power of two is exact while nothing leaves the normal range.

Limits. The decision is taken on the sum of squares: a finite gradient whose squares overflow
fp32 counts as an overflow - the step is skipped and a dynamic scale backs off, which is
conservative and corrects itself. Found flag and coefficient are per step over all buckets.
"""
from __future__ import annotations

import torch

DEFAULTS = {"init_scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000}
# state words (int32; word 0 holds the fp32 scale's bits): csrc/hip/comm_args.h ScaleState
SCALE, TRACKER, APPLIED, SKIPPED = range(4)
# step record words (fp32; word 1 is an integer): csrc/hip/comm_args.h StepRecord
REC_COEF, REC_SKIP, REC_C1, REC_C2_SQRT, REC_NORM, REC_CLIP, REC_SHORT = range(7)
REC_WORDS = 8
TABLE_CAP = 1 << 21   # counts a correction table may hold (16 MiB): betas up to about 1 - 1e-5
TABLE_BLOCK = 4096    # counts filled per host-to-device copy


class LossScaleConfig:
    """`loss_scale=` of ShardedDataParallel, parsed: a float is a static scale, a dict (keys of
    DEFAULTS, all optional) or True a dynamic one."""

    def __init__(self, spec):
        self.dynamic = not isinstance(spec, (int, float)) or isinstance(spec, bool)
        if isinstance(spec, bool):
            if not spec:
                raise ValueError("loss_scale=False: pass None for no loss scaling")
            spec = {}
        if self.dynamic:
            if not isinstance(spec, dict):
                raise TypeError("loss_scale is a float (static), a dict or True (dynamic)")
            unknown = set(spec) - set(DEFAULTS)
            if unknown:
                raise ValueError(f"loss_scale: unknown keys {sorted(unknown)}; known: {sorted(DEFAULTS)}")
            cfg = {**DEFAULTS, **spec}
        else:
            cfg = {**DEFAULTS, "init_scale": spec}
        self.init_scale = float(cfg["init_scale"])
        self.growth_factor = float(cfg["growth_factor"])
        self.backoff_factor = float(cfg["backoff_factor"])
        self.growth_interval = int(cfg["growth_interval"])
        if not (self.init_scale > 0 and self.init_scale < float("inf")):
            raise ValueError("loss_scale: the scale must be positive and finite")
        if float(torch.tensor(self.init_scale, dtype=torch.float32)) != self.init_scale:
            raise ValueError("loss_scale: the initial scale must be an fp32 value (a power of two keeps the step's bits)")
        if self.dynamic and not (self.growth_factor > 1.0 and 0.0 < self.backoff_factor < 1.0
                                 and self.growth_interval >= 1):
            raise ValueError("loss_scale: growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")


def new_state(cfg: LossScaleConfig, device) -> torch.Tensor:
    """The scaler's four device words: [scale (fp32 bits), tracker, applied, skipped]."""
    st = torch.zeros(4, dtype=torch.int32, device=device)
    st[SCALE:SCALE + 1].view(torch.float32).fill_(cfg.init_scale)
    return st


def scale_of(state: torch.Tensor) -> torch.Tensor:
    """The 0-d fp32 view of the scale word."""
    return state[SCALE:SCALE + 1].view(torch.float32)[0]


def scale_step_rule(recs: torch.Tensor, state: torch.Tensor, cfg: LossScaleConfig, max_norm: float | None):
    """The rule of the module docstring on `recs` (float64 [world, 2]); updates `state` in place.
    Returns (norm, clip, coef, found): three 0-d fp32 tensors and a 0-d bool one."""
    total = recs[0, 0]
    for k in range(1, recs.shape[0]):
        total = total + recs[k, 0]
    found = ~torch.isfinite(total)
    scale = scale_of(state)
    inv = scale.reciprocal()
    norm = total.sqrt().to(torch.float32) * inv
    if max_norm is None:
        clip = torch.ones((), dtype=torch.float32, device=recs.device)
    else:
        clip = (float(max_norm) / (norm + 1e-6)).clamp(max=1.0)
    coef = clip * inv
    if cfg.dynamic:
        tracker = torch.where(found, 0, state[TRACKER] + 1).to(torch.int32)
        grow = tracker == cfg.growth_interval
        new_scale = torch.where(found, scale * cfg.backoff_factor, torch.where(grow, scale * cfg.growth_factor, scale))
        state[TRACKER] = torch.where(grow, 0, tracker).to(torch.int32)
        scale.copy_(new_scale)
    state[APPLIED] += (~found).to(torch.int32)
    state[SKIPPED] += found.to(torch.int32)
    return norm, clip, coef, found


class CorrectionTable:
    """AdamW's bias corrections (c1, c2_sqrt) by step count, on the device, with the host's bits:
    the fused step computes them on the host in fp32 with std::pow, and the device's powf need
    not round alike, so a step that takes its count from the device looks them up here. Entry
    t - 1 belongs to count t. Filled with the host's own formula in blocks, ahead of the largest
    count the next step can reach (`ensure`): one small stream-ordered copy per block. The table
    ends at `end`, the first count where both are exactly 1.0f; the kernel clamps its index there."""

    def __init__(self, device, betas):
        from .._native import C

        self._h = C.hip
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])
        self.end = int(self._h.adamw_corrections_end(self.beta1, self.beta2, TABLE_CAP + 1))
        if self.end > TABLE_CAP:
            raise ValueError(f"loss_scale: betas {betas} keep a bias correction below 1 for more than {TABLE_CAP} "
                             "steps, more than the device table holds")
        self.tensor = torch.ones(2 * self.end, dtype=torch.float32, device=device)
        self.filled = 0

    def ensure(self, count: int) -> None:
        """Entries up to `count` (clamped to the end) are on the device once the current stream
        gets there."""
        want = min(max(int(count), 1), self.end)
        while self.filled < want:
            n = min(TABLE_BLOCK, self.end - self.filled)
            blk = torch.tensor(self._h.adamw_corrections(self.beta1, self.beta2, self.filled + 1, n), dtype=torch.float32)
            self.tensor[2 * self.filled:2 * (self.filled + n)].copy_(blk)
            self.filled += n
