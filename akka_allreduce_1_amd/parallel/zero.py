"""Sharded data parallelism on the reference's two phases (ZeRO-2 style).

An allreduce is a reduce-scatter followed by an all-gather (the reference's ScatterBlock +
reduce, then ReduceBlock broadcast: AllreduceWorker.scala:194-251). Data-parallel training
does not need the second half for gradients: after the reduce-scatter every rank owns the
averaged gradient of 1/P of the parameters, so it can keep the optimizer state for that
1/P only, update its parameter shard, and all-gather the updated parameters. Same bytes on
the wire as an allreduce, 1/P of the optimizer memory and optimizer FLOPs per rank.

`ShardedDataParallel(model, comm, optimizer_factory)`:

* parameters are grouped into buckets of ~`bucket_bytes`; each bucket has ONE flat
  parameter buffer and ONE flat gradient buffer, and every `param.data` / `param.grad` is a
  view into them (sizes padded to a multiple of world x 16 B so shards stay aligned);
* a post-accumulate-grad hook launches a bucket's reduce-scatter (mean) on a side stream as
  soon as the bucket is complete - overlapped with the rest of backward;
* `step()` joins the side stream, runs the optimizer on the local shard views (one flat
  parameter per bucket: `optimizer_factory(list_of_shard_params)`), then all-gathers every
  bucket's updated shard back into the full flat parameter buffer.

`comm` needs `reduce_scatter(inp, out, op=)` and `all_gather(inp, out)` on the current stream:
`XgmiCommunicator` (one xGMI launch each, csrc/hip/xgmi_coll.hip) or `TorchDistComm` (RCCL /
gloo).

`fused_adamw={"lr": ..., "betas": ..., "eps": ..., "weight_decay": ...}` (XgmiCommunicator
only): every bucket's reduce-scatter, AdamW on the fp32 shard state and parameter all-gather
run as ONE launch per bucket at `step()` (csrc/hip/xgmi_adam.hip); `optimizer_factory` is
then unused (pass None) and the optimizer state is `self.adamw_states`.

`step_in_backward=True` (with `fused_adamw`, GPU): a bucket's fused step is launched on the
side stream the moment its last gradient is accumulated, so communication AND the optimizer
overlap the rest of backward ("optimizer in backward"). Valid because a parameter's
AccumulateGrad hook fires after its autograd node has used it; parameters shared between
layers (tied weights) must not be used with this mode. `comm_grid` sets the workgroup count
of the fused launches (0 = engine default).

`max_grad_norm=x` clips the mean gradient by its global L2 norm over all parameters and ranks
before the update (the formula of `torch.nn.utils.clip_grad_norm_`: coef = min(1, x / (norm +
1e-6))). `torch.nn.utils.clip_grad_norm_(model.parameters(), ...)` cannot do it here: `p.grad`
is a view of the un-reduced flat gradient. Unfused: after the reduce-scatter every rank takes
the sum of squares of its gradient shards, the per-rank sums are all-gathered and added in
rank order, and `grad_shard` is scaled before the optimizer runs. Fused: the step is split
where the norm has to be known (csrc/hip/xgmi_clip.hip) - per bucket one launch that
reduce-scatters into an fp32 shard `gshard` and sums its squares (from the gradient hooks on
the side stream when `overlap=True`), then the coefficient, then per bucket one launch that
runs AdamW on `gshard * coef` and all-gathers the parameters. `last_grad_norm` /
`last_clip_coef` are 0-d fp32 device tensors of the last step (an inf norm gives coef 0, a NaN
norm NaN everywhere); reading them costs no sync. Not with `step_in_backward`: an update
cannot precede a norm over gradients that do not exist yet.

`grad_accumulation=True` runs one optimizer step over several micro-batches: call
`accumulate()` after the backward of every micro-batch but the last and `step()` after the last.
The optimizer sees the SUM over micro-batches of the rank-mean gradient (torch's convention:
divide the loss by the number of micro-batches for a mean). torch's recipes (`no_sync()`, or a
second `backward()` before `step()`) do not apply: `p.grad` is a view of the un-reduced flat
gradient, a 16-bit one would be rounded at every micro-batch, and the bucket hooks launch a
bucket once until they are re-armed. Here every micro-batch is reduce-scattered when its backward ends and summed in fp32 on the
owned 1/P of the parameters (4 B per owned parameter), never in 16 bits. Fused: the accumulator
is `gshard`; the reduce-scatter half of csrc/hip/xgmi_clip.hip overwrites it for the first
micro-batch and adds into it after that (gshard = fl32(gshard + fl32(scale * sum)): the product
rounded before the add, no fma, so plain fp32 torch ops reproduce it), then - once per step -
the coefficient (a constant 1.0f when not clipping) and the update half. A step without
`accumulate()` runs exactly the launches it runs without the flag. Unfused: one fp32
accumulator per bucket the size of `grad_shard`; at `step()` `grad_shard` receives (sum * coef)
rounded once. Norm and coefficient are those of the accumulated gradient. `accumulate()` zeroes
the flat gradients itself; `zero_grad()` stays a between-steps call. Accumulators are scratch:
`state_dict()` raises between `accumulate()` and `step()`. Not with `step_in_backward`.

`loss_scale=` makes fp16 parameters trainable and makes a non-finite gradient harmless in every
element type: `loss_scale=<float>` is a static scale (`1.0`: only skip non-finite steps, the bf16
use), `loss_scale={"init_scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5,
"growth_interval": 2000}` a dynamic one (all keys optional, these are the defaults - those of
`torch.amp.GradScaler`, which cannot work here: `p.grad` is a view of the un-reduced flat gradient
and the fused path owns the optimizer), `loss_scale=True` dynamic with the defaults. Call
`zdp.scale_loss(loss).backward()` (one device multiply, no sync), then `step()` as ever. The step
is decided where the clipped step takes its norm: the ranks' sums of squares of the reduced
gradient are added in rank order, and the total is non-finite exactly when some reduced element
is. Then the step is skipped - parameters, optimizer state and the step count AdamW's bias
corrections use stay as they were, on every rank alike - and a dynamic scale backs off; otherwise
the gradient is multiplied by coef = clip / scale (rounded once) and the scale grows after
`growth_interval` clean steps. The rule is `loss_scale.scale_step_rule`. `loss_scale` (0-d fp32),
`last_step_skipped` (0-d integer), `skipped_steps` and `applied_steps` (counters; `applied_steps`
is AdamW's t) are device tensors; `last_grad_norm` is the norm of the UNSCALED gradient (inf or
NaN on a skipped step), `last_clip_coef` the clip coefficient; `stats["steps"]` keeps counting
`step()` calls. Works with `max_grad_norm`, with `grad_accumulation` (the scale changes only in
`step()`: every micro-batch of a step is scaled alike, and a non-finite value in any of them reaches
the accumulated shard and so the sum of squares), with both and with neither; not with
`step_in_backward` (the update would precede the decision). Fused: `loss_scale` forces the split
step, as `max_grad_norm` does - the one-launch `step_adamw` cannot know the decision before it
updates. Between the halves ONE one-wave launch (csrc/hip/xgmi_scale.hip) evaluates the rule on
the gathered records, updates scale and counters in place and writes a step record; every
bucket's update half reads coefficient, bias corrections and skip word from it, and a skipped
launch writes nothing. No host sync: `last_grad_norm`, `last_clip_coef` and `last_step_skipped` are
then views of that record, valid until the next `step()`. Unfused: the same rule in torch ops, and
ONE host sync per step (a `bool()` of the found flag) - torch optimizers have no device-side skip,
as `GradScaler` documents for non-fused optimizers. `state_dict()` gains `"loss_scale": {"scale",
"growth_tracker", "skipped"}` and its `"step"` is the applied count (reading them is one sync, at a
checkpoint); a checkpoint without the key loads into a loss-scaled instance (the configured initial
scale, every saved step applied), and one written without `loss_scale=` loads as it always did.
Limits: the decision is taken on the sum of squares, so a finite gradient whose squares overflow
fp32 is treated as an overflow - skipped, the scale backs off: conservative, and it corrects
itself; found flag and coefficient are per step over all buckets, not per bucket.
"""
from __future__ import annotations

from typing import Callable, Iterable

import torch

from . import loss_scale as _ls
from .comm import clip_coef_from_records, comm_stream, gather_sq_records, sq_record

_ALIGN_BYTES = 16


class _Bucket:
    def __init__(self, index: int, dtype: torch.dtype):
        self.index = index
        self.dtype = dtype
        self.params: list[torch.nn.Parameter] = []
        self.offsets: list[int] = []
        self.numel = 0
        self.nbytes = 0
        self.flat_param: torch.Tensor | None = None
        self.flat_grad: torch.Tensor | None = None
        self.grad_shard: torch.Tensor | None = None
        self.shard_param: torch.nn.Parameter | None = None
        self.pending = 0
        self.launched = False


class ShardedDataParallel:
    def __init__(self, module: torch.nn.Module | Iterable[torch.nn.Parameter], comm,
                 optimizer_factory: Callable[[list[torch.nn.Parameter]], torch.optim.Optimizer] | None, *,
                 bucket_bytes: int = 64 << 20, overlap: bool = True, fused_adamw: dict | None = None,
                 step_in_backward: bool = False, comm_grid: int = 0, max_grad_norm: float | None = None,
                 grad_accumulation: bool = False, loss_scale: float | dict | bool | None = None):
        params = module.parameters() if isinstance(module, torch.nn.Module) else module
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        if grad_accumulation and step_in_backward:
            raise ValueError("grad_accumulation cannot be combined with step_in_backward: the update of a bucket "
                             "would precede the gradients of the later micro-batches")
        self.grad_accumulation = bool(grad_accumulation)
        self.micro_batches = 0  # accumulate() calls since the last step()
        if max_grad_norm is not None and step_in_backward:
            raise ValueError("max_grad_norm cannot be combined with step_in_backward: the update of a bucket "
                             "would precede the norm over gradients that do not exist yet")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if loss_scale is not None and step_in_backward:
            raise ValueError("loss_scale cannot be combined with step_in_backward: the update of a bucket would "
                             "precede the decision whether the step is skipped")
        self._scale_cfg = None if loss_scale is None else _ls.LossScaleConfig(loss_scale)
        self.comm = comm
        self.world = int(getattr(comm, "world"))
        self.rank = int(getattr(comm, "rank"))
        self.device = self.params[0].device
        self.on_gpu = self.device.type == "cuda"
        self.stream = comm_stream(self.device) if self.on_gpu else None
        self.buckets = self._build(bucket_bytes)
        self.slot_of = {id(p): (b, off) for b in self.buckets for p, off in zip(b.params, b.offsets)}
        self.fused = dict(fused_adamw) if fused_adamw is not None else None
        # what has to be known over all buckets before any parameter moves: the scale rule (which clips too), the
        # clip coefficient, or nothing. A fused step that decides is split into two halves per bucket (_in_halves)
        self._decide = "scale" if self._scale_cfg is not None else "clip" if self.max_grad_norm is not None else None
        # overlap: a bucket is launched from its last gradient hook, on the side stream. The one-launch fused step
        # has no reduce half to overlap: there only step_in_backward launches from the hooks
        one_launch = self.fused is not None and self._decide is None
        self.overlap = bool(step_in_backward if one_launch else overlap) and self.on_gpu
        self.step_in_backward = bool(step_in_backward) and self.on_gpu
        self.adamw_states: list[dict] = []
        self._t = 0
        if self.fused is not None:
            self.fused["grid"] = int(comm_grid)
            if not hasattr(comm, "step_adamw"):
                raise ValueError("fused_adamw needs a communicator with step_adamw (XgmiCommunicator)")
            cap = comm.world * comm.slot_bytes
            for b in self.buckets:
                if b.nbytes > cap:
                    raise ValueError(f"fused_adamw: bucket of {b.numel} elements exceeds world * slot_bytes = {cap} B")
            self.adamw_states = [comm.adamw_state(b.flat_param) for b in self.buckets]
            if self._decide is not None or self.grad_accumulation:
                if not hasattr(comm, "step_adamw_shard"):
                    raise ValueError("fused_adamw with max_grad_norm, grad_accumulation or loss_scale needs a "
                                     "communicator with step_adamw_shard")
                # scratch, not in state_dict(): the fp32 gradient shard, also the accumulator over micro-batches
                self.gshards = [comm.gshard(b.flat_param) for b in self.buckets]
                self._sqs = [None] * len(self.buckets)
                self._one = torch.ones(1, dtype=torch.float32, device=self.device)  # coef of an unclipped step
            self.optimizer = None
        else:
            if step_in_backward:
                raise ValueError("step_in_backward needs fused_adamw")
            self.optimizer = optimizer_factory([b.shard_param for b in self.buckets])
            if self.grad_accumulation:  # scratch, not in state_dict(): fp32 sums over micro-batches
                self._accs = [torch.zeros(b.grad_shard.numel(), dtype=torch.float32, device=self.device)
                              for b in self.buckets]
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=self.device)
        self.last_clip_coef = torch.ones((), dtype=torch.float32, device=self.device)
        if self._scale_cfg is not None:
            self._init_loss_scale()
        self._t_started = False  # the one-launch step of this backward has taken its step number
        self._folding = False  # inside accumulate()
        self._side_used = False  # the side stream holds launches the current stream has not joined
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for p in self.params]
        self._next = 0
        self.stats = {"steps": 0, "reduce_scatter_bytes": 0, "all_gather_bytes": 0, "clip_bytes": 0}
        if self.grad_accumulation:
            self.stats["accumulates"] = 0

    # ------------------------------------------------------------------ layout
    def _build(self, bucket_bytes: int) -> list[_Bucket]:
        buckets: list[_Bucket] = []
        cur: dict[torch.dtype, _Bucket] = {}
        for p in reversed(self.params):  # backward produces the last layers first
            es = p.element_size()
            align = max(1, _ALIGN_BYTES // es)
            b = cur.get(p.dtype)
            if b is not None and b.numel > 0 and (b.numel + p.numel()) * es > bucket_bytes:
                b = None
            if b is None:
                b = _Bucket(len(buckets), p.dtype)
                buckets.append(b)
                cur[p.dtype] = b
            off = (b.numel + align - 1) // align * align
            b.params.append(p)
            b.offsets.append(off)
            b.numel = off + p.numel()
        for b in buckets:
            es = torch.empty(0, dtype=b.dtype).element_size()
            unit = self.world * max(1, _ALIGN_BYTES // es)  # every shard 16-B sized and aligned
            b.numel = (b.numel + unit - 1) // unit * unit
            b.nbytes = b.numel * es  # of the flat gradient and of the flat parameter: what a collective over it moves
            b.flat_param = torch.zeros(b.numel, dtype=b.dtype, device=self.device)
            b.flat_grad = torch.zeros(b.numel, dtype=b.dtype, device=self.device)
            for p, off in zip(b.params, b.offsets):
                view = b.flat_param[off:off + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = b.flat_grad[off:off + p.numel()].view_as(p)
            s = b.numel // self.world
            b.grad_shard = torch.zeros(s, dtype=b.dtype, device=self.device)
            shard = torch.nn.Parameter(b.flat_param[self.rank * s:(self.rank + 1) * s], requires_grad=True)
            shard.grad = b.grad_shard
            b.shard_param = shard
            b.pending = len(b.params)
        return buckets

    # ------------------------------------------------------------------ hooks
    def _on_grad(self, p: torch.Tensor) -> None:
        b, off = self.slot_of[id(p)]
        expect = b.flat_grad.data_ptr() + off * b.flat_grad.element_size()
        if p.grad is not None and p.grad.data_ptr() != expect:  # .grad was replaced: fold it back
            view = b.flat_grad[off:off + p.numel()].view_as(p)
            view.copy_(p.grad)
            p.grad = view
        b.pending -= 1
        if b.pending == 0 and self.overlap:
            self._launch_ready()

    def _launch_ready(self, all_: bool = False) -> None:
        while self._next < len(self.buckets) and (all_ or self.buckets[self._next].pending == 0):
            self._reduce(self.buckets[self._next])
            self._next += 1

    def _launch(self, side: bool, launch: Callable[[], None]) -> None:
        """`launch()` on the side stream, behind what the current stream holds so far, when `side`;
        else on the current stream. The caller says which: the split step's reduce halves go aside
        when `overlap`, the unfused reduce-scatter whenever there is a GPU (`on_gpu`), the one-launch
        fused step exactly when it is launched in backward."""
        if side:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.stream):
                launch()
            self._side_used = True
        else:
            launch()

    def _in_halves(self) -> bool:
        """Whether this backward's fused launches are the halves of the split step (reduce-scatter
        into gshard + squares; later coefficient, update + gather) and not the one-launch step: where
        a decision over all buckets precedes the update, and for every micro-batch of an accumulated
        step - gshard is the accumulator. A step without accumulate() stays the one-launch step."""
        return self._decide is not None or self._folding or self.micro_batches > 0

    def _reduce(self, b: _Bucket) -> None:
        """Bucket b's launch for this backward: the reduce-scatter, or all of the one-launch step."""
        if self.fused is None:
            self._launch(self.on_gpu, lambda: self.comm.reduce_scatter(b.flat_grad, b.grad_shard, op="avg"))
        elif self._in_halves():
            self._launch(self.overlap, lambda: self._rs_sq_half(b))
        else:
            if not self._t_started:  # first bucket of this backward: a new optimizer step
                self._t += 1
                self._t_started = True
            self._launch(self.step_in_backward, lambda: self.comm.step_adamw(
                b.flat_grad, b.flat_param, self.adamw_states[b.index], step=self._t, **self.fused))
            self.stats["all_gather_bytes"] += b.nbytes
        b.launched = True
        self.stats["reduce_scatter_bytes"] += b.nbytes

    def _rs_sq_half(self, b: _Bucket) -> None:
        """First half of the split step: reduce-scatter into gshard + sum of squares. The first
        micro-batch of a step overwrites gshard, later ones add into it."""
        gs, acc = self.gshards[b.index], self.micro_batches > 0
        self._sqs[b.index] = self.comm.reduce_scatter_sq(b.flat_grad, gs, op="avg", grid=self.fused["grid"],
                                                         accumulate=acc)
        if acc:
            self.stats["clip_bytes"] += 4 * gs.numel()  # the old sum, read back

    def _update_halves(self) -> None:
        """What the split step decides - the control kernel on the gathered sums of squares
        (loss-scaled), the clip coefficient, or the constant 1.0 of a merely accumulated step - then
        every bucket's update half: AdamW on gshard * coef and the all-gather. Loss-scaled, the half
        takes coefficient, bias corrections and skip word from the record, and a skipped one writes
        nothing (its bytes are counted all the same)."""
        if self._decide == "scale":
            self._applied_bound += 1
            self._table.ensure(self._applied_bound)
            self.comm.loss_scale_step(self._sqs, self._scale_state, self._record, self._table, self._scale_cfg,
                                      self.max_grad_norm)
            update, how = self.comm.step_adamw_record, {"record": self._record}
        else:
            coef = self._one
            if self._decide == "clip":
                self.last_grad_norm, coef = self.comm.clip_coef(self._sqs, self.max_grad_norm)
                self.last_clip_coef = coef
            self._t += 1
            update, how = self.comm.step_adamw_shard, {"coef": coef, "step": self._t}
        for b, st, gs in zip(self.buckets, self.adamw_states, self.gshards):
            update(gs, b.flat_param, st, **how, **self.fused)
            self.stats["all_gather_bytes"] += b.nbytes
            self.stats["clip_bytes"] += 8 * gs.numel()  # the fp32 shard: written once, read once

    def _torch_update(self) -> None:
        """The unfused update: grad_shard receives what the optimizer is to see - the folded sum,
        scaled where something is decided - then the optimizer runs on the shards and every bucket's
        shard is all-gathered. A skipped step (loss-scaled, non-finite) stops after the decision."""
        folded = self.micro_batches > 0
        if folded:
            self._add_shards()
        if self._decide is not None:
            if self._scale_shards():
                return
        elif folded:
            for b, acc in zip(self.buckets, self._accs):
                b.grad_shard.copy_(acc)
        self.optimizer.step()
        for b in self.buckets:
            # the shard is part of the gather's output buffer: gather from a copy
            self.comm.all_gather(b.shard_param.detach().clone(), b.flat_param)
            self.stats["all_gather_bytes"] += b.nbytes

    # ------------------------------------------------------------------ step API
    def _finish_backward(self) -> None:
        """Launch what the hooks have not - buckets whose parameters got no gradient included - and
        let the current stream join the side stream where this backward used it."""
        self._launch_ready(all_=True)
        if self._side_used:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            self._side_used = False

    def step(self) -> None:
        """Finish the gradient reduce-scatter, update the local shards, all-gather the
        parameters (call after backward)."""
        self._finish_backward()
        if self.fused is None:
            self._torch_update()
        elif self._in_halves():
            self._update_halves()  # else the one-launch step: its buckets have just been launched, or were in backward
        self._rearm()
        self.micro_batches = 0
        self.stats["steps"] += 1

    def _rearm(self) -> None:
        for b in self.buckets:
            b.pending = len(b.params)
            b.launched = False
        self._next = 0
        self._t_started = self._folding = False

    def accumulate(self) -> None:
        """End a micro-batch that is not the last of its optimizer step (call after its backward;
        `step()` ends the last): finish this backward's reduce-scatters - buckets that got no
        gradient included - into the fp32 accumulators (the first micro-batch of a step
        overwrites them, later ones add), zero the flat gradients (stream-ordered after the
        launches that read them: `zero_grad()` stays a between-steps call) and re-arm the
        gradient hooks. Needs `grad_accumulation=True`."""
        if not self.grad_accumulation:
            raise RuntimeError("accumulate() needs ShardedDataParallel(..., grad_accumulation=True)")
        self._folding = True  # the fused launches of this backward fold into gshard (_in_halves)
        self._finish_backward()
        if self.fused is None:
            self._add_shards()
        for b in self.buckets:
            b.flat_grad.zero_()
        self._rearm()
        self.micro_batches += 1
        self.stats["accumulates"] += 1

    def _add_shards(self) -> None:
        """Unfused accumulation: this micro-batch's reduce-scattered shard into the fp32 sum."""
        for b, acc in zip(self.buckets, self._accs):
            if self.micro_batches == 0:
                acc.copy_(b.grad_shard)
            else:
                acc.add_(b.grad_shard.float())

    def _scale_shards(self) -> bool:
        """The unfused decision: this rank's sum of squares over its gradient shards (fp32, bucket
        order; after accumulate() over the fp32 sums of the micro-batches), the ranks' sums
        all-gathered and added in rank order, the rule - clip_coef_from_records, or
        loss_scale.scale_step_rule with coef = clip / scale - and, unless the step is skipped,
        every shard times coef (after accumulate(): `grad_shard` receives sum * coef, rounded once
        to the parameter dtype). Returns whether the step is skipped: loss-scaled, that is the one
        host sync of the unfused path - torch optimizers cannot skip on the device."""
        folded = self.micro_batches > 0
        srcs = self._accs if folded else [b.grad_shard.float() for b in self.buckets]
        sqs = [s.pow(2).sum() for s in srcs]
        recs = gather_sq_records(self.comm, sq_record(sqs))
        if self._decide == "clip":
            self.last_grad_norm, coef = clip_coef_from_records(recs, self.max_grad_norm)
            self.last_clip_coef = coef
        else:
            self.last_grad_norm, self.last_clip_coef, coef, found = _ls.scale_step_rule(
                recs, self._scale_state, self._scale_cfg, self.max_grad_norm)
            self.last_step_skipped = found.to(torch.int32)
            if bool(found):
                return True
        for b, s in zip(self.buckets, srcs):
            if folded:
                b.grad_shard.copy_(s * coef)
            else:
                b.grad_shard.mul_(coef)
        return False

    # ------------------------------------------------------------------ loss scaling
    def _init_loss_scale(self) -> None:
        cfg = self._scale_cfg
        self._scale_state = _ls.new_state(cfg, self.device)  # int32 [4]: scale bits, tracker, applied, skipped
        self.loss_scale = _ls.scale_of(self._scale_state)
        self.applied_steps = self._scale_state[_ls.APPLIED]
        self.skipped_steps = self._scale_state[_ls.SKIPPED]
        self.last_step_skipped = torch.zeros((), dtype=torch.int32, device=self.device)
        self._applied_bound = 0  # host side: the applied count is at most this (no sync)
        if self.fused is not None:
            if not hasattr(self.comm, "step_adamw_record"):
                raise ValueError("fused_adamw with loss_scale needs a communicator with step_adamw_record")
            self._record = torch.zeros(_ls.REC_WORDS, dtype=torch.float32, device=self.device)
            self._record[_ls.REC_COEF] = 1.0
            self._table = _ls.CorrectionTable(self.device, self.fused.get("betas", (0.9, 0.999)))
            # views of the step record: what they show is the last step's until the next step() runs
            self.last_step_skipped = self._record[_ls.REC_SKIP:_ls.REC_SKIP + 1].view(torch.int32)[0]
            self.last_grad_norm = self._record[_ls.REC_NORM]
            self.last_clip_coef = self._record[_ls.REC_CLIP]

    def scale_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """loss * scale: one device multiply, no sync. Call backward() on the result."""
        if self._scale_cfg is None:
            raise RuntimeError("scale_loss() needs ShardedDataParallel(..., loss_scale=...)")
        return loss * self.loss_scale

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self) -> dict:
        """This rank's shard of the optimizer state, for resume (the reference
        checkpoints nothing; its master restarts at round 0). Parameters are not included -
        every rank holds them in full, so save `module.state_dict()` once. Tensors are
        references, as in `torch.optim.Optimizer.state_dict`; `torch.save` one file per rank
        and reload with `torch.load(..., weights_only=True)`."""
        if self.micro_batches > 0:
            raise RuntimeError(f"state_dict() between accumulate() and step(): {self.micro_batches} micro-batches "
                               "are held in accumulators, which are scratch and never checkpointed")
        sd = {"world": self.world, "rank": self.rank, "step": self._t, "steps": self.stats["steps"],
              "layout": [[b.numel, str(b.dtype), len(b.params)] for b in self.buckets]}
        if self._scale_cfg is not None:  # one sync, at a checkpoint
            _, tracker, applied, skipped = self._scale_state.tolist()
            sd["step"] = applied
            sd["loss_scale"] = {"scale": float(self.loss_scale), "growth_tracker": tracker, "skipped": skipped}
        if self.fused is not None:
            sd["adamw"] = [{k: st[k] for k in ("master", "exp_avg", "exp_avg_sq")} for st in self.adamw_states]
        else:
            sd["optimizer"] = self.optimizer.state_dict()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Resume from `state_dict()` of the same rank of a run with the same parameters,
        bucket_bytes, world size and optimizer kind."""
        layout = [[b.numel, str(b.dtype), len(b.params)] for b in self.buckets]
        if (sd.get("world"), sd.get("rank")) != (self.world, self.rank):
            raise ValueError(f"checkpoint of rank {sd.get('rank')}/{sd.get('world')}, this is {self.rank}/{self.world}")
        if [list(x) for x in sd.get("layout", [])] != layout:
            raise ValueError("checkpoint bucket layout differs (parameters or bucket_bytes changed)")
        if self.fused is not None:
            if "adamw" not in sd:
                raise ValueError("checkpoint has no fused AdamW state")
            for st, saved in zip(self.adamw_states, sd["adamw"]):
                for k in ("master", "exp_avg", "exp_avg_sq"):
                    if saved[k].shape != st[k].shape:
                        raise ValueError(f"{k}: shape {tuple(saved[k].shape)} != {tuple(st[k].shape)}")
                    st[k].copy_(saved[k])
        else:
            if "optimizer" not in sd:
                raise ValueError("checkpoint has no optimizer state")
            self.optimizer.load_state_dict(sd["optimizer"])
        self._t = int(sd["step"])
        self.stats["steps"] = int(sd["steps"])
        if self._scale_cfg is not None:
            # a checkpoint of a run without loss scaling: the configured initial scale, every step of it applied
            # (an unfused one counts them in "steps" alone: its optimizer keeps AdamW's own count)
            saved = sd.get("loss_scale", {"scale": self._scale_cfg.init_scale, "growth_tracker": 0, "skipped": 0})
            if "loss_scale" not in sd and self.fused is None:
                self._t = int(sd["steps"])
            fresh = torch.tensor([0, int(saved["growth_tracker"]), self._t, int(saved["skipped"])], dtype=torch.int32)
            fresh[:1].view(torch.float32).fill_(float(saved["scale"]))
            self._scale_state.copy_(fresh)
            self._applied_bound = self._t

    def zero_grad(self) -> None:
        for b in self.buckets:
            b.flat_grad.zero_()

    def remove_hooks(self) -> None:
        for h in self._hooks:
            h.remove()
        self._hooks = []

    def describe(self) -> list[dict]:
        rows = [{"bucket": b.index, "dtype": str(b.dtype), "params": len(b.params), "numel": b.numel,
                 "shard": b.numel // self.world,
                 "gshard_bytes": 4 * self.gshards[b.index].numel() if getattr(self, "gshards", None) else 0}
                for b in self.buckets]
        if self.grad_accumulation:  # the fp32 sums over micro-batches: gshard itself on the fused path
            for row, b in zip(rows, self.buckets):
                row["accum_bytes"] = row["gshard_bytes"] if self.fused is not None else 4 * self._accs[b.index].numel()
        return rows
