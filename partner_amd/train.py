"""Training step of the nuScenes polar-pillar model on the HIP kernels.

Host mirror of the reference's training iteration
  Trainer.train / batch_processor_inline   det3d/torchie/trainer/trainer.py:446-501, 414-444
  parse_second_losses                      det3d/torchie/trainer/trainer.py:116-137
  DistOptimizerHook / allreduce_grads      det3d/core/utils/dist_utils.py:51-57, 31-42
  OptimizerHook.clip_grads                 det3d/torchie/trainer/hooks/optimizer.py:10-13
  OptimWrapper.step + OneCycle             det3d/solver/fastai_optim.py:155-171,
                                           det3d/solver/learning_schedules_fastai.py:77-95
without autograd: forward in training mode (batch-statistics BatchNorm), the CenterPoint loss, an
explicit backward through every layer of  DynamicPFNet -> DynamicPPScatter -> RPN ->
CenterHeadSinglePos  and one fused clip + decoupled-weight-decay + Adam update over a flat fp32
parameter buffer.  All arithmetic runs in kernels of libpartner_hip; PyTorch allocates tensors and
(for world_size > 1) all-reduces the flat gradient buffer through torch.distributed (RCCL).

The step is made of parts: ``ParamStore`` (the flat buffers), a neck part (``RpnTrain`` here, ``train_stream.ContextNeckTrain`` / ``TrailingEdgeNeckTrain``, ``train_strobe.UberNeckTrain``), the head
part (``train_head.CenterHeadTrain``), the seg head (``seg_heads.SegHeadTrain``) and ``FlatAdam`` (schedule, clip, Adam, checkpoint); the
layer wrappers they are built from are in ``train_layers``.

The module's parameters are re-bound to views of the flat buffer, so ``state_dict()`` keeps the
reference's keys and the inference path (after ``PlanCache`` invalidation) sees the trained weights.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import torch
from torch import nn

from . import hip, ops
from .routes import R
from .heads import CenterHeadSingle
from .readers import DynamicPFNet
from .train_head import CenterHeadTrain
from .train_layers import _ConvBNReLU, _PillarConv      # (_PillarConv: tests import it from here)


def one_cycle(step: int, total_step: int, lr_max: float, moms: Sequence[float], div_factor: float, pct_start: float):
    """(lr, beta1) the OneCycle scheduler sets before optimizer step ``step`` (0-based);
    learning_schedules_fastai.py:52-95 (the last phase whose start has been reached wins)."""
    a1 = int(total_step * pct_start)
    low = lr_max / div_factor

    def cos(start, end, pct):
        return end + (start - end) / 2 * (math.cos(math.pi * pct) + 1)

    if step >= a1:
        pct = (step - a1) / (total_step - a1)
        return cos(lr_max, low / 1e4, pct), cos(moms[1], moms[0], pct)
    pct = step / a1
    return cos(low, lr_max, pct), cos(moms[0], moms[1], pct)


def seg_loss_scale_value(seg_loss_decay) -> float:
    """the trainer's ``seg_loss_decay`` (trainer.py:116-126) as the host factor of the seg loss.  Only the static, non-negative mode is
    built: the dynamic mode (a negative value: the factor follows the ratio of the two losses) needs the losses on the host."""
    v = float(seg_loss_decay)
    if not v >= 0.0:
        raise ValueError(f"seg_loss_scale must be a non-negative float (got {seg_loss_decay}); the trainer's dynamic mode (negative "
                         "seg_loss_decay, trainer.py:116-126) needs a readback of the losses and is not built")
    return v


class ParamStore:
    """All trainable parameters of a module in ONE flat fp32 buffer (+ flat grad / Adam moments);
    every parameter starts on a 16-byte boundary.  The flat gradient buffer is what gets all-reduced
    (one collective per step, dist_utils.py:8-28 coalesces the same way)."""

    def __init__(self, model: nn.Module, device, order_key=None):
        """``order_key(name) -> sortable``: position of a parameter in the flat buffer (default: named_parameters order);
        the training step orders the buffer by the time a gradient is complete in backward, so that a gradient bucket is one
        contiguous range"""
        self.names: List[str] = []
        self.offsets: Dict[str, Tuple[int, torch.Size]] = {}
        off = 0
        named = list(model.named_parameters())
        if order_key is not None:
            named.sort(key=lambda kv: order_key(kv[0]))   # stable: ties keep the module order
        for name, p in named:
            self.names.append(name)
            self.offsets[name] = (off, p.shape)
            off += (p.numel() + 3) // 4 * 4
        self.total = off
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_m = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_v = torch.zeros(off, dtype=torch.float32, device=device)
        self.side = ops.SideStream(device)
        self.fresh = None            # token of the iteration whose packed weights were refreshed ahead (PolarPillarTrainStep._prepack)
        self.convs: List[object] = []   # the step's convolution wrappers (prepack_fwd / prepack_bwd), in construction order
        self.p: Dict[str, torch.Tensor] = {}
        self.g: Dict[str, torch.Tensor] = {}
        for name, p in model.named_parameters():
            o, shape = self.offsets[name]
            view = self.flat_p[o:o + p.numel()].view(shape)
            view.copy_(p.detach().to(device=device, dtype=torch.float32))
            p.data = view
            self.p[name] = view
            self.g[name] = self.flat_g[o:o + p.numel()].view(shape)


def invalidate_inference_plans(model: nn.Module) -> None:
    """the kernels update the parameters behind PyTorch's version counters: drop the packed-weight plans of the
    inference path (f32 and bf16) so that the next eval forward re-packs from the trained weights"""
    for m in model.modules():
        for attr in ("_plan", "_plan_bf16"):
            pc = getattr(m, attr, None)
            if pc is not None and hasattr(pc, "plan"):
                pc.plan = None


def optimizer_state(ps: ParamStore, it: int, sched: dict) -> Dict[str, object]:
    """Adam moments of the flat buffer + where every parameter lives in it (names, offsets, sizes): a checkpoint is independent
    of the ORDER of the buffer (the reference keeps optimizer state per parameter, det3d/torchie/trainer/trainer.py:342-372)"""
    return dict(iter=it, exp_avg=ps.flat_m.clone(), exp_avg_sq=ps.flat_v.clone(), names=list(ps.names),
                offsets=[int(ps.offsets[n][0]) for n in ps.names], numels=[int(ps.offsets[n][1].numel()) for n in ps.names],
                schedule=dict(sched))


def load_optimizer_state(ps: ParamStore, state: Dict[str, object]) -> int:
    """restore the moments BY NAME: a checkpoint written with another layout of the flat buffer (e.g. before the buffer was
    ordered by backward completion) loads as long as it holds the same parameters; returns the iteration count"""
    names = list(state["names"])
    if sorted(names) != sorted(ps.names):
        raise ValueError("optimizer state belongs to a model with different parameters")
    if names == list(ps.names) and state["exp_avg"].numel() == ps.total and "offsets" not in state:
        ps.flat_m.copy_(state["exp_avg"])       # same order, legacy checkpoint without the offset table
        ps.flat_v.copy_(state["exp_avg_sq"])
        return int(state["iter"])
    if "offsets" in state:
        offs, nums = list(state["offsets"]), list(state["numels"])
    else:   # legacy checkpoint (names only): parameters were laid out in the saved order, each on a 4-float boundary
        nums = [int(ps.offsets[n][1].numel()) for n in names]
        offs, o = [], 0
        for k in nums:
            offs.append(o)
            o += (k + 3) // 4 * 4
    m_src, v_src = state["exp_avg"], state["exp_avg_sq"]
    for n, o, k in zip(names, offs, nums):
        dst, shape = ps.offsets[n]
        if shape.numel() != k:
            raise ValueError(f"optimizer state: parameter {n} has {k} elements in the checkpoint, {shape.numel()} in the model")
        ps.flat_m[dst:dst + k].copy_(m_src[o:o + k])
        ps.flat_v[dst:dst + k].copy_(v_src[o:o + k])
    return int(state["iter"])


class FlatAdam:
    """The optimizer of every training step: OneCycle schedule, gradient-norm clip, decoupled weight decay and Adam in one fused update over
    the flat buffers of a ``ParamStore``; checkpoint / resume of its state (the reference saves model + optimizer state per epoch,
    det3d/torchie/trainer/trainer.py:342-372) and the broadcast of the initial parameters."""

    def __init__(self, ps: ParamStore, model: nn.Module, total_steps: int, lr_max, moms, div_factor, pct_start, weight_decay, max_norm, beta2, eps):
        self.ps, self.model = ps, model
        self.sched = dict(total=total_steps, lr_max=lr_max, moms=tuple(moms), div=div_factor, pct=pct_start)
        self.wd, self.max_norm, self.beta2, self.eps = weight_decay, max_norm, beta2, eps
        self.iter = 0

    def step(self):
        s, ps = self.sched, self.ps
        lr, beta1 = one_cycle(self.iter, s["total"], s["lr_max"], s["moms"], s["div"], s["pct"])
        total_norm = ops.grad_norm(ps.flat_g)
        ops.adam_step(ps.flat_p, ps.flat_g, ps.flat_m, ps.flat_v, self.iter + 1, lr, beta1, self.beta2, self.eps,
                      self.wd, total_norm=total_norm, max_norm=self.max_norm)
        self.iter += 1
        invalidate_inference_plans(self.model)   # the kernels updated the parameters behind the plans' packed copies (f32 and bf16)
        return total_norm

    def state_dict(self) -> Dict[str, object]:
        """optimizer-side state; the parameters themselves are in ``model.state_dict()`` (views of the flat buffer)"""
        return optimizer_state(self.ps, self.iter, self.sched)

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.iter = load_optimizer_state(self.ps, state)
        self.sched.update(state.get("schedule", {}))
        invalidate_inference_plans(self.model)

    def sync_initial_params(self, force=False):
        """rank 0's parameters (and floating-point buffers: BatchNorm running statistics) to every rank, once before the first step
        -- what DistributedDataParallel's constructor does in the reference (det3d/torchie/apis/train.py:330-336)"""
        from .dist_utils import broadcast_flat_params
        broadcast_flat_params(self.ps.flat_p, force=force)
        for b in self.model.buffers():
            if b.dtype.is_floating_point:
                broadcast_flat_params(b, force=force)


class OptimizerForwards:
    """the optimizer's surface on a step object (``self.opt``: a FlatAdam)"""
    iter = property(lambda self: self.opt.iter)
    sched = property(lambda self: self.opt.sched)

    def optimizer_step(self):
        return self.opt.step()

    def state_dict(self) -> Dict[str, object]:
        return self.opt.state_dict()

    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.opt.load_state_dict(state)


def flat_order_key(up0: int):
    """-> ``order_key(name)``, the position of a parameter in the step's flat buffer = the reverse of the order in which backward completes
    the gradients: reader | block 0 (+ its deblock) | memory 1 | block 1 (+ its deblock) | ... | seg head | bbox head.  ``up0``: the neck's
    first block with a deblock.  RPNUber's ``neck.memory{i}`` sits in front of block i: its backward runs behind block i's and before
    block i - 1's (and that block's deblock), so its gradients are queued before ``block_done(i - 1)``.  Models without memory modules
    keep the order they had."""

    def order_key(name: str):
        parts = name.split(".")
        if parts[0] == "reader":
            return 0
        if parts[0] == "neck" and parts[1] == "blocks":
            return 1 + 2 * int(parts[2])
        if parts[0] == "neck" and parts[1] == "deblocks":
            return 2 + 2 * (int(parts[2]) + up0)
        if parts[0] == "neck" and parts[1].startswith("memory") and parts[1][6:].isdigit():
            return 2 * int(parts[1][6:]) + 0.5
        return 1000 if parts[0] == "bbox_head" else 999

    return order_key


class RpnTrain:
    """The RPN (det3d/models/necks/rpn.py:144-159) in training form over a ``ParamStore``: a neck part of the step.
      ``forward(canvas, nsectors, **sweep)`` -> the concatenated deblock outputs (this neck: one sector, no sweep arguments)
      ``backward(d_x2, block_done)``       -> the gradient of the canvas, or of the pillar features with a ``sparse_first`` layer;
                                              ``block_done(i)`` once the parameter gradients of block i (and its deblock) are queued
      ``sparse_first``                     the first convolution when it runs on the pillar rows (then no dense canvas exists), else None
      ``early_convs()``                    the wrappers whose forward layouts the main stream takes before it waits for pack event 1
      ``block_out``                        the blocks' outputs of the last forward
    ``wait_packs(k)``: the step's wait for pack event k (PolarPillarTrainStep._prepack)."""

    def __init__(self, ps: ParamStore, neck: nn.Module, wait_packs=lambda k: None):
        self.wait_packs = wait_packs
        self.blocks: List[List[_ConvBNReLU]] = []
        self.sparse_first = None
        for i, blk in enumerate(neck.blocks):
            mods = list(blk._modules.values())
            layers = [_ConvBNReLU(ps, f"neck.blocks.{i}.", 1, mods[2], mods[1])]
            if i == 0 and R.train_pillar_conv and ops.PillarConvLayer.supports(mods[1].weight, mods[1].stride[0], mods[1].groups) and mods[1].out_channels <= 128 \
                    and mods[1].out_channels in (32, 64, 128):
                layers[0].conv = self.sparse_first = _PillarConv(ps, f"neck.blocks.{i}.1.weight", mods[1].stride[0])
            for k in range(4, len(mods), 3):
                layers.append(_ConvBNReLU(ps, f"neck.blocks.{i}.", k, mods[k + 1], mods[k]))
            self.blocks.append(layers)
        self.deblocks = [_ConvBNReLU(ps, f"neck.deblocks.{j}.", 0, de[1], de[0]) for j, de in enumerate(neck.deblocks)]
        self.up_start = neck._upsample_start_idx
        self.up_filters = list(neck._num_upsample_filters)
        self.block_out: List[torch.Tensor] = []

    def early_convs(self):
        """block 0 and the deblock fed by block 0"""
        first = [layer.conv for layer in self.blocks[0]]
        return first + ([self.deblocks[0].conv] if self.up_start == 0 and self.deblocks else [])

    def forward(self, canvas, nsectors=1):
        """canvas (batch, T, R, C) -> the concatenated deblock outputs; keeps what ``backward`` needs"""
        assert nsectors == 1
        x = canvas
        out, off = None, 0
        self.block_out = []
        for i, layers in enumerate(self.blocks):
            if i < 2:
                self.wait_packs(i)
            for layer in layers:
                x = layer.fwd(x)
            self.block_out.append(x)
            j = i - self.up_start
            if j >= 0:
                de = self.deblocks[j]
                if out is None:
                    oh, ow = de.conv.layer.out_hw(x.shape[1], x.shape[2])
                    out = torch.empty((canvas.shape[0], oh, ow, sum(self.up_filters)), dtype=torch.float32, device=canvas.device)
                de.fwd(x, out=out, out_co=off)
                off += self.up_filters[j]
        self.wait_packs(1)    # models with a single block reach the head without having met event 1 in the loop
        return out

    def backward(self, d_x2, block_done=None):
        d_block = None
        for i in range(len(self.blocks) - 1, -1, -1):
            j = i - self.up_start
            if j >= 0:
                off = sum(self.up_filters[:j])
                if d_block is None:
                    d_block = self.deblocks[j].bwd(d_x2, dout_co=off)
                else:
                    self.deblocks[j].bwd(d_x2, dout_co=off, dx=d_block, accumulate=True)
            for layer in reversed(self.blocks[i]):
                d_block = layer.bwd(d_block)
            if block_done is not None:
                block_done(i)
        return d_block


class PolarPillarTrainStep(OptimizerForwards):
    """One training iteration of PointPillars(DynamicPFNet, DynamicPPScatter, RPN, CenterHeadSinglePos).

    ``step(points, sample_offsets, batch, targets)`` runs forward (train mode), loss, backward, gradient
    all-reduce (if torch.distributed is initialised with world_size > 1), clip + decoupled wd + Adam with
    the OneCycle schedule, and returns the loss vector [det, hm, loc, num_pos, elem...] (device)."""

    nsec = 1      # sectors per sweep (the streaming step: the model's)
    # what tests and tools/determinism_check.py read of the neck part under the step's own names
    blocks = property(lambda self: self.neck_train.blocks)
    block_out = property(lambda self: self.neck_train.block_out)

    def __init__(self, model: nn.Module, total_steps: int, lr_max=0.005, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4,
                 weight_decay=0.01, max_norm=35.0, beta2=0.99, eps=1e-8, neck_part=RpnTrain):
        self.model = model
        reader, neck, head = model.reader, model.neck, model.bbox_head
        if not isinstance(reader, DynamicPFNet):
            raise NotImplementedError("training step: the reader must be a DynamicPFNet")
        if not (isinstance(head, CenterHeadSingle) or type(head).__name__ == "CenterHead"):
            raise NotImplementedError("training step: the head must be CenterHead, CenterHeadSingle or CenterHeadSinglePos")
        reader._check_supported()
        dev = next(model.parameters()).device
        hip.require_device(next(model.parameters()))
        self.dev = dev
        # flat-buffer order = reverse of the order in which backward completes the gradients: reader | block 0 (+ its deblock)
        # | block 1 ... | head, so that the buckets of the gradient exchange (head first) are contiguous ranges
        order_key = flat_order_key(neck._upsample_start_idx)
        self.ps = ps = ParamStore(model, dev, order_key)
        # gradient buckets [lo, hi) in the order backward completes them: the head, the last RPN block (+ deblock), the rest
        first_head = min((ps.offsets[n][0] for n in ps.names if n.startswith("bbox_head.")), default=ps.total)
        self.last_block = len(neck.blocks) - 1
        first_last = min((ps.offsets[n][0] for n in ps.names if order_key(n) >= 1 + 2 * self.last_block), default=first_head)
        self.buckets = [b for b in ((first_head, ps.total), (first_last, first_head), (0, first_last)) if b[1] > b[0]]
        # ---- seg super-task (point_pillars.py:99-103): the head's parameters sort between the RPN and the bbox head (order_key 999), i.e. into
        # the second gradient bucket
        self.seg = self.seg_loss = None
        seg_head = getattr(model, "seg_head", None)
        if seg_head is not None:
            from .seg_heads import SegHeadTrain
            if seg_head.loss_func is None:
                raise ValueError("training step: the seg head was built without a loss")
            self.seg = SegHeadTrain(seg_head, ps.p["seg_head.conv.weight"], ps.p["seg_head.conv.bias"], ps.g["seg_head.conv.weight"],
                                    ps.g["seg_head.conv.bias"], side=ps.side)
        self._seg_labels = self._point_labels = None
        self.opt = FlatAdam(ps, model, total_steps, lr_max, moms, div_factor, pct_start, weight_decay, max_norm, beta2, eps)
        self.exchange_enabled = True         # bench.py sets False for its timing-only mode: the same iteration without the collectives (ranks diverge)
        self.exchange_at_world_1 = False     # tests/test_hip_rccl.py sets True: the collectives run over a ONE-rank group too (dist_utils.init(single_rank_group=True))
        self.broadcast_buffers = True        # a caller sets False to drop DDP's per-iteration broadcast of rank 0's BatchNorm statistics (dist_utils.BufferSync)
        self._exchange = self._bufsync = None
        self._iter_start = torch.cuda.Event()
        self._pack_ev = [torch.cuda.Event() for _ in range(3)]
        self._pack_events = None             # the three events while an iteration's packs run on the side stream
        self.reader = reader
        self.spec = ops.GridSpec.from_range(reader.pc_range, reader.voxel_size)
        self.w0, self.w1 = "reader.pfn_layers.0.linear.weight", "reader.pfn_layers.1.linear.weight"
        self.vi = None
        self.neck_train = neck_part(ps, neck, self._packs_ready)
        self.head_train = CenterHeadTrain(ps, head, dev)

    # ------------------------------------------------------------------------------------------
    def _index(self, points, sample_offsets, batch, grid_ind):
        """-> the VoxelIndex of one sweep (``grid_ind`` given: the dataset's cell indices instead of the device's own)"""
        if grid_ind is None:
            _, keys = ops.grid_index(points, sample_offsets, batch, self.spec, want_grid_ind=False)
            n_dev = sample_offsets[batch:]
        else:
            keys = ops.keys_from_grid_ind(grid_ind.to(torch.int64).contiguous(), self.spec, batch)
            n_dev = None
        return ops.build_voxel_index(keys, self.spec, batch, n_dev=n_dev, want_unq=False, sorted_runs=True)

    def _canvas(self, points, vi, batch, sparse_first=None):
        """reader + scatter of one sweep.  With the pillar-rows first layer only the pillars' cells of the canvas are ever read: no
        134 MB-per-sample zero fill"""
        ps, r, spec = self.ps, self.reader, self.spec
        canvas = torch.empty((batch, spec.grid[1], spec.grid[0], r.out_channels), dtype=torch.float32, device=self.dev)
        if sparse_first is not None:
            sparse_first.vi = vi
        else:
            hip.call("pn_fill_zero", canvas.data_ptr(), canvas.numel() * 4, hip.stream())
        ops.dynamic_pfn(points, vi, ps.p[self.w0], ps.p[self.w1], r.vx, r.vy, r.x_offset, r.y_offset, None, canvas, voxel_shape=r.voxel_shape)
        return canvas

    def _forward(self, points, sample_offsets, batch, grid_ind, prev_sweep):
        spec = self.spec
        self.vi = self._index(points, sample_offsets, batch, grid_ind)
        if self._point_labels is not None:
            # the seg targets from the iteration's own index: per cell the majority of its points' labels, as the loss's int32 label - 1
            # (-1 = ignore) -- no int64 voxel_labels map, no get_labels pass
            self._seg_labels = ops.voxel_labels_from_points(self._point_labels, self.vi, dense=False, loss_labels=True).view(
                batch, spec.grid[1], spec.grid[0])
        self.points = points
        first = self.neck_train.sparse_first
        canvas = self._canvas(points, self.vi, batch, first)
        self._prepack()     # issued behind the scatter stage's launches, runs beside them
        sweep = {}
        if prev_sweep is not None:
            # the previous sweep: reader + scatter with nothing kept (polarstream.py:318-336, under no_grad); the neck warps its maps
            pv = self._index(prev_sweep["points"], None, batch, prev_sweep["grid_ind"])
            sweep = dict(prev_canvas=self._canvas(prev_sweep["points"], pv, batch),
                         warp=lambda inputs: self.model.warp_prev_strips(inputs, prev_sweep["transform_matrix"], batch // self.nsec))
        x2 = self.neck_train.forward(canvas, self.nsec, **sweep)
        self.seg_logits = None
        if self._seg_labels is not None:
            # the pillar-features first layer builds no dense canvas: the canvas part of the logits is computed on the pillar rows
            self.seg_logits = self.seg.forward(canvas, x2, vi=self.vi if first is not None else None)
        return self.head_train.forward(x2)

    def _backward(self, targets, losses, grad_scale: float, seg_dlogits=None):
        ps = self.ps
        d_x2 = self.head_train.backward(targets, losses, grad_scale)
        if seg_dlogits is not None:
            # seg head: its RPN half joins d_x2 before the RPN's backward starts; all its parameter gradients (second bucket) are queued here
            self.seg.backward_x2(seg_dlogits, d_x2)
            self.seg.backward_x1(seg_dlogits, need_dx=False)
        self._bucket_ready(0)   # every head gradient is queued: its exchange overlaps the backward of the neck

        def block_done(i):
            # a bucket is ready only once its gradients are complete (the streaming neck: after sector 0's backward)
            if i == self.last_block and len(self.buckets) > 2:
                self._bucket_ready(1)

        d_block = self.neck_train.backward(d_x2, block_done=block_done)
        r = self.reader
        sparse = self.neck_train.sparse_first is not None      # then d_block is d(pillar features) (n_cap, C), not a canvas gradient
        if seg_dlogits is not None:
            self.seg.backward_canvas(seg_dlogits, d_block)      # the seg head's canvas half: d_canvas, or d_features at the pillar rows
        ops.dynamic_pfn_bwd(self.points, self.vi, ps.p[self.w0], ps.p[self.w1], r.vx, r.vy, r.x_offset, r.y_offset,
                            d_features=d_block if sparse else None, d_canvas=None if sparse else d_block, dw0=ps.g[self.w0], dw1=ps.g[self.w1],
                            voxel_shape=r.voxel_shape)
        ps.side.join()

    def _bucket_ready(self, k: int) -> None:
        """start the SUM all-reduce of gradient bucket k (asynchronous: RCCL's stream waits for the kernels queued so far and
        runs next to the rest of backward; the reference's DDP reducer does the same per bucket, det3d/torchie/apis/train.py:330-336)"""
        if self._exchange is not None:
            self.ps.side.join()      # the bucket's weight gradients are computed on the side stream
            self._exchange.ready(k)

    # ------------------------------------------------------------------------------------------
    def _prepack(self):
        """Refresh the packed weight copies of the iteration AHEAD of their use, on the side stream: the forward is a serial chain on the
        main stream with the side stream idle, and every layer's pack launch (2 - 10 us, ~65 per iteration) sat in that chain in front of
        its convolution.  Three events: the first neck stage's forward layouts (the main stream meets them after the PFN), the other forward
        layouts, the data-gradient layouts.  A layout is refreshed here once a call has taken it (the first iteration packs lazily as
        before); ``ps.fresh`` is the iteration's token, the wrappers' own repack calls see it and do nothing."""
        ps = self.ps
        if not R.train_prepack or ps.side.stream is None:
            ps.fresh = self._pack_events = None
            return
        tok = ps.fresh = object()
        # group 0 = every layout the main stream takes before it waits for event 1
        first = {id(c) for c in self.neck_train.early_convs()}
        groups = ([c for c in ps.convs if id(c) in first], [c for c in ps.convs if id(c) not in first])

        def packs():
            for k, group in enumerate(groups):
                for c in group:
                    c.prepack_fwd(tok)
                self._pack_ev[k].record()
            for c in ps.convs:
                c.prepack_bwd(tok)
            self._pack_ev[2].record()

        ps.side.run(packs, after=self._iter_start)
        self._pack_events = self._pack_ev

    def _packs_ready(self, k: int) -> None:
        if self._pack_events is not None:
            torch.cuda.current_stream().wait_event(self._pack_events[k])

    def forward_backward(self, points, sample_offsets, batch, targets: ops.CenterLossTargets, grid_ind=None, grad_scale=1.0, voxel_labels=None,
                         seg_loss_scale=1.0, point_labels=None, prev_sweep=None):
        """forward + loss + backward; gradients land in ``self.ps.flat_g`` (overwritten, not accumulated).

        ``voxel_labels`` (B,1,H,W) integer on the device, 0 = unlabelled (the dataset's majority vote, preprocess.py:172-191): the seg
        super-task trains jointly -- the total loss is det_loss + seg_head.weight * seg_loss_scale * SegLoss; the returned vector is the
        det loss as before and ``self.seg_loss`` the device vector [loss, lovasz, ce, n_valid, n_present] of the unweighted SegLoss.
        ``seg_loss_scale``: the trainer's seg_loss_decay as a non-negative host float.
        ``point_labels`` (one device uint8 / int32 / int64 label per row of ``points``; < 0: unlabelled) instead of ``voxel_labels``: the
        step builds the targets itself from its voxel index (``ops.voxel_labels_from_points``: the dataset's majority vote on the device) and
        trains exactly as with the ``voxel_labels`` that vote gives.  Both: ValueError.  Neither (or a model without a seg head): the
        det-only step; a seg head's gradients are then zero.
        ``prev_sweep``: dict(points, grid_ind, transform_matrix) of the previous sweep, for a neck that streams against it
        (train_stream.PolarStreamBDCPTrainStep)."""
        seg_scale = seg_loss_scale_value(seg_loss_scale)
        self._seg_labels = self._point_labels = self.seg_loss = None
        if voxel_labels is not None and point_labels is not None:
            raise ValueError("give voxel_labels or point_labels, not both")
        if point_labels is not None:
            if self.seg is None:
                raise ValueError("point_labels given, but the model has no seg head")
            hip.require_device(point_labels)
            if self.spec.grid[2] != 1:
                raise ValueError("point_labels: the seg head's map is 2-D, the grid must have one cell along z")
            assert point_labels.numel() == points.shape[0], "point_labels must hold one label per row of points"
            self._point_labels = point_labels
        elif voxel_labels is not None:
            if self.seg is None:
                raise ValueError("voxel_labels given, but the model has no seg head")
            from .seg_heads import get_labels
            hip.require_device(voxel_labels)
            assert voxel_labels.dim() == 4 and voxel_labels.shape[1] == 1, "voxel_labels must be (B, 1, H, W)"
            self._seg_labels = get_labels(voxel_labels.squeeze(1), (self.spec.grid[1], self.spec.grid[0]))
        elif self.seg is not None:
            self.seg.gw.zero_()
            self.seg.gb.zero_()
        self._iter_start.record()     # the previous iteration's optimizer step is queued before it: the packs wait for this, not for the PFN
        try:
            self._forward(points, sample_offsets, batch, grid_ind, prev_sweep)
            losses = self.head_train.losses(targets)
            seg_dlogits = None
            if self._seg_labels is not None:
                head = self.seg.head
                # labels exist only on cells that hold labelled points (preprocess.py:172-191), so the point count bounds the valid cells: the
                # sort's launches are sized by it, not by the map.  More labelled cells than points: the loss vector is NaN (pn_seg_loss_f32)
                self.seg_loss, seg_dlogits = head.loss_func.loss_and_grad(ops.as_nchw(self.seg_logits)[:, :head.num_classes], self._seg_labels,
                                                                          scale=float(head.weight) * seg_scale * grad_scale,
                                                                          max_valid=max(int(self.vi.n_cap), 1))
            self._packs_ready(2)
            self._backward(targets, losses, grad_scale, seg_dlogits)
            loss = losses[0] if len(losses) == 1 else torch.stack(losses)      # several tasks: one row per task (the trainer sums the det_loss terms)
        finally:
            self.ps.fresh = None
            self._pack_events = None
            self._seg_labels = self._point_labels = None
        return loss

    def invalidate_inference_plans(self):
        invalidate_inference_plans(self.model)

    def step(self, points, sample_offsets, batch, targets: ops.CenterLossTargets, grid_ind=None, voxel_labels=None, seg_loss_scale=1.0,
             point_labels=None, prev_sweep=None):
        # (this class's forward_backward by name: the streaming steps' take their sweeps in another form)
        return self._step(lambda scale: PolarPillarTrainStep.forward_backward(
            self, points, sample_offsets, batch, targets, grid_ind, grad_scale=scale, voxel_labels=voxel_labels, seg_loss_scale=seg_loss_scale,
            point_labels=point_labels, prev_sweep=prev_sweep))

    def _step(self, forward_backward):
        """one iteration around ``forward_backward(grad_scale) -> loss``: gradient exchange, buffer broadcast, optimizer step"""
        import torch.distributed as dist
        from .dist_utils import BufferSync, GradExchange
        live = dist.is_available() and dist.is_initialized()
        world = dist.get_world_size() if live else 1
        if world > 1 and self.ps.side.on and dist.get_backend() == "gloo":
            # gloo is the transport of the same-GPU dry runs (several ranks on ONE device, tests / bench.py --backend gloo): with the ranks'
            # extra streams the device's hardware queues are oversubscribed across processes and every collective waits for a time slice
            # (1585 against 42 ms per iteration, two ranks on one GPU) -- one stream per rank there
            self.ps.side.on = False
        force = self.exchange_at_world_1 and world == 1 and live     # the RCCL path of a one-GPU box; the result is the no-exchange step's, bit for bit
        exchange = (world > 1 or force) and self.exchange_enabled
        self._exchange = GradExchange(self.ps.flat_g, self.buckets, force=force) if exchange else None
        # DDP's broadcast_buffers=True (the reference's setting, dist_utils.BufferSync): rank 0's BatchNorm running statistics to every rank
        # at the start of the forward -- one broadcast of one flat tensor, queued in front of the iteration
        if exchange and self.broadcast_buffers:
            if self._bufsync is None:
                self._bufsync = BufferSync(self.model, self.dev)
            self._bufsync.sync(force=force)
        # the reference averages the gradients over ranks (dist_utils.py:17-28): fold 1/world into the loss gradient
        try:
            loss = forward_backward(1.0 / world)
            if self._exchange is not None:
                self._exchange.finish()   # the last bucket (reader + first blocks), then the stream waits for all of them
        finally:
            self._exchange = None
        self.optimizer_step()
        return loss

    def sync_initial_params(self):
        """rank 0's parameters (and BatchNorm running statistics) to every rank, once before the first step"""
        self.opt.sync_initial_params(force=bool(self.exchange_at_world_1))
