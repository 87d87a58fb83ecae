"""Training of the Cartesian sector streamer (STROBE) on the HIP kernels.

Reference: ``STROBE.forward`` with ``return_loss`` (det3d/models/detectors/strobe_uber.py:124-228) over ``RPNUber``
(det3d/models/necks/rpn_uber.py:27-69), under autograd.  Every sweep but the last runs under ``torch.no_grad()`` (strobe_uber.py:162-210), so
nothing flows back through the memory: `pn_cart_memory_build_f32` / `pn_cart_memory_read_f32` are used as they are, and the previous
sweeps' maps are constants of the last sweep's backward.  Those feature-only sweeps still run in TRAIN mode: each moves every BatchNorm's
running statistics once before the last sweep does.  Here, without autograd:

``UberNeckTrain``     the train-mode form of RPNUber, a neck part of the step with the interface of ``train.RpnTrain`` plus the memory modules:
                      in front of every block i >= 1 the block's input x and the previous sweeps' map of that level share one wide
                      (n, h, w, 2C) map (x in the first half; ``RPNUber.prev_slot`` lets the memory read write the second half in place), which
                      ``memory{i}`` = Conv3x3(2C -> 2C, bias), GroupNorm(C, 2C), ReLU, Conv1x1(2C -> C, bias), GroupNorm(C, C), ReLU reduces to
                      C channels.  Backward of a module: GroupNorm -> 1x1 data / weight / bias gradients -> GroupNorm -> 3x3 weight / bias
                      gradients, then the data gradient of the FIRST C input channels only (``ConvDgrad`` over ``w[:, :C]``): the previous
                      sweeps' half has no consumer.  The result is the gradient of block i - 1's output and joins that block's deblock
                      gradient.
``STROBETrainStep``   ``PolarPillarTrainStep`` with that neck: reader, head part, losses, seg super-task, optimizer, checkpoint and gradient
                      buckets are the plain step's.  The targets of the stacked sector samples come from ``ops.assign_heatmap_cart_sectors``.
"""
from __future__ import annotations

from typing import List

import torch

from . import hip, ops
from .necks import RPNUber
from .train import PolarPillarTrainStep, RpnTrain
from .train_layers import _ConvGNReLU


class _MemoryTrain:
    """one ``memory{i}`` module of RPNUber in training form (see the module text)"""

    def __init__(self, ps, i: int, mem):
        conv3, gn2, _, conv1, gn1, _ = mem._modules.values()
        if tuple(conv3.kernel_size) != (3, 3) or tuple(conv1.kernel_size) != (1, 1) or conv3.bias is None or conv1.bias is None:
            raise NotImplementedError("RPNUber memory module: Conv3x3(bias) + GroupNorm + ReLU + Conv1x1(bias) + GroupNorm + ReLU")
        p = f"neck.memory{i}."
        self.ps, self.c, self.wname = ps, int(conv1.out_channels), p + "0.weight"
        self.wide = _ConvGNReLU(ps, p + "0.weight", p + "0.bias", p + "1.weight", p + "1.bias", gn2.num_groups, 1, gn2.eps)
        self.reduce = _ConvGNReLU(ps, p + "3.weight", p + "3.bias", p + "4.weight", p + "4.bias", gn1.num_groups, 1, gn1.eps, pad=0)
        self.names = [p + k for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias")]
        self.dgrad_x = ops.ConvDgrad(ps.p[self.wname][:, :self.c], 1, 1)      # the block input's half of the 3x3 convolution

    def fwd(self, x, prev):
        n, h, w, c = x.shape
        hip.require_device(prev)
        assert c == self.c and tuple(prev.shape) == tuple(x.shape), f"memory module: prev {tuple(prev.shape)} does not match the block input {tuple(x.shape)}"
        both = RPNUber._wide_of(prev)
        if both is None:
            both = RPNUber._wide_of(RPNUber.prev_slot(x.shape, x.device))
            ops.assemble_rows([[(prev.contiguous(), k, 0, h)] for k in range(n)], w, c, out=both, out_channel_offset=c)
        ops.assemble_rows([[(x, k, 0, h)] for k in range(n)], w, c, out=both)
        return self.reduce.fwd(self.wide.fwd(both))

    def drop(self):
        for layer in (self.wide, self.reduce):
            layer.y = layer.stat = layer.conv.x = None

    def bwd(self, dout):
        """dout: gradient of the module's output (own tensor, overwritten) -> gradient of the block input x (n, h, w, C)"""
        (d_mid,) = self.reduce.bwd(dout)
        self.wide.bwd(d_mid, need_dx=False)          # d_mid now holds the 3x3 convolution's output gradient
        self.dgrad_x.repack(self.ps.p[self.wname][:, :self.c])
        return self.dgrad_x(d_mid)

    def zero_grads(self):
        for name in self.names:
            self.ps.g[name].zero_()


class UberNeckTrain(RpnTrain):
    """RPNUber in training form over a ``ParamStore`` (see the module text).
      ``forward_prev(canvas, prev_sweep)``  a feature-only sweep: train-mode statistics, nothing saved, ALL blocks and deblocks (so that the last
                                            block's and the deblocks' running statistics take the update, as ``ContextNeckTrain.forward_prev``
                                            does for polarstream.py) -> ``cur_sweep`` for ``STROBE.update_memory``
      ``forward(canvas, prev_sweep)``       the last sweep -> the concatenated deblock outputs; ``cur_sweep`` is kept on the object
      ``backward(d_x2, block_done)``        -> the gradient of the canvas
    ``prev_sweep``: None (no memory modules run; their gradients are then zero) or one map per block i >= 1.  The stacked sector canvases
    take the dense first layer: the pillar-rows form is not used."""

    def __init__(self, ps, neck, wait_packs=lambda k: None):
        if not isinstance(neck, RPNUber):
            raise NotImplementedError("UberNeckTrain: the neck must be an RPNUber")
        with ops.R.override(train_pillar_conv=False):
            super().__init__(ps, neck, wait_packs)
        self.memory = {i: _MemoryTrain(ps, i, getattr(neck, "memory" + str(i))) for i in range(1, len(neck.blocks))}
        self.cur_sweep: List[torch.Tensor] = []
        self._with_memory = False

    def _run(self, canvas, prev_sweep, save: bool):
        if prev_sweep is not None and len(prev_sweep) != len(self.blocks) - 1:
            raise ValueError(f"prev_sweep must hold one map per block i >= 1 ({len(self.blocks) - 1}), got {len(prev_sweep)}")
        x, out, off, cur = canvas, None, 0, []
        self.block_out = []
        for i, layers in enumerate(self.blocks):
            if i < 2:
                self.wait_packs(i)
            if i > 0:
                if prev_sweep is not None:
                    x = self.memory[i].fwd(x, prev_sweep[i - 1])
                cur.append(x)
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
        self.wait_packs(1)
        if not save:
            for layer in [l for layers in self.blocks for l in layers] + self.deblocks:
                layer.take_saved()
            for m in self.memory.values():
                m.drop()
        return out, cur

    def forward_prev(self, canvas, prev_sweep=None):
        return self._run(canvas, prev_sweep, save=False)[1]

    def forward(self, canvas, prev_sweep=None):
        self._with_memory = prev_sweep is not None
        out, self.cur_sweep = self._run(canvas, prev_sweep, save=True)
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
            if i > 0:      # memory{i}: queued behind block i and before block_done(i - 1)
                if self._with_memory:
                    d_block = self.memory[i].bwd(d_block)
                else:
                    self.memory[i].zero_grads()
        return d_block


class STROBETrainStep(PolarPillarTrainStep):
    """One training iteration of STROBE(DynamicPFNet, DynamicPPScatter, RPNUber, <a head of PolarPillarTrainStep>[, SingleConvHead]).

    ``step(sweeps, targets, voxel_labels=None, point_labels=None, seg_loss_scale=1.0)`` / ``forward_backward(...)``: ``sweeps`` = the list of
    collated examples ``STROBE.forward`` takes, oldest first, each with ``points``, ``grid_ind`` (both on the device), ``num_points``,
    ``grid_size`` and ``transform_matrix``, every sweep's sectors stacked sector-major on the sector grid; ``targets`` = the last sweep's
    ``CenterLossTargets`` of the stacked samples (``ops.assign_heatmap_cart_sectors``); ``voxel_labels`` (nsectors * bs, 1, h, w) /
    ``point_labels`` as in the plain step, over the last sweep's stacked samples.  Every sweep but the last: reader + scatter with nothing
    kept, the neck's feature-only pass (train-mode statistics), ``model.update_memory``.  The last sweep: forward, losses (det + seg
    jointly), backward, one ``FlatAdam`` update.  Nothing flows back through the memory (strobe_uber.py:162-210).

    A list of fewer than two sweeps raises ValueError: with no previous sweep the memory modules would get no gradient, and what the
    reference's optimizer wrapper does with such parameters is not built here."""

    def __init__(self, model, total_steps: int, **kw):
        from .detectors import STROBE
        if not isinstance(model, STROBE) or not isinstance(model.neck, RPNUber):
            raise NotImplementedError("STROBETrainStep: the model must be a STROBE with an RPNUber neck")
        if model._get("pc_range") is None:
            raise ValueError("STROBETrainStep: the model's test_cfg must hold pc_range (the memory of the feature-only sweeps is built with it)")
        self.nsec = int(model.nsectors)
        super().__init__(model, total_steps, neck_part=UberNeckTrain, **kw)
        self.spec = ops.GridSpec(self.spec.lo, self.spec.vs, tuple(ops.cart_sector_grid(self.spec.grid, self.nsec)))      # STROBE._canvas

    def _check_sweeps(self, sweeps) -> int:
        if isinstance(sweeps, dict) or len(sweeps) < 2:
            raise ValueError("STROBETrainStep takes a list of at least two sweeps, oldest first: with no previous sweep the memory modules "
                             "get no gradient")
        batch = len(sweeps[-1]["num_points"])
        g = tuple(int(v) for v in sweeps[-1]["grid_size"][0])
        if g != tuple(self.spec.grid):
            raise ValueError(f"the sweeps' grid {g} is not the sector grid {tuple(self.spec.grid)} of {self.nsec} sectors")
        for ex in sweeps:
            hip.require_device(ex["points"], ex["grid_ind"])
            if len(ex["num_points"]) != batch or batch % self.nsec:
                raise ValueError(f"every sweep must stack nsectors * bs samples ({self.nsec} sectors)")
        return batch

    def _forward(self, points, sample_offsets, batch, grid_ind, prev_sweep):
        """``prev_sweep``: the list of the earlier sweeps' examples"""
        neck, bs, memory = self.neck_train, batch // self.nsec, None
        for k, ex in enumerate(prev_sweep):
            pv = self._index(ex["points"], None, batch, ex["grid_ind"])
            canvas = self._canvas(ex["points"], pv, batch)
            if k == 0:
                self._prepack()     # issued behind the first scatter stage's launches, runs beside them
            memory = self.model.update_memory(neck.forward_prev(canvas, memory), ex["transform_matrix"], bs)
        spec = self.spec
        self.vi = self._index(points, None, batch, grid_ind)
        if self._point_labels is not None:
            self._seg_labels = ops.voxel_labels_from_points(self._point_labels, self.vi, dense=False, loss_labels=True).view(
                batch, spec.grid[1], spec.grid[0])
        self.points = points
        canvas = self._canvas(points, self.vi, batch)
        x2 = neck.forward(canvas, memory)
        self.seg_logits = None
        if self._seg_labels is not None:
            self.seg_logits = self.seg.forward(canvas, x2)
        return self.head_train.forward(x2)

    def forward_backward(self, sweeps, targets, grad_scale=1.0, voxel_labels=None, point_labels=None, seg_loss_scale=1.0):
        """-> the det loss vector; gradients in ``ps.flat_g``; ``self.seg_loss`` as in the plain step"""
        batch = self._check_sweeps(sweeps)
        cur = sweeps[-1]
        return super().forward_backward(cur["points"], None, batch, targets, cur["grid_ind"], grad_scale, voxel_labels, seg_loss_scale, point_labels,
                                        prev_sweep=list(sweeps[:-1]))

    def step(self, sweeps, targets, voxel_labels=None, point_labels=None, seg_loss_scale=1.0):
        return self._step(lambda scale: self.forward_backward(sweeps, targets, grad_scale=scale, voxel_labels=voxel_labels, point_labels=point_labels,
                                                              seg_loss_scale=seg_loss_scale))
