"""Training of the bidirectional sector-streaming detector (PolarStreamBDCP) on the HIP kernels.

Reference: the two-sweep loss path  det3d/models/detectors/polarstream.py:267-416  (previous sweep under ``torch.no_grad()`` in
``feature_only`` mode :318-381, current sweep streamed sector by sector in ``train`` mode :386-402) over the context-padded neck
det3d/models/necks/rpn_context.py:96-215, under autograd.  Here, without autograd:

``ContextNeckTrain``   the train-mode form of RPNBDCP.  Per layer and neck call: the padded map P is assembled from whole-row pieces
                       (the pieces of the inference neck, ``RPNBDCP._pad_feature_only`` / ``_pad_streaming``), convolved with padding
                       (0, 1), and normalised with THAT CALL's batch statistics (BatchNorm statistics are taken once per neck call: one
                       stacked feature-only pass plus one call per sector, each updating the running statistics in that order).  Saved per
                       (layer, sector): P, the convolution's output, the statistics.  Backward runs the sectors in reverse and, inside a
                       sector, the layers in reverse; parameter gradients accumulate across the sector calls.  The gradient of P's centre
                       rows is the plain pad-1 data gradient (``ops.ConvDgrad``, its F(4,3) / F(2,3) forms included); the gradient of the
                       TOP row -- the trailing row of the sector before -- comes from `pn_conv_border_dgrad_f32` and is what carries
                       gradient between sectors.  It is launched once the gradient of the earlier sector's layer input exists, ACCUMULATING
                       into that map's last row before the layer below consumes it (no pending copy, no separate add); with one sector the
                       padding is circular and both border rows accumulate into rows h - 1 and 0 of the same map.  Rows taken from the
                       previous sweep or from zeros get no gradient.
``PolarStreamBDCPTrainStep``  ``PolarPillarTrainStep`` built with that neck as its neck part (``neck_train``, also ``ctx_neck``): reader, head
                       part, losses, seg super-task, optimizer, checkpoint and gradient buckets are the plain step's, and so are the bodies
                       of ``forward_backward`` and ``step`` -- the previous sweep is their ``prev_sweep`` argument.  It runs reader + neck in
                       feature-only form with nothing saved; the rows the streaming pass reads are warped by `pn_polar_warp_strips_f32`.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import hip, ops
from .necks_context import RPNBDCP
from .train import PolarPillarTrainStep
from .train_layers import _ConvBNReLU
from .utils.synth import synthetic_iteration      # noqa: F401  (its callers import it from here)

RELU = ops.ACT_RELU


def context_layer_names(neck) -> List[Dict[str, str]]:
    """the parameter names (relative to the model: ``neck. ...``) of every context-padded layer, in forward order: block i, layer j ->
    conv ``neck.blocks.i.j.block.0.weight``, norm ``neck.blocks.i.j.block.1.weight`` / ``.bias``"""
    table = []
    for i, blk in enumerate(neck.blocks):
        for j in range(len(blk._modules)):
            p = f"neck.blocks.{i}.{j}.block."
            table.append(dict(block=i, layer=j, weight=p + "0.weight", gamma=p + "1.weight", beta=p + "1.bias"))
    return table


def deblock_names(neck) -> List[Dict[str, str]]:
    return [dict(weight=f"neck.deblocks.{j}.0.weight", gamma=f"neck.deblocks.{j}.1.weight", beta=f"neck.deblocks.{j}.1.bias")
            for j in range(len(neck.deblocks))]


class _CtxLayer:
    """one ConvBDCP (3x3 convolution on the context-padded map + BatchNorm + ReLU) in training form; the caller keeps what ``fwd`` saved"""

    def __init__(self, ps, names: Dict[str, str], cc):
        conv, bn = cc.block[0], cc.block[1]
        if tuple(conv.kernel_size) != (3, 3) or int(cc.padding) != 1 or conv.bias is not None or conv.stride[0] not in (1, 2):
            raise NotImplementedError("context-padded training layer: 3x3, padding 1, stride 1 or 2, no bias")
        self.ps, self.mod, self.bn = ps, cc, bn
        self.wname, self.gname, self.bname = names["weight"], names["gamma"], names["beta"]
        self.stride = int(conv.stride[0])
        w = ps.p[self.wname]
        self.layer = ops.ConvLayer(w, stride=self.stride, pad=(0, 1))
        self.dgrad = ops.ConvDgrad(w, self.stride, 1)
        self.pieces = dict(padding=1, mod=cc, ctx=lambda padded: padded)     # what RPNBDCP._pad_* take as a plan layer: they return P itself

    def fwd(self, padded, token, save=True):
        ps, bn = self.ps, self.bn
        self.layer.repack(ps.p[self.wname], None, token=token)
        y = self.layer(padded)
        out, stat = ops.batchnorm_train(y, ps.p[self.gname], ps.p[self.bname], bn.eps, bn.momentum, bn.running_mean, bn.running_var, act=RELU)
        return out, ((padded, y, stat) if save else None)

    def bwd(self, saved, dout, token, wacc, dx=None):
        """dout: gradient of the layer's output (own tensor; overwritten with the convolution's output gradient, which is returned next to the
        gradient of P's centre rows)"""
        ps = self.ps
        padded, y, stat = saved
        ops.batchnorm_bwd(y, dout, ps.p[self.gname], ps.p[self.bname], stat, act=RELU, dx=dout, dgamma=ps.g[self.gname], dbeta=ps.g[self.bname],
                          accumulate=wacc)
        dy = dout
        ps.side.run(lambda: ops.conv_wgrad(padded, dy, 3, 3, self.stride, (0, 1), out=ps.g[self.wname], accumulate=wacc), dy, padded)
        self.dgrad.repack(ps.p[self.wname], token=token)
        return self.dgrad(dy, out=dx), dy


class ContextNeckTrain:
    """RPNBDCP in training form over a ``ParamStore`` (see the module text): a neck part of the step, with the interface of ``train.RpnTrain``.
    ``forward_prev`` = the previous sweep's feature-only pass, ``forward`` = the current sweep (all sectors), ``backward`` = its gradients."""

    sparse_first = None     # the sector canvases are dense

    def __init__(self, ps, neck: RPNBDCP, wait_packs=lambda k: None):
        if not isinstance(neck, RPNBDCP):
            raise NotImplementedError("ContextNeckTrain: the neck must be an RPNBDCP")
        self.ps, self.neck, self.wait_packs = ps, neck, wait_packs
        mods = [cc for blk in neck.blocks for cc in blk._modules.values()]
        self.layers = [_CtxLayer(ps, names, cc) for names, cc in zip(context_layer_names(neck), mods)]
        self.block_of = [names["block"] for names in context_layer_names(neck)]
        self.deblocks = [_ConvBNReLU(ps, f"neck.deblocks.{j}.", 0, de[1], de[0]) for j, de in enumerate(neck.deblocks)]
        self.up_start = neck._upsample_start_idx
        self.up_filters = list(neck._num_upsample_filters)
        self.token = self._prev_token = None
        self.saved = self.de_saved = None

    def early_convs(self):
        """the deblock fed by block 0: the deblocks' layouts are refreshed on the side stream, the context layers pack on first use"""
        return [self.deblocks[0].conv] if self.up_start == 0 and self.deblocks else []

    # ---------------------------------------------------------------------------------------------------------------- forward
    def forward_prev(self, canvas, nsectors: int):
        """the stacked sectors of the PREVIOUS sweep in feature-only form, train-mode statistics (they update the running statistics before
        the current sweep's calls do), nothing saved -> the layers' inputs.  The streaming pass reads nothing past the last layer's input,
        but the reference's pass runs the whole neck in train mode (polarstream.py:318-336), so the last layer's and the deblocks' running
        statistics take this call's update too: they are run for their statistics and their outputs dropped."""
        self.token = self._prev_token = object()
        x, cur = canvas, []
        for k, layer in enumerate(self.layers):
            cur.append(x)
            x, _ = layer.fwd(self.neck._pad_feature_only(layer.pieces, x, nsectors), self.token, save=False)
            if k + 1 == len(self.layers) or self.block_of[k + 1] != self.block_of[k]:
                j = self.block_of[k] - self.up_start
                if j >= 0:
                    self.deblocks[j].fwd(x)
                    self.deblocks[j].take_saved()
        return cur

    def forward(self, canvas, nsectors: int, prev_sweep=(), prev_canvas=None, warp=None):
        """canvas (nsectors * bs, hs, w, c) stacked sector-major -> the stacked concatenated deblock outputs.  The previous sweep: its
        warped rows per layer (``prev_sweep``), or its stacked canvas (``prev_canvas``) and ``warp(layer inputs) -> prev_sweep``: then its
        feature-only pass runs here first."""
        self.wait_packs(0)
        self.wait_packs(1)
        if prev_canvas is not None:
            inputs = self.forward_prev(prev_canvas, nsectors)
            if nsectors > 1:          # one sector pads circularly: the previous sweep's pass only moves the running statistics, as in the reference
                prev_sweep = warp(inputs)
        self.token, self._prev_token = (self._prev_token or object()), None      # one token per iteration: the packed weights are refreshed once
        n = canvas.shape[0]
        assert n % nsectors == 0
        bs = n // nsectors
        self.nsec, self.bs = nsectors, bs
        self.saved = [[None] * len(self.layers) for _ in range(nsectors)]
        self.de_saved = [[None] * len(self.deblocks) for _ in range(nsectors)]
        self.top_from_ctx = [[False] * len(self.layers) for _ in range(nsectors)]
        out, ctx = None, []
        for s in range(nsectors):
            x = canvas[s * bs:(s + 1) * bs]
            cur, prev, layer_id = [], list(ctx), 0
            for k, layer in enumerate(self.layers):
                cur.append(x)
                if nsectors > 1:
                    assert len(prev_sweep) > 0, "several sectors stream against the previous sweep's maps"
                    sweep = prev_sweep[layer_id]
                    layer_id = (layer_id + 1) % len(prev_sweep)
                    self.top_from_ctx[s][k] = s > 0
                else:
                    sweep = None
                padded, prev = self.neck._pad_streaming(layer.pieces, x, sweep, prev, s)
                x, self.saved[s][k] = layer.fwd(padded, self.token)
                if k + 1 == len(self.layers) or self.block_of[k + 1] != self.block_of[k]:
                    j = self.block_of[k] - self.up_start
                    if j >= 0:
                        de = self.deblocks[j]
                        if out is None:
                            oh, ow = de.conv.layer.out_hw(x.shape[1], x.shape[2])
                            out = torch.empty((n, oh, ow, sum(self.up_filters)), dtype=torch.float32, device=x.device)
                        de.fwd(x, out=out[s * bs:(s + 1) * bs], out_co=sum(self.up_filters[:j]))
                        self.de_saved[s][j] = de.take_saved()
            ctx = cur
        return out

    # ---------------------------------------------------------------------------------------------------------------- backward
    def backward(self, d_out, d_canvas: Optional[torch.Tensor] = None, block_done=None):
        """d_out: gradient of ``forward``'s result -> gradient of the stacked canvas.  Parameter gradients are OVERWRITTEN by the last sector's
        call (the first to run) and accumulated by the others.  ``block_done(i)`` is called once block i's parameter gradients (and its
        deblock's) are all queued, i.e. inside sector 0's backward."""
        nsec, bs, nl = self.nsec, self.bs, len(self.layers)
        first = self.saved[0][0][0]
        if d_canvas is None:
            d_canvas = torch.empty((nsec * bs, first.shape[1] - 2, first.shape[2], first.shape[3]), dtype=torch.float32, device=first.device)
        later = [None] * nl       # per layer: the convolution-output gradient of the sector after this one, whose top row is this sector's last row
        for s in range(nsec - 1, -1, -1):
            wacc = s < nsec - 1
            d = None
            for k in range(nl - 1, -1, -1):
                layer = self.layers[k]
                if k + 1 == nl or self.block_of[k + 1] != self.block_of[k]:        # the block's output: its deblock joins the gradient
                    j = self.block_of[k] - self.up_start
                    if j >= 0:
                        de = self.deblocks[j]
                        de.restore(self.de_saved[s][j])
                        off = sum(self.up_filters[:j])
                        if d is None:
                            d = de.bwd(d_out[s * bs:(s + 1) * bs], dout_co=off, wacc=wacc)
                        else:
                            de.bwd(d_out[s * bs:(s + 1) * bs], dout_co=off, dx=d, accumulate=True, wacc=wacc)
                padded = self.saved[s][k][0]
                h, w = padded.shape[1] - 2, padded.shape[2]
                d_in, dy = layer.bwd(self.saved[s][k], d, self.token, wacc, dx=d_canvas[s * bs:(s + 1) * bs] if k == 0 else None)
                wt = self.ps.p[layer.wname]
                if nsec == 1:       # circular: P's top row is this map's last row, its bottom row this map's first
                    ops.conv_border_dgrad(wt, dy, layer.stride, h, w, top=(d_in, h - 1, 0, True), bottom=(d_in, 0, 0, True))
                else:
                    if later[k] is not None:
                        ops.conv_border_dgrad(wt, later[k], layer.stride, h, w, top=(d_in, h - 1, 0, True))
                    later[k] = dy if self.top_from_ctx[s][k] else None
                d = d_in
                self.saved[s][k] = None
                if s == 0 and block_done is not None and (k == 0 or self.block_of[k - 1] != self.block_of[k]):
                    block_done(self.block_of[k])
        self.saved = self.de_saved = None
        self.token = None
        return d_canvas


class PolarStreamBDCPTrainStep(PolarPillarTrainStep):
    """One training iteration of PolarStreamBDCP(DynamicPFNet, DynamicPPScatter, RPNBDCP, <a head of PolarPillarTrainStep>[, SingleConvHead]).

    ``forward_backward(prev, cur, batch, targets, ...)`` / ``step(...)``: ``prev`` = dict(points, grid_ind, transform_matrix) of the
    previous sweep, ``cur`` = dict(points, grid_ind) of the current one, both stacked sector-major (index = sector * bs + b, as
    collate_kitti stacks them, collate.py:88-98); ``batch`` = nsectors * bs.  ``grid_ind`` (n, 4) [stacked sample, z, azimuth, range] is
    relative to the sector's canvas.  ``voxel_labels`` (batch, 1, hs, w) / ``point_labels`` as in the plain step, over the stacked samples.
    The previous sweep carries no gradient.  The sparse first-layer route does not apply: the sector canvases are dense, zero-filled."""

    def __init__(self, model, total_steps: int, **kw):
        from .detectors import PolarStreamBDCP
        if not isinstance(model, PolarStreamBDCP) or not isinstance(model.neck, RPNBDCP):
            raise NotImplementedError("PolarStreamBDCPTrainStep: the model must be a PolarStreamBDCP with an RPNBDCP neck")
        self.nsec = int(model.nsectors)
        super().__init__(model, total_steps, neck_part=ContextNeckTrain, **kw)
        self.ctx_neck = self.neck_train
        g = self.spec.grid
        if g[1] % self.nsec:
            raise ValueError(f"the azimuth axis ({g[1]} cells) does not divide into {self.nsec} sectors")
        self.spec = ops.GridSpec(self.spec.lo, self.spec.vs, (g[0], g[1] // self.nsec, g[2]))      # one sector's canvas (detectors._canvas)

    def _check_sweeps(self, prev, cur):
        hip.require_device(cur["points"], cur["grid_ind"])
        if self.nsec > 1:
            if prev is None:
                raise ValueError("several sectors stream against the previous sweep: prev = dict(points, grid_ind, transform_matrix)")
            hip.require_device(prev["points"], prev["grid_ind"])

    def forward_backward(self, prev, cur, batch, targets, grad_scale=1.0, voxel_labels=None, seg_loss_scale=1.0, point_labels=None):
        """-> the det loss vector; gradients in ``ps.flat_g``; ``self.seg_loss`` as in the plain step"""
        self._check_sweeps(prev, cur)
        return super().forward_backward(cur["points"], None, batch, targets, cur["grid_ind"], grad_scale, voxel_labels, seg_loss_scale, point_labels,
                                        prev_sweep=prev)

    def step(self, prev, cur, batch, targets, voxel_labels=None, seg_loss_scale=1.0, point_labels=None):
        self._check_sweeps(prev, cur)
        return super().step(cur["points"], None, batch, targets, cur["grid_ind"], voxel_labels, seg_loss_scale, point_labels, prev_sweep=prev)
