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

The trailing-edge detector (PolarStream + RPNTECP, polarstream.py:83-107 over rpn_context.py:46-95) trains through
``TrailingEdgeNeckTrain`` (the plain step's layers plus the border terms of csrc/conv_border.hip: nothing is assembled) and
``PolarStreamTrainStep`` (a list of sector examples, one neck call per sector, losses averaged over the sectors); see the classes.
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


class _BorderLayer(_ConvBNReLU):
    """one ConvContext of the trailing-edge neck in training form: the plain step's conv + BatchNorm + ReLU layer (every form ``_Conv``
    selects) plus the border terms of the context row.  ``top``: the input of the same layer in the sector before, whose last row is P's
    top row -- read in place."""

    def __init__(self, ps, names: Dict[str, str], cc):
        conv, bn = cc.block[0], cc.block[1]
        if tuple(conv.kernel_size) != (3, 3) or int(cc.padding) != 1 or conv.bias is not None or conv.stride[0] not in (1, 2):
            raise NotImplementedError("context-padded training layer: 3x3, padding 1, stride 1 or 2, no bias")
        assert names["weight"].endswith("block.0.weight")
        super().__init__(ps, names["weight"][:-len("0.weight")], 0, bn, conv)
        self.wname, self.stride = names["weight"], int(conv.stride[0])

    def fwd(self, x, top=None):
        ps = self.ps
        self.y = self.conv.fwd(x)
        if top is not None:
            ops.conv_border_fwd(ps.p[self.wname], self.y, self.stride, x.shape[1], x.shape[2], top=(top, top.shape[1] - 1, 0))
        res, self.stat = ops.batchnorm_train(self.y, ps.p[self.gname], ps.p[self.bname], self.bn.eps, self.bn.momentum, self.bn.running_mean,
                                             self.bn.running_var, act=RELU)
        return res

    def bwd(self, dout, top=None, wacc=False, dx=None):
        """dout: gradient of the layer's output (own tensor; overwritten with the convolution's output gradient) -> (gradient of the layer's
        input, the convolution's output gradient)"""
        ps, x = self.ps, self.conv.x
        ops.batchnorm_bwd(self.y, dout, ps.p[self.gname], ps.p[self.bname], self.stat, act=RELU, dx=dout, dgamma=ps.g[self.gname],
                          dbeta=ps.g[self.bname], accumulate=wacc)
        dy = dout
        d_in = self.conv.bwd(dy, dx=dx, wacc=wacc)
        if top is not None:      # behind the layer's weight gradient on the stream that runs it: both add into the same tensor
            ps.side.run(lambda: ops.conv_border_wgrad(dy, ps.g[self.wname], self.stride, x.shape[1], x.shape[2], top=(top, top.shape[1] - 1, 0)),
                        dy, top)
        return d_in, dy


class TrailingEdgeNeckTrain:
    """RPNTECP (rpn_context.py:46-95) in training form over a ``ParamStore``: a neck part of the step, with the interface of
    ``train.RpnTrain``.  A trailing-edge layer is the plain pad-1 layer plus one row: P = [ctx; x; 0] with ctx the last row of the same
    layer's input in the sector before, so  conv(P) = conv_pad1(x) + T(ctx)  where T touches output row 0 only.  The layers are
    the plain step's; per sector s > 0 and layer, `pn_conv_border_fwd_f32` adds T between the convolution and the BatchNorm,
    `pn_conv_border_wgrad_f32` adds its weight gradient behind the layer's, and `pn_conv_border_dgrad_f32` carries the gradient of ctx into
    the last row of the earlier sector's input gradient before the layer below consumes it -- nothing is assembled or copied.  BatchNorm
    statistics are taken per neck call (one per sector, in sector order).
      ``begin(nsectors)`` / ``forward_sector(canvas)``   one neck call per sector, in streaming order
      ``forward(canvas, nsectors)``                      all sectors of a canvas stacked sector-major
      ``backward(d_out, d_canvas, block_done)``          sectors in reverse; ``d_out`` stacked or one tensor per sector"""

    sparse_first = None     # the sector canvases are dense

    def __init__(self, ps, neck, wait_packs=lambda k: None):
        from .necks_context import RPNTECP
        if type(neck) is not RPNTECP:
            raise NotImplementedError("TrailingEdgeNeckTrain: the neck must be an RPNTECP")
        self.ps, self.neck, self.wait_packs = ps, neck, wait_packs
        names = context_layer_names(neck)
        mods = [cc for blk in neck.blocks for cc in blk._modules.values()]
        self.layers = [_BorderLayer(ps, nm, cc) for nm, cc in zip(names, mods)]
        self.block_of = [nm["block"] for nm in names]
        self.deblocks = [_ConvBNReLU(ps, f"neck.deblocks.{j}.", 0, de[1], de[0]) for j, de in enumerate(neck.deblocks)]
        self.up_start = neck._upsample_start_idx
        self.up_filters = list(neck._num_upsample_filters)
        self.block_out: List[torch.Tensor] = []      # the blocks' outputs of the last neck call
        self.saved = self.de_saved = None
        self.nsec = self.bs = 0

    def early_convs(self):
        """block 0 and the deblock fed by block 0"""
        first = [layer.conv for layer, i in zip(self.layers, self.block_of) if i == 0]
        return first + ([self.deblocks[0].conv] if self.up_start == 0 and self.deblocks else [])

    def _block_end(self, k: int) -> bool:
        return k + 1 == len(self.layers) or self.block_of[k + 1] != self.block_of[k]

    # ---------------------------------------------------------------------------------------------------------------- forward
    def begin(self, nsectors: int):
        self.nsec, self.bs = int(nsectors), 0
        self.saved, self.de_saved = [], []

    def forward_sector(self, canvas, out=None):
        """the next sector's canvas (bs, hs, w, c) -> the concatenated deblock outputs of that sector (written to ``out`` when given)"""
        s = len(self.saved)
        assert s < self.nsec, "begin(nsectors) first; one call per sector"
        self.bs = canvas.shape[0]
        saved, de_saved, x = [], [None] * len(self.deblocks), canvas
        self.block_out = []
        for k, layer in enumerate(self.layers):
            if k == 0 or self.block_of[k] != self.block_of[k - 1]:
                if self.block_of[k] < 2:
                    self.wait_packs(self.block_of[k])
            x = layer.fwd(x, top=self.saved[s - 1][k][0] if s > 0 else None)
            saved.append(layer.take_saved())
            if self._block_end(k):
                self.block_out.append(x)
                j = self.block_of[k] - self.up_start
                if j >= 0:
                    de = self.deblocks[j]
                    if out is None:
                        oh, ow = de.conv.layer.out_hw(x.shape[1], x.shape[2])
                        out = torch.empty((canvas.shape[0], oh, ow, sum(self.up_filters)), dtype=torch.float32, device=canvas.device)
                    de.fwd(x, out=out, out_co=sum(self.up_filters[:j]))
                    de_saved[j] = de.take_saved()
        self.wait_packs(1)
        self.saved.append(saved)
        self.de_saved.append(de_saved)
        return out

    def forward(self, canvas, nsectors: int = 1):
        n = canvas.shape[0]
        assert n % nsectors == 0
        bs = n // nsectors
        self.begin(nsectors)
        out = None
        for s in range(nsectors):
            if out is None:
                first = self.forward_sector(canvas[s * bs:(s + 1) * bs])
                if nsectors == 1:
                    return first
                out = torch.empty((n,) + tuple(first.shape[1:]), dtype=torch.float32, device=canvas.device)
                out[:bs].copy_(first)
            else:
                self.forward_sector(canvas[s * bs:(s + 1) * bs], out=out[s * bs:(s + 1) * bs])
        return out

    # ---------------------------------------------------------------------------------------------------------------- backward
    def backward(self, d_out, d_canvas: Optional[torch.Tensor] = None, block_done=None):
        """d_out: gradient of the sectors' outputs (stacked sector-major, or a list of one tensor per sector) -> gradient of the stacked
        canvas.  Parameter gradients are OVERWRITTEN by the last sector's call (the first to run) and accumulated by the others;
        ``block_done(i)`` is called inside sector 0's backward."""
        nsec, bs, nl = self.nsec, self.bs, len(self.layers)
        assert len(self.saved) == nsec, "one forward_sector call per sector before backward"
        first = self.saved[0][0][0]
        if d_canvas is None:
            d_canvas = torch.empty((nsec * bs,) + tuple(first.shape[1:]), dtype=torch.float32, device=first.device)
        later = [None] * nl       # per layer: the convolution-output gradient of the sector after this one, whose top row is this sector's last row
        for s in range(nsec - 1, -1, -1):
            wacc = s < nsec - 1
            d_s = d_out[s] if isinstance(d_out, (list, tuple)) else d_out[s * bs:(s + 1) * bs]
            d = None
            for k in range(nl - 1, -1, -1):
                layer = self.layers[k]
                if self._block_end(k):        # the block's output: its deblock joins the gradient
                    j = self.block_of[k] - self.up_start
                    if j >= 0:
                        de = self.deblocks[j]
                        de.restore(self.de_saved[s][j])
                        off = sum(self.up_filters[:j])
                        if d is None:
                            d = de.bwd(d_s, dout_co=off, wacc=wacc)
                        else:
                            de.bwd(d_s, dout_co=off, dx=d, accumulate=True, wacc=wacc)
                layer.restore(self.saved[s][k])
                x = self.saved[s][k][0]
                top = self.saved[s - 1][k][0] if s > 0 else None
                d_in, dy = layer.bwd(d, top=top, wacc=wacc, dx=d_canvas[s * bs:(s + 1) * bs] if k == 0 else None)
                if later[k] is not None:
                    ops.conv_border_dgrad(self.ps.p[layer.wname], later[k], layer.stride, x.shape[1], x.shape[2], top=(d_in, x.shape[1] - 1, 0, True))
                later[k] = dy if s > 0 else None
                d = d_in
                layer.take_saved()
                if s == 0 and block_done is not None and (k == 0 or self.block_of[k - 1] != self.block_of[k]):
                    block_done(self.block_of[k])
            self.saved[s] = self.de_saved[s] = None      # (what the side stream still reads is kept by ``ps.side`` until its join)
        self.saved = self.de_saved = None
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


class PolarStreamTrainStep(PolarPillarTrainStep):
    """One training iteration of the trailing-edge PolarStream(DynamicPFNet, DynamicPPScatter, RPNTECP, <a head of PolarPillarTrainStep>
    [, SingleConvHead]) on a sweep given as a LIST of sector examples (polarstream.py:83-107 with ``return_loss``: the sectors run one after
    another, every sector's ``next_context`` -- not detached -- pads the next one, and ``merge_list``, single_stage.py:10-22, averages every
    loss term over the sectors).

    ``forward_backward(sectors, batch, targets, ...)`` / ``step(...)``: ``sectors`` = one dict(points, grid_ind) per sector in streaming
    order, each stacked over ``batch`` samples with ``grid_ind`` (n, 4) [sample, z, azimuth, range] relative to the sector's canvas
    (collate.py:100-107); ``targets`` = one ``CenterLossTargets`` per sector; ``voxel_labels`` / ``point_labels`` = lists of per-sector
    tensors, or None.  Per sector, in order: index, reader + scatter, neck call, seg head, bbox head, losses -- every module's running
    statistics move in the reference's order -- and right away the backward of the two heads, which do not couple sectors: what stays for
    the reverse pass is the sector's ``d_x2`` and the seg head's canvas half.  Every sector's loss gradient carries ``grad_scale / nsec``.
    The parameter gradients of reader, heads and seg head are summed over the sectors in ``ps.flat_g`` (`pn_add_f32` over the heads' flat
    range, the reader kernel's accumulate flag); the neck's through ``TrailingEdgeNeckTrain``.  Returns the per-sector det loss vectors
    stacked (nsec, ...); ``self.seg_loss`` is (nsec, 5); the merged values a trainer logs are their means."""

    def __init__(self, model, total_steps: int, **kw):
        from .detectors import PolarStream, PolarStreamBDCP
        from .necks_context import RPNTECP
        if not isinstance(model, PolarStream) or isinstance(model, PolarStreamBDCP) or type(model.neck) is not RPNTECP:
            raise NotImplementedError("PolarStreamTrainStep: the model must be a PolarStream with an RPNTECP neck")
        super().__init__(model, total_steps, neck_part=TrailingEdgeNeckTrain, **kw)
        self.sweep_spec = self.spec
        ps = self.ps
        # the heads' parameters are the tail of the flat buffer (seg head, then bbox head): one range to sum over the sectors
        self._heads_lo = min((ps.offsets[n][0] for n in ps.names if n.split(".")[0] in ("seg_head", "bbox_head")), default=ps.total)
        self._heads_sum = torch.empty(ps.total - self._heads_lo, dtype=torch.float32, device=self.dev)

    def _check(self, sectors, targets, voxel_labels, point_labels):
        if not isinstance(sectors, (list, tuple)) or len(sectors) < 1:
            raise ValueError("sectors: a list of dict(points, grid_ind), one per sector")
        nsec = len(sectors)
        if not isinstance(targets, (list, tuple)) or len(targets) != nsec:
            raise ValueError(f"{nsec} sectors, but targets is not a list of {nsec} CenterLossTargets")
        for name, labels in (("voxel_labels", voxel_labels), ("point_labels", point_labels)):
            if labels is not None and (not isinstance(labels, (list, tuple)) or len(labels) != nsec):
                raise ValueError(f"{nsec} sectors, but {name} is not a list of {nsec} tensors")
        if voxel_labels is not None and point_labels is not None:
            raise ValueError("give voxel_labels or point_labels, not both")
        if (voxel_labels is not None or point_labels is not None) and self.seg is None:
            raise ValueError("labels given, but the model has no seg head")
        g = self.sweep_spec.grid
        if g[1] % nsec:
            raise ValueError(f"the azimuth axis ({g[1]} cells) does not divide into {nsec} sectors")
        for sec in sectors:
            hip.require_device(sec["points"], sec["grid_ind"])
        for labels in (voxel_labels, point_labels):
            if labels is not None:
                hip.require_device(*labels)
        return nsec

    def forward_backward(self, sectors, batch, targets, grad_scale=1.0, voxel_labels=None, seg_loss_scale=1.0, point_labels=None):
        """-> the det loss vectors (nsec, ...); gradients in ``ps.flat_g`` (overwritten); ``self.seg_loss`` (nsec, 5) or None"""
        from .train import seg_loss_scale_value
        nsec = self._check(sectors, targets, voxel_labels, point_labels)
        seg_scale = seg_loss_scale_value(seg_loss_scale)
        ps, neck, head_train, seg = self.ps, self.neck_train, self.head_train, self.seg
        g = self.sweep_spec.grid
        self.nsec = nsec
        self.spec = spec = ops.GridSpec(self.sweep_spec.lo, self.sweep_spec.vs, (g[0], g[1] // nsec, g[2]))      # one sector's canvas
        with_seg = voxel_labels is not None or point_labels is not None
        if point_labels is not None and spec.grid[2] != 1:
            raise ValueError("point_labels: the seg head's map is 2-D, the grid must have one cell along z")
        self.seg_loss = None
        if seg is not None and not with_seg:
            seg.gw.zero_()
            seg.gb.zero_()
        scale = grad_scale / nsec      # the merged loss is the mean over the sectors
        heads = ps.flat_g[self._heads_lo:]
        self._iter_start.record()
        try:
            neck.begin(nsec)
            kept, det_losses, seg_losses = [], [], []
            for s, sec in enumerate(sectors):
                points = sec["points"]
                vi = self._index(points, None, batch, sec["grid_ind"])
                labels = None
                if point_labels is not None:
                    assert point_labels[s].numel() == points.shape[0], "point_labels must hold one label per row of points"
                    labels = ops.voxel_labels_from_points(point_labels[s], vi, dense=False, loss_labels=True).view(batch, spec.grid[1], spec.grid[0])
                elif voxel_labels is not None:
                    from .seg_heads import get_labels
                    assert voxel_labels[s].dim() == 4 and voxel_labels[s].shape[1] == 1, "voxel_labels must be (B, 1, H, W) per sector"
                    labels = get_labels(voxel_labels[s].squeeze(1), (spec.grid[1], spec.grid[0]))
                canvas = self._canvas(points, vi, batch)
                if s == 0:
                    self._prepack()     # issued behind the first scatter stage's launches, runs beside them
                x2 = neck.forward_sector(canvas)
                logits = seg.forward(canvas, x2) if with_seg else None
                head_train.forward(x2)
                losses = head_train.losses(targets[s])
                dlogits = None
                if with_seg:
                    sh = seg.head
                    sl, dlogits = sh.loss_func.loss_and_grad(ops.as_nchw(logits)[:, :sh.num_classes], labels, scale=float(sh.weight) * seg_scale * scale,
                                                             max_valid=max(int(vi.n_cap), 1))
                    seg_losses.append(sl)
                det_losses.append(losses[0] if len(losses) == 1 else torch.stack(losses))
                # the heads do not couple sectors: their backward runs here; d_x2 (and the seg head's canvas half) wait for the reverse pass
                self._packs_ready(2)
                d_x2 = head_train.backward(targets[s], losses, scale)
                if with_seg:
                    seg.backward_x2(dlogits, d_x2)
                    seg.backward_x1(dlogits, need_dx=False)
                if nsec > 1:      # the heads' parameter gradients, summed in sector order: ((g0 + g1) + g2) + ...
                    ps.side.join()
                    if s == 0:
                        self._heads_sum.copy_(heads)
                    elif s < nsec - 1:
                        ops.add(self._heads_sum, heads, out=self._heads_sum)
                    else:
                        ops.add(self._heads_sum, heads, out=heads)
                kept.append((points, vi, d_x2, dlogits))
            self._bucket_ready(0)   # every head gradient is complete: its exchange overlaps the backward of the neck

            def block_done(i):
                if i == self.last_block and len(self.buckets) > 2:
                    self._bucket_ready(1)

            d_canvas = neck.backward([k[2] for k in kept], block_done=block_done)
            r = self.reader
            for s in range(nsec - 1, -1, -1):
                points, vi, _, dlogits = kept[s]
                d_sec = d_canvas[s * batch:(s + 1) * batch]
                if dlogits is not None:
                    seg.backward_canvas(dlogits, d_sec)      # (the canvases of all sectors have one shape: the head's saved one stands for it)
                ops.dynamic_pfn_bwd(points, vi, ps.p[self.w0], ps.p[self.w1], r.vx, r.vy, r.x_offset, r.y_offset, d_canvas=d_sec, dw0=ps.g[self.w0],
                                    dw1=ps.g[self.w1], accumulate=s < nsec - 1, voxel_shape=r.voxel_shape)
            ps.side.join()
            self.vi = kept[-1][1]
            if with_seg:
                self.seg_loss = torch.stack(seg_losses)
            return torch.stack(det_losses)
        finally:
            ps.fresh = None
            self._pack_events = None

    def step(self, sectors, batch, targets, voxel_labels=None, seg_loss_scale=1.0, point_labels=None):
        return self._step(lambda scale: self.forward_backward(sectors, batch, targets, grad_scale=scale, voxel_labels=voxel_labels,
                                                              seg_loss_scale=seg_loss_scale, point_labels=point_labels))
