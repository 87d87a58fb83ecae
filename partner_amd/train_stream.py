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
``PolarStreamBDCPTrainStep``  ``PolarPillarTrainStep`` with that neck: reader, heads, losses, seg super-task, optimizer, schedule,
                       checkpoint and gradient buckets are the plain step's.  The previous sweep runs reader + neck in feature-only form
                       with nothing saved; the rows the streaming pass reads are warped by `pn_polar_warp_strips_f32`.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import hip, ops
from .necks_context import RPNBDCP
from .train import PolarPillarTrainStep, _ConvBNReLU

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
    """RPNBDCP in training form over a ``ParamStore`` (see the module text).  ``forward_prev`` = the previous sweep's feature-only pass,
    ``forward`` = the current sweep (all sectors), ``backward`` = its gradients."""

    def __init__(self, ps, neck: RPNBDCP):
        if not isinstance(neck, RPNBDCP):
            raise NotImplementedError("ContextNeckTrain: the neck must be an RPNBDCP")
        self.ps, self.neck = ps, neck
        mods = [cc for blk in neck.blocks for cc in blk._modules.values()]
        self.layers = [_CtxLayer(ps, names, cc) for names, cc in zip(context_layer_names(neck), mods)]
        self.block_of = [names["block"] for names in context_layer_names(neck)]
        self.deblocks = [_ConvBNReLU(ps, f"neck.deblocks.{j}.", 0, de[1], de[0]) for j, de in enumerate(neck.deblocks)]
        self.up_start = neck._upsample_start_idx
        self.up_filters = list(neck._num_upsample_filters)
        self.token = self._prev_token = None
        self.saved = self.de_saved = None

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
                    de = self.deblocks[j]
                    de.fwd(x)
                    de.conv.x = de.y = de.stat = None
        return cur

    def forward(self, canvas, nsectors: int, prev_sweep=()):
        """canvas (nsectors * bs, hs, w, c) stacked sector-major -> the stacked concatenated deblock outputs"""
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
                        self.de_saved[s][j] = (de.conv.x, de.conv.in_co, de.y, de.stat)
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
                        de.conv.x, de.conv.in_co, de.y, de.stat = self.de_saved[s][j]
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
        super().__init__(model, total_steps, **kw)
        g = self.spec.grid
        if g[1] % self.nsec:
            raise ValueError(f"the azimuth axis ({g[1]} cells) does not divide into {self.nsec} sectors")
        self.spec = ops.GridSpec(self.spec.lo, self.spec.vs, (g[0], g[1] // self.nsec, g[2]))      # one sector's canvas (detectors._canvas)
        self._prev = None

    def _build_rpn(self, neck):
        self.ctx_neck = ContextNeckTrain(self.ps, neck)
        self.blocks = [[] for _ in neck.blocks]       # the plain step's tables (its pack groups read them): the context layers pack on first use
        self.deblocks = self.ctx_neck.deblocks
        self.up_start = neck._upsample_start_idx
        self.up_filters = list(neck._num_upsample_filters)

    def _sparse_first(self):
        return None

    def _prev_canvas(self, prev, batch):
        """reader + scatter of the previous sweep: nothing kept (polarstream.py:318-336, under no_grad)"""
        spec, r, ps = self.spec, self.reader, self.ps
        keys = ops.keys_from_grid_ind(prev["grid_ind"].to(torch.int64).contiguous(), spec, batch)
        vi = ops.build_voxel_index(keys, spec, batch, n_dev=None, want_unq=False, sorted_runs=True)
        canvas = torch.empty((batch, spec.grid[1], spec.grid[0], r.out_channels), dtype=torch.float32, device=self.dev)
        hip.call("pn_fill_zero", canvas.data_ptr(), canvas.numel() * 4, hip.stream())
        ops.dynamic_pfn(prev["points"], vi, ps.p[self.w0], ps.p[self.w1], r.vx, r.vy, r.x_offset, r.y_offset, None, canvas)
        return canvas

    def _rpn_forward(self, canvas, batch):
        nsec = self.nsec
        assert batch % nsec == 0, "batch is the stacked count nsectors * bs"
        self._packs_ready(0)
        self._packs_ready(1)      # the deblocks' layouts are refreshed on the side stream; the context layers pack on first use
        strips = []
        if self._prev is not None:
            inputs = self.ctx_neck.forward_prev(self._prev_canvas(self._prev, batch), nsec)
            if nsec > 1:          # one sector pads circularly: the previous sweep's pass only moves the running statistics, as in the reference
                strips = self.model.warp_prev_strips(inputs, self._prev["transform_matrix"], batch // nsec)
        return self.ctx_neck.forward(canvas, nsec, strips)

    def _rpn_backward(self, d_x2):
        nblk = len(self.neck.blocks)

        def block_done(i):
            # a bucket is ready only once its gradients are complete: the neck's blocks are after sector 0's backward
            if i == nblk - 1 and len(self.buckets) > 2:
                self._bucket_ready(1)

        return self.ctx_neck.backward(d_x2, block_done=block_done)

    def _check_sweeps(self, prev, cur):
        hip.require_device(cur["points"], cur["grid_ind"])
        if self.nsec > 1:
            if prev is None:
                raise ValueError("several sectors stream against the previous sweep: prev = dict(points, grid_ind, transform_matrix)")
            hip.require_device(prev["points"], prev["grid_ind"])

    def forward_backward(self, prev, cur, batch, targets, grad_scale=1.0, voxel_labels=None, seg_loss_scale=1.0, point_labels=None):
        """-> the det loss vector; gradients in ``ps.flat_g``; ``self.seg_loss`` as in the plain step"""
        self._check_sweeps(prev, cur)
        self._prev = prev
        try:
            return self._forward_backward(cur["points"], None, batch, targets, grid_ind=cur["grid_ind"], grad_scale=grad_scale,
                                          voxel_labels=voxel_labels, seg_loss_scale=seg_loss_scale, point_labels=point_labels)
        finally:
            self._prev = None

    def step(self, prev, cur, batch, targets, voxel_labels=None, seg_loss_scale=1.0, point_labels=None):
        self._check_sweeps(prev, cur)
        self._prev = prev
        try:
            return super().step(cur["points"], None, batch, targets, grid_ind=cur["grid_ind"], voxel_labels=voxel_labels,
                                seg_loss_scale=seg_loss_scale, point_labels=point_labels)
        finally:
            self._prev = None


def synthetic_iteration(model, bs: int, points_per_sweep: int = 30000, seed: int = 0, angle: float = 0.03, max_objs: int = 500, n_pos: int = 20):
    """A synthetic two-sweep iteration shaped for ``PolarStreamBDCPTrainStep(model)`` (profiling tool, tests): ``bs`` polar sweeps per sweep
    slot split into the model's sectors on the device (``ops.split_polar_sectors``), an ego rotation, random CenterPoint targets on the
    head's map and, with a seg head, labels on ~70 % of the cells that hold points.
    -> (prev, cur, batch, targets, voxel_labels or None)"""
    import numpy as np
    from .utils import synth
    dev = next(model.parameters()).device
    nsec, reader = int(model.nsectors), model.reader
    rng_, vs = [float(v) for v in reader.pc_range], [float(v) for v in reader.voxel_size]
    batch = nsec * bs

    def sweep(base):
        sweeps = [synth.synth_sweep_polar(points_per_sweep + 100 * b, seed=base + b, rho_max=min(55.0, rng_[3] - 0.5)) for b in range(bs)]
        offs = torch.tensor(np.concatenate([[0], np.cumsum([len(s) for s in sweeps])]), dtype=torch.int32, device=dev)
        out, part, gi, _ = ops.split_polar_sectors(torch.from_numpy(np.concatenate(sweeps, 0)).to(dev), offs, bs, nsec, rng_, vs)
        po = part.cpu().numpy()
        n = int(po[batch])
        gi = gi[:n].clone()
        for k in range(batch):
            gi[int(po[k]):int(po[k + 1]), 0] = k                      # stacked sample index, sector-major
        return dict(points=out[:n].contiguous(), grid_ind=gi.contiguous())

    prev, cur = sweep(1000 + seed), sweep(2000 + seed)
    c, s = float(np.cos(angle)), float(np.sin(angle))
    prev["transform_matrix"] = torch.tensor([[[c, -s], [s, c]]] * bs, dtype=torch.float32, device=dev)
    spec = ops.GridSpec.from_range(rng_, vs)
    hs, w = spec.grid[1] // nsec, spec.grid[0]
    neck = model.neck
    factor = int(round(np.prod(neck._layer_strides[:neck._upsample_start_idx + 1]) / neck._upsample_strides[0]))      # canvas cells per head-map cell
    h2, w2 = hs // factor, w // factor
    r = np.random.default_rng(seed)
    ncls = sum(model.bbox_head.num_classes)
    hm = (r.uniform(0, 1, (batch, ncls, h2, w2)) ** 8).astype(np.float32)
    ind, mask = np.zeros((batch, max_objs), np.int64), np.zeros((batch, max_objs), np.uint8)
    cat, anno = np.zeros((batch, max_objs), np.int64), np.zeros((batch, max_objs, 10), np.float32)
    for b in range(batch):
        ind[b, :n_pos] = r.choice(h2 * w2, n_pos, replace=False)
        mask[b, :n_pos] = 1
        cat[b, :n_pos] = r.integers(0, ncls, n_pos)
        anno[b, :n_pos] = r.standard_normal((n_pos, 10)).astype(np.float32)
        hm[b, cat[b, :n_pos], ind[b, :n_pos] // w2, ind[b, :n_pos] % w2] = 1.0
    targets = ops.CenterLossTargets(torch.from_numpy(hm), torch.from_numpy(ind), torch.from_numpy(mask), torch.from_numpy(cat), torch.from_numpy(anno), dev)
    labels = None
    if getattr(model, "seg_head", None) is not None:
        cells = torch.unique(cur["grid_ind"][:, [0, 2, 3]], dim=0).cpu().numpy()
        pick = cells[r.uniform(0, 1, len(cells)) < 0.7]
        lab = np.zeros((batch, 1, hs, w), np.int64)
        lab[pick[:, 0], 0, pick[:, 1], pick[:, 2]] = r.integers(1, model.seg_head.num_classes + 1, len(pick))
        labels = torch.from_numpy(lab).to(dev)
    return prev, cur, batch, targets, labels
