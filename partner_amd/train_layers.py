"""Layer wrappers of the training steps (train.py, train_head.py, train_stream.py): a convolution (+ norm + activation) over the parameters
of a ``ParamStore`` with an explicit backward.  ``fwd`` keeps what ``bwd`` needs; ``bwd`` queues the parameter gradients on the store's
side stream and returns the data gradient.  A wrapper that appends itself to ``ps.convs`` has its packed weight layouts refreshed ahead of
the iteration (``prepack_fwd`` / ``prepack_bwd``, PolarPillarTrainStep._prepack); its own ``repack`` calls then see the iteration's token
(``ps.fresh``) and do nothing."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import ops
from .heads import RangeStratified
from .routes import R

RELU, NONE, TANH = ops.ACT_RELU, ops.ACT_NONE, ops.ACT_TANH


class _Conv:
    """plain convolution (optional bias, optional fused activation) with explicit backward"""

    def __init__(self, ps, wname: str, bname: Optional[str], stride=1, pad=0, act=NONE, transposed=False, cin_pad: Optional[int] = None):
        self.ps, self.wname, self.bname = ps, wname, bname
        w = ps.p[wname]
        self.stride, self.pad, self.act, self.transposed = stride, pad, act, transposed
        self.k = w.shape[2]
        if transposed:  # ConvTranspose2d(k=2, s=2): weight (Cin, Cout, 2, 2)
            self.layer = ops.ConvLayer(w, deconv2x2=True, act=act)
            # its data gradient is the stride-2 convolution with the same tensor read as (Cout_conv, Cin_conv, 2, 2)
            self.dgrad = ops.ConvLayer(w, stride=2, pad=0)
        else:
            self.layer = ops.ConvLayer(w, stride=stride, pad=pad, shift=None if bname is None else ps.p[bname], act=act, wino4=R.train_wino4_max_pixels > 0)
            self.layer.wino4_max_pixels = R.train_wino4_max_pixels
            if cin_pad is not None:
                self.layer.pad_input_channels(cin_pad)
            self.dgrad = ops.ConvDgrad(w, stride, pad)
        self.cin_real = w.shape[1] if not transposed else w.shape[0]
        self.x = None
        self.in_co = 0
        ps.convs.append(self)

    def prepack_fwd(self, token):
        self.layer.repack(self.ps.p[self.wname], None if self.bname is None else self.ps.p[self.bname], token=token)
        self.layer.prepack_used()

    def prepack_bwd(self, token):
        self.dgrad.repack(self.ps.p[self.wname], token=token)
        self.dgrad.prepack_used()

    def _chain_ok(self, t, layer) -> bool:
        return (R.train_chain_max_pixels > 0 and not self.transposed and self.k == 3 and self.stride == 1 and self.pad == 1
                and t.shape[1] * t.shape[2] <= R.train_chain_max_pixels and t.shape[3] == layer.cin
                and ops.conv_chain_supported([layer], t.shape[0], t.shape[1], t.shape[2]))

    def fwd(self, x, out=None, out_co=0, in_co=0):
        w = self.ps.p[self.wname]
        self.layer.repack(w, None if self.bname is None else self.ps.p[self.bname], token=self.ps.fresh)
        self.x, self.in_co = x, in_co
        if out is None and in_co == 0 and self._chain_ok(x, self.layer):
            return ops.conv_chain([self.layer], x)
        return self.layer(x, out=out, out_channel_offset=out_co, in_channel_offset=in_co)

    def bwd(self, dout, cout: Optional[int] = None, need_dx=True, dx=None, dx_co=0, accumulate=False, wacc=False):
        """dout: NHWC gradient of the (pre-activation) output, own tensor (channel offset 0).  ``wacc``: ADD the parameter gradients (a layer
        called several times per iteration: the sector calls of the streaming necks)"""
        w = self.ps.p[self.wname]
        gw = self.ps.g[self.wname]
        if self.transposed:
            self.ps.side.run(lambda: ops.conv_wgrad(dout, self.x, 2, 2, 2, 0, cout=w.shape[0], dout_channel_offset=self.in_co, out=gw, accumulate=wacc),
                             dout, self.x)
        else:
            cout = w.shape[0] if cout is None else cout

            def weight_grads():
                ops.conv_wgrad(self.x, dout, self.k, self.k, self.stride, self.pad, cin=self.cin_real, in_channel_offset=self.in_co,
                               cout=cout, out=gw, accumulate=wacc)
                if self.bname is not None:
                    ops.channel_sum(dout, c=cout, out=self.ps.g[self.bname], accumulate=wacc)

            self.ps.side.run(weight_grads, dout, self.x)
        if need_dx:
            self.dgrad.repack(w, token=self.ps.fresh)
            return self.dgrad(dout, out=dx, out_channel_offset=dx_co, accumulate=accumulate)
        return None


class _PillarConv:
    """the first convolution of the RPN on the sparse pillar canvas (ops.PillarConvLayer, csrc/pillar_conv.hip): forward over the
    (pillar, tap) pairs, data gradient straight to d(pillar features), weight gradient over the pairs -- the dense forms spend
    2.2 ms of a bs = 4 iteration on a map that is 89 % zeros.  ``vi`` (the iteration's VoxelIndex) is set before ``fwd``."""

    def __init__(self, ps, wname: str, stride: int):
        self.ps, self.wname = ps, wname
        self.layer = ops.PillarConvLayer(ps.p[wname], stride)
        self.vi = self.x = self.tables = None
        ps.convs.append(self)

    def prepack_fwd(self, token):
        self.layer.repack(self.ps.p[self.wname], token=token)

    def prepack_bwd(self, token):
        pass

    def fwd(self, x, out=None, out_co=0, in_co=0):
        assert out is None and in_co == 0
        self.layer.repack(self.ps.p[self.wname], token=self.ps.fresh)
        self.x = x
        self.tables = self.layer.build_tables(self.vi, x.shape[0], x.shape[1], x.shape[2])
        return self.layer.forward_tables(x, self.vi, self.tables)

    def bwd(self, dout, cout=None, need_dx=True, dx=None, dx_co=0, accumulate=False, wacc=False):
        """-> d(pillar features) (n_cap, Cin) instead of a dense canvas gradient (dynamic_pfn_bwd takes either)"""
        assert not wacc, "the pillar-rows first layer is called once per iteration"
        self.ps.side.run(lambda: self.layer.wgrad(self.x, dout, self.vi, self.tables, out=self.ps.g[self.wname]), dout, self.x, self.tables)
        return self.layer.dgrad_features(dout, self.vi, self.tables) if need_dx else None


class _GroupedConv:
    """3x3 / pad 1 convolution with ``groups > 1`` and a bias: forward in one launch, backward per group on weight / channel slices.  It takes
    no prepack token (it is not in ``ps.convs``): every call packs the layout it takes."""

    def __init__(self, ps, wname: str, bname: str, groups: int):
        self.ps, self.wname, self.bname, self.groups = ps, wname, bname, groups
        w = ps.p[wname]
        self.cg, self.cin_g = w.shape[0] // groups, w.shape[1]        # output / input channels of one group
        self.layer = ops.ConvLayer(w, stride=1, pad=1, groups=groups, shift=ps.p[bname])
        self.dgrads = [ops.ConvDgrad(w[g * self.cg:(g + 1) * self.cg], 1, 1) for g in range(groups)]
        self.x = None

    def fwd(self, x):
        self.x = x
        self.layer.repack(self.ps.p[self.wname], self.ps.p[self.bname])
        return self.layer(x)

    def bwd(self, dout, dx=None, accumulate=False):
        """dout: the output's gradient as ONE map over all groups' channels, or one map per group, each at channel offset 0 (the loss's
        per-head gradients of a merged branch, zero pad channels included) -> dx over all groups' input channels"""
        ps, x, cg, cin_g = self.ps, self.x, self.cg, self.cin_g
        w, gw, gb = ps.p[self.wname], ps.g[self.wname], ps.g[self.bname]
        whole = torch.is_tensor(dout)
        if whole:
            def weight_grads():
                ops.channel_sum(dout, out=gb)
                for g in range(self.groups):
                    ops.conv_wgrad(x, dout, 3, 3, 1, 1, cin=cin_g, in_channel_offset=g * cin_g, cout=cg, dout_channel_offset=g * cg,
                                   out=gw[g * cg:(g + 1) * cg])

            ps.side.run(weight_grads, dout, x)
        if dx is None:
            dx = torch.empty_like(x)
        for g in range(self.groups):
            dy, rows = dout if whole else dout[g], slice(g * cg, (g + 1) * cg)
            if not whole:
                def weight_grads(dy=dy, g=g, rows=rows):
                    ops.conv_wgrad(x, dy, 3, 3, 1, 1, cin=cin_g, in_channel_offset=g * cin_g, cout=cg, out=gw[rows])
                    ops.channel_sum(dy, c=cg, out=gb[rows])

                ps.side.run(weight_grads, dy, x)
            self.dgrads[g].repack(w[rows])
            self.dgrads[g](dy, out=dx, dout_channel_offset=g * cg if whole else 0, out_channel_offset=g * cin_g, accumulate=accumulate)
        return dx


class _ConvBNReLU:
    """Conv2d / ConvTranspose2d + BatchNorm2d (batch statistics) + ReLU  (rpn.py:124-142, 80-110: no bias; the heat-map head of DCNSepHead,
    center_head.py:141-146: a convolution WITH a bias -- the batch mean takes it out again, so its gradient, the channel sum of the
    BatchNorm backward's output, is zero up to rounding)"""

    def __init__(self, ps, prefix: str, conv_idx: int, bn: nn.BatchNorm2d, conv: nn.Module):
        transposed = isinstance(conv, nn.ConvTranspose2d)
        pad = 1 if conv.kernel_size[0] == 3 else 0  # nn.ZeroPad2d(1) + Conv2d(3, padding=0) == padding 1
        bias = f"{prefix}{conv_idx}.bias" if getattr(conv, "bias", None) is not None else None
        self.conv = _Conv(ps, f"{prefix}{conv_idx}.weight", bias, conv.stride[0], pad, NONE, transposed)
        self.gname, self.bname = f"{prefix}{conv_idx + 1}.weight", f"{prefix}{conv_idx + 1}.bias"
        self.ps, self.bn = ps, bn
        self.y = self.stat = None

    def fwd(self, x, out=None, out_co=0, in_co=0):
        self.y = self.conv.fwd(x, in_co=in_co)
        res, self.stat = ops.batchnorm_train(self.y, self.ps.p[self.gname], self.ps.p[self.bname], self.bn.eps, self.bn.momentum,
                                             self.bn.running_mean, self.bn.running_var, act=RELU, out=out, out_channel_offset=out_co)
        return res

    def take_saved(self):
        """what ``fwd`` saved for ``bwd`` (the convolution's input and its channel offset, the convolution's output, the statistics) as one
        value; the wrapper forgets it.  For a layer called several times per iteration: ``restore`` the call's value before its ``bwd``."""
        saved = (self.conv.x, self.conv.in_co, self.y, self.stat)
        self.conv.x = self.y = self.stat = None
        return saved

    def restore(self, saved):
        self.conv.x, self.conv.in_co, self.y, self.stat = saved

    def bwd(self, dout, dout_co=0, need_dx=True, dx=None, accumulate=False, wacc=False, dx_co=0):
        c = self.y.shape[3]
        inplace = dout.shape[3] == c and dout_co == 0
        dy = dout if inplace else torch.empty_like(self.y)
        ops.batchnorm_bwd(self.y, dout, self.ps.p[self.gname], self.ps.p[self.bname], self.stat, act=RELU, dx=dy,
                          dgamma=self.ps.g[self.gname], dbeta=self.ps.g[self.bname], dout_channel_offset=dout_co, accumulate=wacc)
        return self.conv.bwd(dy, need_dx=need_dx, dx=dx, dx_co=dx_co, accumulate=accumulate, wacc=wacc)


class _ConvReLU:
    """Conv2d(bias) + ReLU of the plain CenterHead (center_head.py:65-109, 166-242)"""

    def __init__(self, ps, wname: str, bname: str, pad: int):
        self.conv = _Conv(ps, wname, bname, 1, pad, act=RELU)
        self.z = None

    def fwd(self, x, in_co=0):
        self.z = self.conv.fwd(x, in_co=in_co)   # ReLU fused into the epilogue; its output is also the backward mask
        return self.z

    def bwd(self, dout, dx=None, accumulate=False, dx_co=0):
        dy = ops.relu_bwd(self.z, dout, dx=dout)
        return self.conv.bwd(dy, dx=dx, dx_co=dx_co, accumulate=accumulate)


class _ConvGNReLU:
    """Conv2d(bias) + GroupNorm-family + ReLU (+ calibration second output) of the merged heads and of RPNUber's memory modules.  ``pad``:
    the convolution's padding (its kernel is the weight's: 3x3 / pad 1 in the heads, also 1x1 / pad 0 in the memory modules)"""

    def __init__(self, ps, wname, bname, gname, bename, cgroups, strata, eps, groups=1, pad=1):
        self.ps = ps
        self.cgroups, self.strata, self.eps = cgroups, strata, eps
        self.gname, self.bename = gname, bename
        assert groups == 1 or pad == 1, "the grouped convolution is 3x3 / pad 1"
        self.conv = _Conv(ps, wname, bname, 1, pad) if groups == 1 else _GroupedConv(ps, wname, bname, groups)
        self.y = None

    def fwd(self, x, mul=None, add=None):
        self.y = self.conv.fwd(x)
        self.mul = mul
        self.stat = torch.empty(2 * self.y.shape[0] * self.strata * self.cgroups, dtype=torch.float32, device=self.y.device)
        return ops.groupnorm_strat(self.y, self.cgroups, self.strata, self.ps.p[self.gname], self.ps.p[self.bename], self.eps,
                                   act=RELU, mul=mul, add=add, stat_out=self.stat)

    def bwd(self, dout, dout2=None, dx=None, accumulate=False, need_dx=True):
        """-> (dx,) or, with ``dout2`` (the gradient of the calibrated second output), (dx, dmul, dadd).  ``need_dx=False`` (ungrouped): the
        parameter gradients only; ``dout`` then holds the convolution's output gradient and dx is None"""
        res = ops.groupnorm_strat_bwd(self.y, dout, self.cgroups, self.strata, self.ps.p[self.gname], self.ps.p[self.bename], self.eps,
                                      RELU, dout2=dout2, mul=self.mul if dout2 is not None else None, dx=dout,
                                      dgamma=self.ps.g[self.gname], dbeta=self.ps.g[self.bename], stat=self.stat)
        extra = res[3:] if dout2 is not None else ()
        if not need_dx:
            return (self.conv.bwd(res[0], need_dx=False),) + tuple(extra)
        return (self.conv.bwd(res[0], dx=dx, accumulate=accumulate),) + tuple(extra)


class _StratConvGNReLU:
    """RangeStratified: per-range-stratum 3x3 convolution + GroupNorm(strata) + ReLU (center_head_parallel.py:27-59)"""

    def __init__(self, ps, prefix: str, m: RangeStratified):
        self.ps, self.strata, self.nheads = ps, m.ngroups * m.nheads, m.nheads
        self.wname, self.bname = prefix + "conv.0.weight", prefix + "conv.0.bias"
        self.gname, self.bename = prefix + "conv.1.weight", prefix + "conv.1.bias"
        self.eps = m.conv[1].eps
        w = ps.p[self.wname]
        self.layer = ops.ConvLayer(w, stride=1, pad=1, range_strata=self.strata, shift=ps.p[self.bname])
        # r4: gradients at the convolution's own multiply-add count (ops.StratConvDgrad, pn_conv2d_wgrad_f32 with range_strata); r3
        # expanded dy to strata * C channels and ran ordinary gradient convolutions over the zeros: 1.0 ms of a 14 ms iteration
        self.masked = not R.train_strat_expand
        self.dgrad = ops.StratConvDgrad(w, self.strata) if self.masked else ops.ConvDgrad(w, 1, 1)
        self.x = self.y = None
        ps.convs.append(self)

    def prepack_fwd(self, token):
        self.layer.repack(self.ps.p[self.wname], self.ps.p[self.bname], token=token)
        self.layer.prepack_used()

    def prepack_bwd(self, token):
        self.dgrad.repack(self.ps.p[self.wname], token=token)
        self.dgrad.prepack_used()

    def fwd(self, x):
        self.x = x
        self.layer.repack(self.ps.p[self.wname], self.ps.p[self.bname], token=self.ps.fresh)
        self.y = self.layer(x)
        self.stat = torch.empty(2 * self.y.shape[0] * self.strata * self.nheads, dtype=torch.float32, device=self.y.device)
        return ops.groupnorm_strat(self.y, self.nheads, self.strata, self.ps.p[self.gname], self.ps.p[self.bename], self.eps, act=RELU,
                                   stat_out=self.stat)

    def bwd(self, dout, dx=None, accumulate=False):
        """-> (dx,), as _ConvGNReLU.bwd"""
        dy, _, _ = ops.groupnorm_strat_bwd(self.y, dout, self.nheads, self.strata, self.ps.p[self.gname], self.ps.p[self.bename], self.eps,
                                           RELU, dx=dout, dgamma=self.ps.g[self.gname], dbeta=self.ps.g[self.bename], stat=self.stat)
        if self.masked:
            def weight_grads():
                ops.conv_wgrad(self.x, dy, 3, 3, 1, 1, out=self.ps.g[self.wname], range_strata=self.strata)
                ops.strat_channel_sum(dy, self.strata, self.ps.g[self.bname])
        else:
            dy = ops.strat_expand(dy, self.strata)  # zeros outside the pixel's stratum: an ordinary conv gradient (the r3 form)

            def weight_grads():
                ops.conv_wgrad(self.x, dy, 3, 3, 1, 1, out=self.ps.g[self.wname])
                ops.channel_sum(dy, out=self.ps.g[self.bname])

        self.ps.side.run(weight_grads, dy, self.x)
        self.dgrad.repack(self.ps.p[self.wname], token=self.ps.fresh)
        return (self.dgrad(dy, out=dx, accumulate=accumulate),)
