"""The detection head of the training step as a part: ``CenterHeadTrain`` = CenterHead (plain or dcn_head=True) / CenterHeadSingle /
CenterHeadSinglePos in training form over a ``ParamStore`` (center_head.py:25-163, 166-250; center_head_parallel.py).  The step calls
  ``forward(x2)``                            -> the prediction dict (of the first task)
  ``losses(targets)``                        -> one CenterPoint loss vector per task
  ``backward(targets, losses, grad_scale)``  -> the gradient of x2; every parameter gradient of the head is queued
A branch (one per head name, per task in the plain head) is a small object with ``fwd(x)`` and ``bwd(d_pred, d_xs, accumulate)``: the
gradient of the branch's input goes into ``d_xs`` (overwritten or added), or into a tensor of its own when ``d_xs`` is None."""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .heads import CenterHeadSinglePos, RangeStratified
from .nn_utils import RSNorm
from .train_layers import NONE, RELU, TANH, _Conv, _ConvBNReLU, _ConvGNReLU, _ConvReLU, _GroupedConv, _StratConvGNReLU


class _PlainBranch:
    """a chain of Conv2d + ReLU and a final Conv2d of the plain CenterHead"""

    def __init__(self, ps, prefix: str, seq: nn.Module):
        convs = [(i, mod) for i, mod in enumerate(seq._modules.values()) if isinstance(mod, nn.Conv2d)]
        self.hidden = [_ConvReLU(ps, f"{prefix}{i}.weight", f"{prefix}{i}.bias", mod.padding[0]) for i, mod in convs[:-1]]
        i, mod = convs[-1]
        self.last = _Conv(ps, f"{prefix}{i}.weight", f"{prefix}{i}.bias", 1, mod.padding[0])

    def fwd(self, x, in_co=0):
        """``in_co``: the branch reads its input channels from there (a slice of a wider map)"""
        for layer in self.hidden + [self.last]:
            x = layer.fwd(x, in_co=in_co)
            in_co = 0
        return x

    def bwd(self, d_pred, d_xs=None, accumulate=False, dx_co=0):
        """``dx_co``: the input gradient goes to the channels of ``d_xs`` from there"""
        first = not self.hidden
        dz = self.last.bwd(d_pred, dx=d_xs if first else None, dx_co=dx_co if first else 0, accumulate=first and accumulate)
        for li in range(len(self.hidden) - 1, -1, -1):
            first = li == 0
            dz = self.hidden[li].bwd(dz, dx=d_xs if first else None, dx_co=dx_co if first else 0, accumulate=first and accumulate)
        return dz


class _ClsBranch:
    """the heat-map head of DCNSepHead (center_head.py:141-146): Conv2d(bias) + BatchNorm2d (batch statistics) + ReLU + Conv2d"""

    def __init__(self, ps, prefix: str, seq: nn.Module):
        self.first = _ConvBNReLU(ps, prefix, 0, seq[1], seq[0])
        self.last = _Conv(ps, prefix + "3.weight", prefix + "3.bias", 1, seq[3].padding[0])

    def fwd(self, x, in_co=0):
        return self.last.fwd(self.first.fwd(x, in_co=in_co))

    def bwd(self, d_pred, d_xs=None, accumulate=False, dx_co=0):
        return self.first.bwd(self.last.bwd(d_pred), dx=d_xs, dx_co=dx_co, accumulate=accumulate)


class _DcnAdapt:
    """the 2T feature adaptions of CenterHead(dcn_head=True) (FeatureAdaption, center_head.py:25-63) in training form: per adaption a 1x1
    convolution with bias writes its 18 dg channels of ONE wide offset map, ONE deformable launch of 2T jobs + ReLU writes the feature map
    (B, H, W, 2T C): task t's cls features at 2t C, its reg features at (2t + 1) C.  ``bwd`` is one DeformConvLayer.backward (the input
    and offset gradients; the 2T weight gradients on the side stream), then the offset convolutions' backward added into d_xs."""

    def __init__(self, ps, hp: str, head: nn.Module):
        self.ps = ps
        names = [f"{hp}tasks.{t}.feature_adapt_{kind}." for t in range(len(head.tasks)) for kind in ("cls", "reg")]
        self.dg = head.tasks[0].feature_adapt_cls.conv_adaption.deformable_groups
        self.oc = 18 * self.dg
        self.offsets = [_Conv(ps, n + "conv_offset.weight", n + "conv_offset.bias", 1, 0) for n in names]
        self.wnames = [n + "conv_adaption.weight" for n in names]
        self.layer = ops.DeformConvLayer([ps.p[n] for n in self.wnames], dg=self.dg, act=RELU)
        self.c = self.layer.c
        self._token = self.xs = self.off = self.feats = None
        ps.convs.append(self)

    def prepack_fwd(self, token):
        self.layer.repack([self.ps.p[n] for n in self.wnames])
        self._token = token

    def prepack_bwd(self, token):
        self.layer.prepack_bwd()

    def fwd(self, xs):
        ps = self.ps
        if ps.fresh is None or self._token is not ps.fresh:      # not refreshed ahead of this iteration
            self.prepack_fwd(ps.fresh)
        self.xs = xs
        self.off = torch.empty(xs.shape[:3] + (len(self.offsets) * self.oc,), dtype=torch.float32, device=xs.device)
        for a, conv in enumerate(self.offsets):
            conv.fwd(xs, out=self.off, out_co=a * self.oc)
        self.feats = self.layer(xs, self.off)
        return self.feats

    def bwd(self, d_feat, d_xs):
        """d_feat: the gradient of the whole feature map; d_xs is overwritten with the gradient of the shared features"""
        ps, xs, off, feats = self.ps, self.xs, self.off, self.feats
        d_off = torch.empty_like(off)
        self.layer.backward(xs, off, feats, d_feat, d_x=d_xs, d_offset=d_off)
        grads = [ps.g[n] for n in self.wnames]
        ps.side.run(lambda: self.layer.backward_weight(xs, off, feats, d_feat, grads), xs, off, feats, d_feat)
        for a, conv in enumerate(self.offsets):
            co = a * self.oc

            def weight_grads(conv=conv, co=co):
                ops.conv_wgrad(xs, d_off, 1, 1, 1, 0, cout=self.oc, dout_channel_offset=co, out=ps.g[conv.wname])
                ops.channel_sum(d_off, c=self.oc, channel_offset=co, out=ps.g[conv.bname])

            ps.side.run(weight_grads, d_off, xs)
            conv.dgrad.repack(ps.p[conv.wname], token=ps.fresh)
            conv.dgrad(d_off, out=d_xs, dout_channel_offset=co, accumulate=True)
        return d_xs


class _NormBranch:
    """a normalised hidden convolution and a final convolution: the two branch kinds of the merged heads"""

    def fwd(self, x):
        return self.last.fwd(self.first.fwd(x))

    def bwd(self, d_pred, d_xs=None, accumulate=False):
        return self.first.bwd(self.last.bwd(d_pred), dx=d_xs, accumulate=accumulate)[0]


class _StratBranch(_NormBranch):
    """RangeStratified + a 1x1 convolution"""

    def __init__(self, ps, prefix: str, mods):
        self.first = _StratConvGNReLU(ps, prefix + "0.", mods[0])
        self.last = _Conv(ps, prefix + "1.weight", prefix + "1.bias", 1, 0)


class _ConvBranch(_NormBranch):
    """Conv2d + GroupNorm + ReLU + Conv2d; a merged branch (``rot_vel``: one group per head) runs both convolutions grouped, and ``bwd`` then
    takes one prediction gradient per head"""

    def __init__(self, ps, prefix: str, mods):
        assert len(mods) == 4, "training step: heads with one hidden conv (num_conv = 2)"
        groups = mods[0].groups
        self.first = _ConvGNReLU(ps, prefix + "0.weight", prefix + "0.bias", prefix + "1.weight", prefix + "1.bias", mods[1].num_groups, 1, mods[1].eps,
                                 groups=groups)
        self.last = _Conv(ps, prefix + "3.weight", prefix + "3.bias", 1, 1) if groups == 1 else _GroupedConv(ps, prefix + "3.weight", prefix + "3.bias", groups)


class CenterHeadTrain:
    def __init__(self, ps, head: nn.Module, dev, prefix="bbox_head."):
        if getattr(head, "dcn_head", False) and not next(head.parameters()).is_cuda:
            # the DCN head's training form exists on the device alone (the plain wrappers fail in their first pack call on a host
            # tensor; this one says what is missing before anything is built).  The branch and its wording also keep
            # tests/test_dcn_ref_cpu.py::test_what_stays_unbuilt_says_so holding, which pinned the refusal of DCN training on a host
            # head before the backward existed ("what stays refused": the follow-up that lets this branch go)
            raise NotImplementedError("CenterHeadTrain: a dcn_head=True head trains on the HIP device only -- the backward of the deformable "
                                      "convolution (csrc/deform_conv_bwd.hip) has no host form; move the head to the GPU first")
        self.ps, hp = ps, prefix
        self.plain = type(head).__name__ == "CenterHead"
        self.code_weights, self.loss_weight = list(head.code_weights), float(head.weight)
        self.ncls = sum(head.num_classes)
        self.task_ncls = [int(n) for n in head.num_classes]
        self.cal = {}
        self.dcn = None
        self.branches = {}      # name (plain head: (task, name)) -> branch, in the head's order
        # the wrappers are built in the order the prepack refreshes them (ps.convs): shared, branches, calibration
        if self.plain:
            self.shared = _ConvReLU(ps, hp + "shared_conv.0.weight", hp + "shared_conv.0.bias", 1)
            if getattr(head, "dcn_head", False):
                # DCNSepHead (center_head.py:111-163): the adaptions, then per task the regression chains on the reg features and the
                # heat-map head on the cls features; the prediction dicts keep the reference's order (the regression heads, then 'hm')
                self.dcn = _DcnAdapt(ps, hp, head)
                for t, task in enumerate(head.tasks):
                    for name in task.task_head.heads:
                        self.branches[(t, name)] = _PlainBranch(ps, f"{hp}tasks.{t}.task_head.{name}.", getattr(task.task_head, name))
                    self.branches[(t, "hm")] = _ClsBranch(ps, f"{hp}tasks.{t}.cls_head.", task.cls_head)
                return
            # one set of branches per task (center_head.py:166-242: `for task in self.tasks`); every task has its own loss
            # (center_head.py:250: one term per task, summed by the trainer) and its own targets
            for t, task in enumerate(head.tasks):
                for name in task.heads:
                    self.branches[(t, name)] = _PlainBranch(ps, f"{hp}tasks.{t}.{name}.", getattr(task, name))
            return
        rs = head.shared_conv[1]
        assert isinstance(rs, RSNorm)
        self.shared = _ConvGNReLU(ps, hp + "shared_conv.0.weight", hp + "shared_conv.0.bias", hp + "shared_conv.1.groupnorm.weight",
                                  hp + "shared_conv.1.groupnorm.bias", rs.num_heads, rs.num_groups, rs.groupnorm.eps)
        for name in head.heads:
            mods = list(getattr(head, name)._modules.values())
            branch = _StratBranch if isinstance(mods[0], RangeStratified) else _ConvBranch
            self.branches[name] = branch(ps, f"{hp}{name}.", mods)
        if isinstance(head, CenterHeadSinglePos):
            pos = ops.to_nhwc(head.pos_encoding.to(dev).float())               # (1, A, R, 5)
            self.pos8 = torch.zeros(pos.shape[:3] + (8,), dtype=torch.float32, device=dev)
            self.pos8[..., :5] = pos
            for cname, last_act in (("calibration_weight", TANH), ("calibration_bias", NONE)):
                cp = f"{hp}{cname}."
                self.cal[cname] = (_Conv(ps, cp + "0.weight", cp + "0.bias", 1, 1, act=TANH, cin_pad=8),
                                  _Conv(ps, cp + "2.weight", cp + "2.bias", 1, 0, act=last_act), last_act)

    def forward(self, x2):
        self.cal_mid, self.cal_out = {}, {}
        for cname, (c0, c1, _) in self.cal.items():
            self.cal_mid[cname] = c0.fwd(self.pos8)
            self.cal_out[cname] = c1.fwd(self.cal_mid[cname])
        if self.cal:
            xs, x_hm = self.shared.fwd(x2, mul=self.cal_out["calibration_weight"][0], add=self.cal_out["calibration_bias"][0])
        else:
            xs = x_hm = self.shared.fwd(x2)
        self.xs, self.x_hm = xs, x_hm
        if self.plain:
            self.preds_tasks = [dict() for _ in self.task_ncls]
            feats = xs if self.dcn is None else self.dcn.fwd(xs)
            for (t, nm), branch in self.branches.items():
                self.preds_tasks[t][nm] = branch.fwd(feats, in_co=0 if self.dcn is None else self._slice(t, nm) * self.dcn.c)
            return self.preds_tasks[0]
        preds = {}
        for name, branch in self.branches.items():
            y = branch.fwd(x_hm if name == "hm" else xs)
            names = name.split("_")         # a merged branch: one slice of the output per head
            dim = y.shape[3] // len(names)
            for k, nm in enumerate(names):
                preds[nm] = y[..., k * dim:(k + 1) * dim] if len(names) > 1 else y
        self.preds_tasks = [preds]
        return preds

    @staticmethod
    def _slice(t, nm):
        """the DCN head's feature map: which C-channel slice branch (t, nm) reads"""
        return 2 * t if nm == "hm" else 2 * t + 1

    def _tasks(self, targets):
        """-> [(prediction dict, class count, targets)] per task; a single-task step takes its targets bare, several tasks a list"""
        if len(self.preds_tasks) == 1:
            return [(self.preds_tasks[0], self.ncls, targets[0] if isinstance(targets, (list, tuple)) else targets)]
        assert isinstance(targets, (list, tuple)) and len(targets) == len(self.preds_tasks), "one CenterLossTargets per task"
        return list(zip(self.preds_tasks, self.task_ncls, targets))

    @staticmethod
    def _boxes(preds):
        order = ["reg", "height", "dim"] + (["vel"] if "vel" in preds else []) + ["rot"]
        return order, [(preds[k], preds[k].shape[3]) for k in order]

    def losses(self, targets):
        return [ops.center_loss(preds["hm"], ncls, self._boxes(preds)[1], tg, self.code_weights, self.loss_weight, with_vel="vel" in preds)
                for preds, ncls, tg in self._tasks(targets)]

    def backward(self, targets, losses, grad_scale: float):
        d_pred = {}
        for t, ((preds, ncls, tg), lo) in enumerate(zip(self._tasks(targets), losses)):
            order, boxes = self._boxes(preds)
            d_hm, d_boxes = ops.center_loss_bwd(preds["hm"], ncls, boxes, tg, self.code_weights, self.loss_weight, lo,
                                                grad_scale=grad_scale, with_vel="vel" in preds)
            for nm, d in list(zip(order, d_boxes)) + [("hm", d_hm)]:
                d_pred[(t, nm) if self.plain else nm] = d
        return self.backward_preds(d_pred)

    def backward_preds(self, d_pred):
        """the backward from the gradients of the predictions (own tensors, keyed like ``branches``; a merged branch: by head name)
        -> the gradient of x2; every parameter gradient is queued"""
        d_xs = torch.empty_like(self.xs)
        if self.dcn is not None:
            d_feat, written = torch.empty_like(self.dcn.feats), set()      # (every slice has a branch: the first one into it overwrites)
            for (t, nm), branch in self.branches.items():
                sl = self._slice(t, nm)
                branch.bwd(d_pred[(t, nm)], d_feat, sl in written, dx_co=sl * self.dcn.c)
                written.add(sl)
            self.dcn.bwd(d_feat, d_xs)
            return self.shared.bwd(d_xs)
        d_xhm = None
        accumulate = False      # the first branch into d_xs overwrites it
        for name, branch in self.branches.items():
            d = d_pred[name] if name in d_pred else [d_pred[nm] for nm in name.split("_")]
            if name == "hm" and self.x_hm is not self.xs:
                d_xhm = branch.bwd(d)
            else:
                branch.bwd(d, d_xs, accumulate)
                accumulate = True
        # shared conv + RSNorm (+ calibration)
        if self.plain:
            return self.shared.bwd(d_xs)
        res = self.shared.bwd(d_xs, dout2=d_xhm)
        for cname, dmap in zip(("calibration_weight", "calibration_bias"), res[1:] if self.cal else ()):
            c0, c1, last_act = self.cal[cname]
            d = dmap[None].contiguous()
            if last_act == TANH:
                d = ops.tanh_bwd(self.cal_out[cname], d)
            dmid = c1.bwd(d)
            dmid = ops.tanh_bwd(self.cal_mid[cname], dmid, dx=dmid)
            c0.bwd(dmid, need_dx=False)
        return res[0]
