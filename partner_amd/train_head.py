"""The detection head of the training step as a part: ``CenterHeadTrain`` = CenterHead / CenterHeadSingle / CenterHeadSinglePos in training
form over a ``ParamStore`` (center_head.py:65-109, 166-250; center_head_parallel.py).  The step calls
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
from .train_layers import NONE, TANH, _Conv, _ConvGNReLU, _ConvReLU, _GroupedConv, _StratConvGNReLU


class _PlainBranch:
    """a chain of Conv2d + ReLU and a final Conv2d of the plain CenterHead"""

    def __init__(self, ps, prefix: str, seq: nn.Module):
        convs = [(i, mod) for i, mod in enumerate(seq._modules.values()) if isinstance(mod, nn.Conv2d)]
        self.hidden = [_ConvReLU(ps, f"{prefix}{i}.weight", f"{prefix}{i}.bias", mod.padding[0]) for i, mod in convs[:-1]]
        i, mod = convs[-1]
        self.last = _Conv(ps, f"{prefix}{i}.weight", f"{prefix}{i}.bias", 1, mod.padding[0])

    def fwd(self, x):
        for layer in self.hidden:
            x = layer.fwd(x)
        return self.last.fwd(x)

    def bwd(self, d_pred, d_xs=None, accumulate=False):
        first = not self.hidden
        dz = self.last.bwd(d_pred, dx=d_xs if first else None, accumulate=first and accumulate)
        for li in range(len(self.hidden) - 1, -1, -1):
            first = li == 0
            dz = self.hidden[li].bwd(dz, dx=d_xs if first else None, accumulate=first and accumulate)
        return dz


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


def refuse_dcn_training(head: nn.Module, what: str) -> None:
    """CenterHead(dcn_head=True) runs inference only: the deformable convolution has a forward kernel (csrc/deform_conv.hip) and no backward"""
    if getattr(head, "dcn_head", False):
        raise NotImplementedError(f"{what}: dcn_head=True is not trained -- the backward of the deformable convolution (col2im into the input "
                                  "gradient and the offset gradient, deform_conv_cuda_kernel.cu:279-465) is not built")


class CenterHeadTrain:
    def __init__(self, ps, head: nn.Module, dev, prefix="bbox_head."):
        refuse_dcn_training(head, "CenterHeadTrain")
        self.ps, hp = ps, prefix
        self.plain = type(head).__name__ == "CenterHead"
        self.code_weights, self.loss_weight = list(head.code_weights), float(head.weight)
        self.ncls = sum(head.num_classes)
        self.task_ncls = [int(n) for n in head.num_classes]
        self.cal = {}
        self.branches = {}      # name (plain head: (task, name)) -> branch, in the head's order
        # the wrappers are built in the order the prepack refreshes them (ps.convs): shared, branches, calibration
        if self.plain:
            self.shared = _ConvReLU(ps, hp + "shared_conv.0.weight", hp + "shared_conv.0.bias", 1)
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
            for (t, nm), branch in self.branches.items():
                self.preds_tasks[t][nm] = branch.fwd(xs)
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
        d_xs = torch.empty_like(self.xs)
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
