"""Training of the CenterPoint second stage on a frozen first stage (the reference's four two-stage configs, ``freeze=True``).

Reference call stack: ``TwoStageDetector.forward(example, return_loss=True)`` (det3d/models/detectors/two_stage.py:154-193) ->
``RoIHead.forward(training=True)`` (roi_heads/roi_head.py:70-106) -> ``assign_targets`` / ``ProposalTargetLayer``
(roi_head_template.py:43-86, target_assigner/proposal_target_layer.py) -> ``get_loss`` (roi_head_template.py:88-151) -> ``combine_loss``
(two_stage.py:40-47), under autograd; the optimizer is every step's (train.FlatAdam).

``RoIHeadTrain``       the RoIHead on the reverse-mode tape of autodiff.py: every Conv1d + BatchNorm1d + ReLU is ``ad.linear`` +
                       ``ad.batchnorm_rows(training=True)`` (batch statistics over all B * M rows, the zero-feature padding rows included as in
                       the reference, and the running-statistics update), every Dropout ``ad.dropout`` where the reference puts it.  The two
                       biased final layers run with their rows zero-padded to 4 and pad4(code_size) (the token GEMM's n % 4 == 0) and land in
                       the (rows, 4 + pad4(code_size)) buffer `pn_roi_loss_f32` reads -- the layout ``RoIHead.rcnn_rows`` writes.  The pad
                       rows are no parameters: their gradient (zero: the loss kernel writes zeros into the pad columns) is dropped.
``TwoStageTrainStep``  one iteration: first stage in eval form without a tape (neck map, head, its loss dict, its device list),
                       `pn_roi_bev_gather_f32`, the proposal targets (roi_targets.ProposalTargetLayer), RoIHeadTrain, `pn_roi_loss_f32`,
                       the tape's backward, the gradient all-reduce (world_size > 1), FlatAdam.  Only ``roi_head.*`` trains.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import autodiff as ad
from . import hip, ops
from .roi_targets import ProposalTargetLayer
from .train import FlatAdam, OptimizerForwards, ParamStore
from .two_stage import RoIHead, TwoStageDetector, _get, _pad4

PREFIX = "roi_head."


def _prefixed_store(head: nn.Module, device) -> ParamStore:
    """the flat buffers of the RoIHead's parameters under the names they carry in the detector (``roi_head.*``): optimizer checkpoints
    then name them as the model's state_dict does"""
    ps = ParamStore(head, device)
    ps.names = [PREFIX + n for n in ps.names]
    ps.offsets = {PREFIX + n: v for n, v in ps.offsets.items()}
    ps.p = {PREFIX + n: v for n, v in ps.p.items()}
    ps.g = {PREFIX + n: v for n, v in ps.g.items()}
    return ps


class RoIHeadTrain:
    """``forward(t, feats, seed)``: (rows, input_channels) features -> the node of the (rows, 4 + pad4(code_size)) row buffer (rcnn_cls in
    column ``RoIHead.CLS_COL``, rcnn_reg from ``RoIHead.REG_COL``); ``collect()`` after ``t.backward()`` adds every parameter gradient into
    ``ps.g``.  ``dropouts``: (input, output) of every dropout of the last forward with p > 0, in layer order."""

    def __init__(self, ps: ParamStore, head: RoIHead, prefix: str = PREFIX):
        if head.num_class != 1:
            raise NotImplementedError("RoIHeadTrain: num_class != 1 is not built (one class-agnostic score per ROI, as in RoIHead's eval plan)")
        self.ps, self.head, self.prefix = ps, head, prefix
        self.width = RoIHead.REG_COL + _pad4(head.code_size)
        self._finals: List[Tuple[str, ad.Node, ad.Node, int]] = []
        self._tape: Optional[ad.Tape] = None

    def _branch(self, t: ad.Tape, P: Dict[str, ad.Node], name: str, x: ad.Node, seed: int, pad_rows: int = 0) -> ad.Node:
        seq = getattr(self.head, name)
        mods = list(seq)
        for i, m in enumerate(mods):
            key = f"{self.prefix}{name}.{i}."
            if isinstance(m, nn.Conv1d):
                w = P[key + "weight"]
                n_out, k = m.out_channels, m.in_channels
                if i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d):
                    x = ad.linear(t, x, t.reshaped(w, (n_out, k)), None)
                    x = ad.batchnorm_rows(t, x, mods[i + 1], P[f"{self.prefix}{name}.{i + 1}.weight"], P[f"{self.prefix}{name}.{i + 1}.bias"], training=True)
                else:      # the biased final layer, rows zero-padded to ``pad_rows``; the padded copies are plain nodes, not parameters
                    wp = torch.zeros((pad_rows, k), dtype=torch.float32, device=w.v.device)
                    bp = torch.zeros((pad_rows,), dtype=torch.float32, device=w.v.device)
                    wp[:n_out].copy_(w.v.view(n_out, k))
                    bp[:n_out].copy_(P[key + "bias"].v)
                    wn, bn = ad.Node(wp, None, None), ad.Node(bp, None, None)
                    self._finals.append((key, wn, bn, n_out))
                    x = ad.linear(t, x, wn, bn)
            elif isinstance(m, nn.Dropout):
                y = ad.dropout(t, x, float(m.p), seed + len(self.dropouts) + 1)
                if y is not x:
                    self.dropouts.append((x.v, y.v))
                x = y
        return x

    def forward(self, t: ad.Tape, feats: torch.Tensor, seed: int = 0) -> ad.Node:
        hip.require_device(feats)
        assert feats.dim() == 2 and feats.dtype == torch.float32 and feats.is_contiguous()
        self._finals, self.dropouts, self._tape = [], [], t
        P = {name: t.param(self.ps.p[name], name) for name in self.ps.names}
        shared = self._branch(t, P, "shared_fc_layer", t.const(feats), seed)
        cls = self._branch(t, P, "cls_layers", shared, seed, pad_rows=4)
        reg = self._branch(t, P, "reg_layers", shared, seed, pad_rows=_pad4(self.head.code_size))
        return ad.concat_channels(t, [cls, reg], self.width)

    def collect(self) -> None:
        """after ``t.backward()``: the gradients of the tape's leaves (and the final layers' own rows) added into ``ps.g``"""
        g = self.ps.g
        for leaf in self._tape.params:
            if leaf.g is not None:
                ops.add(g[leaf.name].view(-1), leaf.g.contiguous().view(-1), out=g[leaf.name].view(-1))
        for key, wn, bn, n_out in self._finals:
            if wn.g is not None:
                ops.add(g[key + "weight"].view(-1), wn.g[:n_out].contiguous().view(-1), out=g[key + "weight"].view(-1))
            if bn.g is not None:
                ops.add(g[key + "bias"].view(-1), bn.g[:n_out].contiguous().view(-1), out=g[key + "bias"].view(-1))
        self._tape = None


class TwoStageTrainStep(OptimizerForwards):
    """``step(example)``: one training iteration of a ``TwoStageDetector`` built with ``freeze=True``.  ``example``: whatever the model's
    ``forward`` takes, the first stage's targets (``hm``, ``anno_box``, ``ind``, ``mask``, ``cat``: its loss is computed and reported under
    ``freeze`` too, as in the reference) and ``gt_boxes_and_cls`` (B, N, 7 [+ 2 velocity] + 1) on the device.  Returns ``combine_loss``'s
    dict: the first stage's with the RoIHead's loss added to its total (``det_loss[0]``: the key the first stage's head writes;
    two_stage.py:41 reads 'loss', which no head of the reference returns), plus ``roi_reg_loss`` / ``roi_cls_loss``.  The roi terms are
    device tensors and nothing in the step synchronises with the host.

    ``forward_backward(example, u_fg=None, u_bg=None)``: everything but the optimizer; the gradients land in ``ps.flat_g``.  ``u_fg``
    (B, NMS_POST_MAXSIZE) / ``u_bg`` (B, ROI_PER_IMAGE): the sampler's draws (include/partner_hip.h); without them they come from a device
    generator seeded with (seed, iter), as the dropout masks are."""

    def __init__(self, model: nn.Module, total_steps: int, lr_max=0.003, moms=(0.95, 0.85), div_factor=10.0, pct_start=0.4, weight_decay=0.01,
                 max_norm=35.0, beta2=0.99, eps=1e-8, seed=0):
        if not isinstance(model, TwoStageDetector):
            raise NotImplementedError("TwoStageTrainStep: the model must be a TwoStageDetector")
        if not getattr(model, "freeze", False):
            raise NotImplementedError("TwoStageTrainStep: freeze=False is not built (it needs the backward of pn_roi_bev_gather_f32 and a training "
                                      "step of the plain PointPillars / VoxelNet first stage); the reference's two-stage configs set freeze=True")
        head = model.roi_head
        if head.num_class != 1:
            raise NotImplementedError("TwoStageTrainStep: num_class != 1 is not built")
        cfg = head.model_cfg
        loss_cfg, target_cfg = _get(cfg, "LOSS_CONFIG"), _get(cfg, "TARGET_CONFIG")
        if loss_cfg is None or target_cfg is None:
            raise ValueError("TwoStageTrainStep: the RoIHead's model_cfg must hold TARGET_CONFIG and LOSS_CONFIG")
        if _get(loss_cfg, "CLS_LOSS") != "BinaryCrossEntropy":
            raise NotImplementedError(f"TwoStageTrainStep: CLS_LOSS {_get(loss_cfg, 'CLS_LOSS')!r} is not built; 'BinaryCrossEntropy' is")
        if _get(loss_cfg, "REG_LOSS") != "L1":
            raise NotImplementedError(f"TwoStageTrainStep: REG_LOSS {_get(loss_cfg, 'REG_LOSS')!r} is not built; 'L1' is")
        if model.test_cfg is None:
            raise ValueError("TwoStageTrainStep: the detector needs its test_cfg (the first stage's boxes are decoded with it)")
        p0 = next(head.parameters())
        hip.require_device(p0)
        self.model, self.dev = model, p0.device
        self.weights = _get(loss_cfg, "LOSS_WEIGHTS")
        self.target_layer = ProposalTargetLayer(target_cfg)
        if not bool(_get(target_cfg, "SAMPLE_ROI_BY_EACH_CLASS", False)) and head.code_size == 9:
            raise NotImplementedError("TwoStageTrainStep: SAMPLE_ROI_BY_EACH_CLASS=False with code_size 9 is not built (the reference's own "
                                      "`assert boxes_a.shape[1] == 7`, iou3d_nms_utils.py:46, fails there)")
        self.ps = _prefixed_store(head, self.dev)
        self.opt = FlatAdam(self.ps, model, total_steps, lr_max, moms, div_factor, pct_start, weight_decay, max_norm, beta2, eps)
        self.head_train = RoIHeadTrain(self.ps, head)
        self.seed = int(seed)
        self.last_targets: Optional[Dict[str, torch.Tensor]] = None
        self.roi_loss: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------------------------------
    def _targets(self, example, u_fg, u_bg):
        m = self.model
        cs = m.roi_head.code_size
        if "gt_boxes_and_cls" not in example:
            raise KeyError("gt_boxes_and_cls: TwoStageTrainStep needs example['gt_boxes_and_cls'], (B, N, 7 [+ 2 velocity] + 1) rows "
                           "[x, y, z, w, l, h, rot, (vx, vy,) class] on the device, zero rows at the end")
        gt = example["gt_boxes_and_cls"]
        hip.require_device(gt)
        with torch.no_grad():
            preds, bev = m.single_det.two_stage_preds(example)
            one_stage = m.bbox_head.loss(example, preds, device_only=True)
            dets = m.bbox_head.predict(example, preds, m.test_cfg, device_only=True)
            batch = m.second_stage[0](dets, bev, m.num_point, cs, m.NMS_POST_MAXSIZE)
        if cs == 7 and gt.shape[2] != 8:          # drop the velocity (two_stage.py:170-172)
            gt = torch.cat([gt[:, :, :7], gt[:, :, -1:]], 2)
        batch["gt_boxes_and_cls"] = gt.float().contiguous()
        gen = None
        if u_fg is None or u_bg is None:
            gen = torch.Generator(device=self.dev)
            gen.manual_seed(self.seed * 7919 + self.iter)
        return one_stage, self.target_layer(batch, u_fg, u_bg, generator=gen)

    def forward_backward(self, example, u_fg=None, u_bg=None, grad_scale=1.0):
        """-> (the first stage's loss dict, loss (3,) = (rcnn_loss, rcnn_loss_cls, rcnn_loss_reg) on the device)"""
        head = self.model.roi_head
        one_stage, tg = self._targets(example, u_fg, u_bg)
        b, m, f = tg["roi_features"].shape
        t = ad.Tape()
        rows = self.head_train.forward(t, tg["roi_features"].view(b * m, f), seed=self.seed * 7919 + self.iter * 16)
        loss, d_rows = ops.roi_loss(rows.v, head.CLS_COL, head.REG_COL, head.code_size, tg["rcnn_cls_labels"], tg["gt_of_rois"], tg["reg_valid_mask"],
                                    list(_get(self.weights, "code_weights")), float(_get(self.weights, "rcnn_cls_weight")),
                                    float(_get(self.weights, "rcnn_reg_weight")))
        if grad_scale != 1.0:
            sc = torch.full((d_rows.shape[1],), float(grad_scale), dtype=torch.float32, device=d_rows.device)
            hip.call("pn_scale_channels_f32", d_rows.data_ptr(), sc.data_ptr(), d_rows.numel(), d_rows.shape[1], d_rows.data_ptr(), hip.stream())
        t.backward(rows, d_rows)
        hip.call("pn_fill_zero", self.ps.flat_g.data_ptr(), self.ps.flat_g.numel() * 4, hip.stream())
        self.head_train.collect()
        self.last_targets, self.roi_loss = tg, loss
        return one_stage, loss

    @staticmethod
    def combine_loss(one_stage, loss: torch.Tensor):
        """two_stage.py:40-47 on the device"""
        out = {k: list(v) for k, v in one_stage.items()}
        out["det_loss"][0] = ops.add(out["det_loss"][0].reshape(1), loss[0:1]).reshape(())
        out["roi_reg_loss"] = [loss[2] for _ in out["det_loss"]]
        out["roi_cls_loss"] = [loss[1] for _ in out["det_loss"]]
        return out

    def sync_initial_params(self):
        self.opt.sync_initial_params()

    def step(self, example, u_fg=None, u_bg=None):
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        one_stage, loss = self.forward_backward(example, u_fg, u_bg, grad_scale=1.0 / world)
        if world > 1:
            from .dist_utils import GradExchange
            ex = GradExchange(self.ps.flat_g, [(0, self.ps.total)])
            ex.ready(0)
            ex.finish()
        self.optimizer_step()
        return self.combine_loss(one_stage, loss)
