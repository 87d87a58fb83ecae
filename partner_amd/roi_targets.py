"""The proposal targets of the CenterPoint second stage: ``ProposalTargetLayer`` under the reference's name.

Reference: det3d/models/roi_heads/target_assigner/proposal_target_layer.py:14-244 fused with ``RoIHeadTemplate.assign_targets``
(roi_head_template.py:43-86).  Two launches, `pn_roi_max_iou3d_f32` and `pn_roi_sample_targets_f32` (csrc/roi_train.hip): no per-sample Python
loop, nothing read back.  The reference draws its random picks inside the layer (np.random.permutation, np.random.rand, torch.randint);
here the draws are an INPUT -- uniform numbers in [0, 1) whose use include/partner_hip.h spells out -- so the targets are a pure function of
(inputs, draws) with the same distribution of picks, and the reference run on recorded draws is an exact yardstick
(tests/golden/make_golden_two_stage_train.py)."""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from . import hip, ops


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class ProposalTargetLayer(nn.Module):
    """``forward(batch_dict, u_fg=None, u_bg=None)``: batch_dict holds 'rois' (B, R, cs), 'roi_scores', 'roi_labels' (int64, 1-based, 0 in
    padding slots), 'roi_features' (B, R, F) -- what ``BEVFeatureExtractor.forward`` returns -- and 'gt_boxes_and_cls' (B, N, cs + 1)
    [x, y, z, w, l, h, rot, (vx, vy,) class] with zero rows at the end.  -> the reference's targets_dict ('rois', 'gt_of_rois' (encoded),
    'gt_iou_of_rois', 'roi_scores', 'roi_labels', 'roi_features', 'reg_valid_mask', 'rcnn_cls_labels', 'gt_of_rois_src') plus
    'sampled_inds' (B, M) int32, every tensor (B, M, ...) with M = ROI_PER_IMAGE.

    ``u_fg`` (B, R) / ``u_bg`` (B, M): the uniform draws; without them they come from ``torch.rand`` on the device with ``generator``
    (a ``torch.Generator`` of that device the caller seeds)."""

    def __init__(self, roi_sampler_cfg):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg
        score_type = _get(roi_sampler_cfg, "CLS_SCORE_TYPE")
        if score_type not in ops.ROI_SCORE_TYPES:
            raise NotImplementedError(f"ProposalTargetLayer: CLS_SCORE_TYPE {score_type!r} is not built; 'roi_iou' and 'cls' are")

    def forward(self, batch_dict, u_fg: Optional[torch.Tensor] = None, u_bg: Optional[torch.Tensor] = None,
                generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        cfg = self.roi_sampler_cfg
        rois, gt = batch_dict["rois"], batch_dict["gt_boxes_and_cls"]
        hip.require_device(rois, gt)
        b, r, cs = rois.shape
        by_class = bool(_get(cfg, "SAMPLE_ROI_BY_EACH_CLASS", False))
        if not by_class and cs == 9:
            raise NotImplementedError("ProposalTargetLayer: SAMPLE_ROI_BY_EACH_CLASS=False with code_size 9 is not built (the reference's own "
                                      "`assert boxes_a.shape[1] == 7`, iou3d_nms_utils.py:46, fails there)")
        m = int(_get(cfg, "ROI_PER_IMAGE"))
        if u_fg is None:
            u_fg = torch.rand((b, r), dtype=torch.float32, device=rois.device, generator=generator)
        if u_bg is None:
            u_bg = torch.rand((b, m), dtype=torch.float32, device=rois.device, generator=generator)
        gt = gt.contiguous()
        max_overlaps, gt_assignment = ops.roi_max_iou3d(rois, batch_dict["roi_labels"], gt, by_class)
        return ops.roi_sample_targets(rois, batch_dict["roi_labels"], batch_dict["roi_scores"], batch_dict["roi_features"], gt, max_overlaps, gt_assignment,
                                      u_fg, u_bg, m, _get(cfg, "FG_RATIO"), _get(cfg, "REG_FG_THRESH"), _get(cfg, "CLS_FG_THRESH"),
                                      _get(cfg, "CLS_BG_THRESH"), _get(cfg, "CLS_BG_THRESH_LO"), _get(cfg, "HARD_BG_RATIO"), _get(cfg, "CLS_SCORE_TYPE"))
